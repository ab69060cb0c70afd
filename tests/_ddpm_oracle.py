"""The DDPM U-Net forward restated in plain PyTorch ops, written from the architecture's description (Ho et al. 2020 as the
`ddpm` model family arranges it), for checking the HIP program where no reference output is stored (the 256-px configs).

Functional: `ddpm_forward(cfg, sd, x, labels, dtype)` reads a state dict with the family's parameter names
(`all_modules.<i>.<Leaf>`) and walks it with a running module index, so the only thing it shares with the package under
test is that naming.  tests/test_ddpm_cpu.py pins it to the reference's stored outputs (tests/golden/unet_*_ddpm*.npz).
"""
import math

import torch
import torch.nn.functional as F


def _swish(v):
    return v * torch.sigmoid(v)


class _Walker:
    def __init__(self, sd, dtype):
        self.sd, self.dtype, self.i = sd, dtype, 0

    def p(self, leaf):
        return self.sd["all_modules.%d.%s" % (self.i, leaf)].to(self.dtype)

    def has(self, leaf):
        return "all_modules.%d.%s" % (self.i, leaf) in self.sd

    def next(self):
        self.i += 1


def _gn(w, prefix, v):
    return F.group_norm(v, 32, w.p(prefix + "weight"), w.p(prefix + "bias"), eps=1e-6)


def _nin(w, name, v):
    # per-pixel linear map with a [in, out] matrix
    return torch.einsum("bihw,io->bohw", v, w.p(name + ".W")) + w.p(name + ".b")[None, :, None, None]


def _res_block(w, v, temb):
    h = F.conv2d(_swish(_gn(w, "GroupNorm_0.", v)), w.p("Conv_0.weight"), w.p("Conv_0.bias"), padding=1)
    if temb is not None:
        h = h + F.linear(_swish(temb), w.p("Dense_0.weight"), w.p("Dense_0.bias"))[:, :, None, None]
    h = F.conv2d(_swish(_gn(w, "GroupNorm_1.", h)), w.p("Conv_1.weight"), w.p("Conv_1.bias"), padding=1)
    if w.has("NIN_0.W"):
        v = _nin(w, "NIN_0", v)
    w.next()
    return v + h


def _attn_block(w, v):
    b, c, hh, ww = v.shape
    h = _gn(w, "GroupNorm_0.", v)
    q, k, val = (_nin(w, n, h).reshape(b, c, hh * ww) for n in ("NIN_0", "NIN_1", "NIN_2"))
    att = torch.softmax(torch.einsum("bcq,bck->bqk", q, k) * (c ** -0.5), dim=-1)
    o = torch.einsum("bqk,bck->bcq", att, val).reshape(b, c, hh, ww)
    o = _nin(w, "NIN_3", o)
    w.next()
    return v + o


def timestep_embedding(labels, dim, dtype):
    half = dim // 2
    freqs = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000.0) / (half - 1))).to(dtype)
    arg = labels.to(dtype)[:, None] * freqs[None, :]
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)


def ddpm_forward(cfg, sd, x, labels, dtype=torch.float32):
    m = cfg.model
    nf, ch_mult, nrb = m.nf, tuple(m.ch_mult), m.num_res_blocks
    attn_res, with_conv = tuple(m.attn_resolutions), m.resamp_with_conv
    nres = len(ch_mult)
    w = _Walker(sd, dtype)
    x = x.to(dtype)
    temb = None
    if m.conditional:
        temb = timestep_embedding(labels, nf, dtype)
        temb = F.linear(temb, w.p("weight"), w.p("bias")); w.next()
        temb = F.linear(_swish(temb), w.p("weight"), w.p("bias")); w.next()
    h = x if cfg.data.centered else 2.0 * x - 1.0
    h = F.conv2d(h, w.p("weight"), w.p("bias"), padding=1); w.next()
    skips = [h]
    for lvl in range(nres):
        for _ in range(nrb):
            h = _res_block(w, skips[-1], temb)
            if h.shape[-1] in attn_res:
                h = _attn_block(w, h)
            skips.append(h)
        if lvl != nres - 1:
            h = skips[-1]
            if with_conv:
                # one zero row below and one zero column to the right, then a stride-2 convolution without padding
                h = F.conv2d(F.pad(h, (0, 1, 0, 1)), w.p("Conv_0.weight"), w.p("Conv_0.bias"), stride=2)
            else:
                h = F.avg_pool2d(h, 2)
            w.next()
            skips.append(h)
    h = skips[-1]
    h = _res_block(w, h, temb)
    h = _attn_block(w, h)
    h = _res_block(w, h, temb)
    for lvl in reversed(range(nres)):
        for _ in range(nrb + 1):
            h = _res_block(w, torch.cat([h, skips.pop()], dim=1), temb)
        if h.shape[-1] in attn_res:
            h = _attn_block(w, h)
        if lvl != 0:
            h = h.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)          # nearest neighbour x2
            if with_conv:
                h = F.conv2d(h, w.p("Conv_0.weight"), w.p("Conv_0.bias"), padding=1)
            w.next()
    assert not skips
    h = _swish(F.group_norm(h, 32, w.p("weight"), w.p("bias"), eps=1e-6)); w.next()
    h = F.conv2d(h, w.p("weight"), w.p("bias"), padding=1); w.next()
    assert w.i == 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("all_modules."))
    if m.scale_by_sigma:
        h = h / sd["sigmas"].to(dtype)[labels.long()][:, None, None, None]
    return h
