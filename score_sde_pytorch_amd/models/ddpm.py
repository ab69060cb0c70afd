"""DDPM score network (Ho et al. 2020), MI355X-native.

Drop-in for the reference's `models.ddpm.DDPM` (models/ddpm.py:39-181): same constructor
(`DDPM(config)`), same `forward(x[B,C,H,W], labels[B])`, same `all_modules` ordering and
parameter names, so reference checkpoints load with `strict=True`.

As in ncsnpp.py the modules are parameter containers that describe themselves to
`score_sde_pytorch_amd.engine`, which lowers the forward to one program of HIP kernels;
there is no PyTorch-eager forward.  What the family has that NCSN++ lacks is one
convolution form: `Downsample(with_conv=True)` pads one zero row and column at the bottom /
right only (models/layers.py:608-611), which runs as a single end-padded stride-2 launch
(`ssde_conv_args.pad_end`).
"""
import torch
import torch.nn as nn

from . import utils
from .ncsnpp import HipUNet, NIN, _conv, _dense

GROUPS = 32     # nn.GroupNorm(num_groups=32) everywhere (models/layers.py:562,625,633; ddpm.py:104)


def _group_norm(ch):
    # the GroupNorm prologue of the kernels normalises four channels per lane: a group must be a whole number of quads
    if ch % GROUPS != 0 or (ch // GROUPS) % 4 != 0:
        raise NotImplementedError("DDPM: GroupNorm(32 groups) over %d channels gives groups of %s channels; the HIP path needs a "
                                  "multiple of 4 (nf a multiple of 128)" % (ch, ch / GROUPS))
    return nn.GroupNorm(num_groups=GROUPS, num_channels=ch, eps=1e-6)


class AttnBlock(nn.Module):
    """GroupNorm -> q,k,v NIN -> softmax(q k / sqrt(C)) v -> NIN -> x + h (models/layers.py:558-581)."""
    kind = "attn"
    skip_rescale = False

    def __init__(self, channels):
        super().__init__()
        self.GroupNorm_0 = _group_norm(channels)
        self.NIN_0 = NIN(channels, channels)
        self.NIN_1 = NIN(channels, channels)
        self.NIN_2 = NIN(channels, channels)
        self.NIN_3 = NIN(channels, channels, init_scale=0.0)
        self.channels = channels


class ResnetBlockDDPM(nn.Module):
    """models/layers.py:619-662: no resampling inside the block, no 1/sqrt(2) rescale, a NIN shortcut where the widths differ."""
    kind = "res"
    skip_rescale = False
    up = down = fir = False

    def __init__(self, in_ch, out_ch=None, temb_dim=None, conv_shortcut=False, dropout=0.1):
        super().__init__()
        out_ch = out_ch if out_ch else in_ch
        self.GroupNorm_0 = _group_norm(in_ch)
        self.Conv_0 = _conv(in_ch, out_ch, 3, padding=1)
        if temb_dim is not None:
            self.Dense_0 = _dense(temb_dim, out_ch)
        self.GroupNorm_1 = _group_norm(out_ch)
        self.Dropout_0 = nn.Dropout(dropout)
        self.Conv_1 = _conv(out_ch, out_ch, 3, init_scale=0.0, padding=1)
        if in_ch != out_ch:
            if conv_shortcut:
                raise NotImplementedError("ResnetBlockDDPM(conv_shortcut=True): the 3x3 shortcut (Conv_2) is not built; "
                                          "DDPM never sets it (models/ddpm.py:57)")
            self.NIN_0 = NIN(in_ch, out_ch)
        self.in_ch, self.out_ch = in_ch, out_ch
        self.dropout = dropout


class Downsample(nn.Module):
    """models/layers.py:599-616: F.pad(x, (0, 1, 0, 1)) + 3x3 / stride 2 / no padding, or the 2x2 average."""
    kind = "down"

    def __init__(self, channels, with_conv=False):
        super().__init__()
        if with_conv:
            self.Conv_0 = _conv(channels, channels, 3, stride=2, padding=0)
        self.channels, self.with_conv = channels, with_conv


class Upsample(nn.Module):
    """models/layers.py:584-596: nearest-neighbour x2, then an optional 3x3 convolution."""
    kind = "up"

    def __init__(self, channels, with_conv=False):
        super().__init__()
        if with_conv:
            self.Conv_0 = _conv(channels, channels, 3, padding=1)
        self.channels, self.with_conv = channels, with_conv


@utils.register_model(name="ddpm")
class DDPM(HipUNet):
    """The U-Net of the configs/vp/ddpm/* experiments."""
    family = "ddpm"
    embedding_type = "positional"       # get_timestep_embedding(labels, nf) (models/ddpm.py:116)

    def __init__(self, config):
        super().__init__()
        self.config = config
        m = config.model
        if m.nonlinearity.lower() != "swish":
            raise NotImplementedError("the HIP path fuses SiLU; nonlinearity=%r is not built" % m.nonlinearity)
        self.register_buffer("sigmas", torch.tensor(utils.get_sigmas(config)))
        self.nf = nf = m.nf
        ch_mult = tuple(m.ch_mult)
        self.num_res_blocks = nrb = m.num_res_blocks
        self.attn_resolutions = tuple(m.attn_resolutions)
        self.num_resolutions = nres = len(ch_mult)
        self.all_resolutions = [config.data.image_size // (2 ** i) for i in range(nres)]
        self.conditional = bool(m.conditional)
        self.resamp_with_conv = bool(m.resamp_with_conv)
        self.scale_by_sigma = m.scale_by_sigma
        self.centered = config.data.centered
        self.channels = channels = config.data.num_channels

        mods = []
        add = mods.append
        if self.conditional:
            add(_dense(nf, nf * 4))
            add(_dense(nf * 4, nf * 4))

        def res_block(in_ch, out_ch=None):
            # Dense_0 exists in every block whether the model is conditioned or not (models/ddpm.py:57 passes temb_dim
            # always): an unconditional checkpoint carries the tensors, the forward never reads them (temb is None)
            return ResnetBlockDDPM(in_ch, out_ch, temb_dim=4 * nf, dropout=m.dropout)

        # ---- encoder
        add(_conv(channels, nf, 3, padding=1))
        skip_chs = [nf]
        cur = nf
        for lvl in range(nres):
            for _ in range(nrb):
                out_ch = nf * ch_mult[lvl]
                add(res_block(cur, out_ch))
                cur = out_ch
                if self.all_resolutions[lvl] in self.attn_resolutions:
                    add(AttnBlock(cur))
                skip_chs.append(cur)
            if lvl != nres - 1:
                add(Downsample(cur, with_conv=self.resamp_with_conv))
                skip_chs.append(cur)

        # ---- bottleneck
        cur = skip_chs[-1]
        add(res_block(cur))
        add(AttnBlock(cur))
        add(res_block(cur))

        # ---- decoder
        for lvl in reversed(range(nres)):
            for _ in range(nrb + 1):
                out_ch = nf * ch_mult[lvl]
                add(res_block(cur + skip_chs.pop(), out_ch))
                cur = out_ch
            if self.all_resolutions[lvl] in self.attn_resolutions:
                add(AttnBlock(cur))
            if lvl != 0:
                add(Upsample(cur, with_conv=self.resamp_with_conv))
        assert not skip_chs
        add(_group_norm(cur))
        add(_conv(cur, channels, 3, init_scale=0.0, padding=1))

        self.all_modules = nn.ModuleList(mods)
        self._engines = {}
