"""The input side of the two-kernel F(4x4,3x3) convolution: the transform pass (wino4_xform.hip) writing V with non-temporal
stores against the same pass with plain stores, shared by tests/test_fir_v_cpu.py (emulator) and tests/test_fir_v_gpu.py.

What is compared, through ssde_wino4_input_transform (the pass on its own):
  * V of the library's own choice of stores == V of plain stores (SSDE_CONVF_XFORM_PLAIN: the kept instantiations), BIT FOR BIT
    -- the same arithmetic per thread, another kind of store;
  * the statistics a merging pass leaves in gn_mean / gn_rstd, bit for bit as well;
  * V of the plain stores against B^T pro(x) B in fp64, _util.rel_err < TOL_OP = 2e-5 (the bound of tests/_conv_shape_checks.py
    for an F(4x4,3x3) result: the transform alone rounds less than the convolution it feeds).
Maps: part of an image per workgroup, several images per workgroup, workgroups that straddle images, ragged quad blocks, batch
tails, a concatenated source, and the channel count from which the launch keeps plain stores (512)."""
import ctypes as C

import torch
import torch.nn.functional as F

import _util

TOL_OP = 2e-5

# (name, batch, h, w, c0, c1): the three shapes of the issue, then the remaining tilings and the rule's other side
CASES = [("32x32_8ch", 3, 32, 32, 8, 0),            # 4 tile blocks per image; 2 of 16 quads
         ("8x8_16ch", 5, 8, 8, 16, 0),              # four images per block, batch tail
         ("32x32_8+12ch", 2, 32, 32, 8, 12),        # concatenated source
         ("64x64_72ch", 1, 64, 64, 72, 0),          # two quad blocks, the second ragged
         ("24x24_8ch", 3, 24, 24, 8, 0),            # 36 tiles per image: blocks straddle images
         ("8x8_512ch", 2, 8, 8, 512, 0)]            # 512 channels: plain stores either way
PROLOGUES = ["none", "gn_silu", "gn_silu_merged"]

BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                   [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=torch.float64)


def v_fp64(xact):
    """V[36][C/4][T][4] of an activated NHWC tensor in fp64: zero ring, 6x6 patches every 4 pixels, B^T d B"""
    n, h, w, c = xact.shape
    xp = F.pad(xact.double(), (0, 0, 1, 1, 1, 1))
    p = xp.unfold(1, 6, 4).unfold(2, 6, 4)                           # [n, ty, tx, c, a, b]
    v = torch.einsum("ak,nyxckl,bl->abnyxc", BT, p, BT)
    return v.reshape(36, n * (h // 4) * (w // 4), c // 4, 4).permute(0, 2, 1, 3).contiguous()


def partials(x, slices):
    """(mean, M2, count) per (image, slice of rows, channel quad), [N][S][C/4][3]: what a producer's epilogue leaves"""
    n, h, w, c = x.shape
    xs = x.double().reshape(n, slices, (h // slices) * w, c // 4, 4).permute(0, 1, 3, 2, 4).reshape(n, slices, c // 4, -1)
    m = xs.mean(-1)
    return torch.stack([m, ((xs - m[..., None]) ** 2).sum(-1), torch.full_like(m, xs.shape[-1])], -1).float().contiguous()


def check_streamed_v(dev, case, prologue):
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    lib = L.load()
    name, n, h, w, c0, c1 = case
    ctot = c0 + c1
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(n, h, w, c0, generator=g) * 1.5 + 0.3
    x1 = torch.randn(n, h, w, c1, generator=g) - 0.2 if c1 else None
    xcat = torch.cat([x0, x1], -1) if c1 else x0
    G = ctot // 4 if ctot < 128 else 32
    gamma, beta = torch.randn(ctot, generator=g), torch.randn(ctot, generator=g)
    x0d, x1d = x0.to(dev), (x1.to(dev) if c1 else None)
    T = n * (h // 4) * (w // 4)
    keep = []

    def run(flags):
        a = L.ConvArgs()
        if prologue == "none":
            ops._fill_src(a.main, x0d, x1d, L.PRO_NONE)
            mean = rstd = None
        else:
            if prologue == "gn_silu":
                mean, rstd = ops.groupnorm_stats(x0d, G, 1e-6, x2=x1d)
            else:
                mean, rstd = torch.full((n, G), float("nan"), device=dev), torch.full((n, G), float("nan"), device=dev)
                p0, p1 = partials(x0, 2).to(dev), (partials(x1, 1).to(dev) if c1 else None)
                a.gn_in_part0, a.gn_in_slices0, a.gn_in_eps = p0.data_ptr(), 2, 1e-6
                if c1:
                    a.gn_in_part1, a.gn_in_slices1 = p1.data_ptr(), 1
                keep.extend([p0, p1])
            gd, bd = gamma.to(dev), beta.to(dev)
            keep.extend([gd, bd])
            ops._fill_src(a.main, x0d, x1d, L.PRO_GN_SILU, (mean, rstd, gd, bd, G))
        v = torch.full((36 * T * ctot,), float("nan"), device=dev)
        a.ksize, a.stride, a.pad, a.h_in, a.w_in, a.n, a.h_out, a.w_out = 3, 1, 1, h, w, n, h, w
        a.tile, a.flags, a.wino_v = L.TILE_WINOGRAD4R, flags, v.data_ptr()
        L.check(lib.ssde_wino4_input_transform(C.byref(a), ops._stream()), "ssde_wino4_input_transform")
        if dev != "cpu":
            torch.cuda.synchronize()
        return v.cpu(), (mean.cpu(), rstd.cpu()) if mean is not None else None

    v_plain, st_plain = run(L.CONVF_XFORM_PLAIN)
    v_new, st_new = run(0)
    assert torch.equal(v_new, v_plain), (name, prologue, "V differs from the plain stores'")
    if prologue == "gn_silu_merged":
        assert torch.equal(st_new[0], st_plain[0]) and torch.equal(st_new[1], st_plain[1]), (name, "merged statistics differ")
        assert not torch.isnan(st_new[0]).any() and not torch.isnan(st_new[1]).any(), (name, "a statistic was not written")
    xact = xcat
    if prologue != "none":
        xact = F.silu(F.group_norm(xcat.double().permute(0, 3, 1, 2), G, gamma.double(), beta.double(), 1e-6)).permute(0, 2, 3, 1)
    err = _util.rel_err(v_plain.reshape(36, ctot // 4, T, 4), v_fp64(xact))
    print("%s %s: V vs fp64 rel err %.3g" % (name, prologue, err))
    assert err < TOL_OP, (name, prologue, err)


def check_entry_refusals(dev):
    """the pass on its own refuses, by name and before any launch, what is not a two-kernel launch's pass"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    lib = L.load()
    x = torch.zeros(1, 8, 8, 8, device=dev)
    v = torch.zeros(36 * 4 * 8, device=dev)
    a = L.ConvArgs()
    ops._fill_src(a.main, x, None, L.PRO_NONE)
    a.ksize, a.stride, a.pad, a.h_in, a.w_in, a.n, a.h_out, a.w_out = 3, 1, 1, 8, 8, 1, 8, 8
    a.wino_v, a.tile = v.data_ptr(), L.TILE_WINOGRAD4
    assert lib.ssde_wino4_input_transform(C.byref(a), ops._stream()) != 0 and b"SSDE_TILE_WINOGRAD4R" in lib.ssde_last_error()
    a.tile, a.flags = L.TILE_WINOGRAD4R, L.CONVF_V_GIVEN
    assert lib.ssde_wino4_input_transform(C.byref(a), ops._stream()) != 0 and b"V_GIVEN" in lib.ssde_last_error()
    a.flags, a.wino_v = 0, None
    assert lib.ssde_wino4_input_transform(C.byref(a), ops._stream()) != 0 and b"wino_v" in lib.ssde_last_error()
    a.wino_v, a.h_in = v.data_ptr(), 6
    assert lib.ssde_wino4_input_transform(C.byref(a), ops._stream()) != 0 and b"bad shape" in lib.ssde_last_error()


def check_cifar_program_shape(monkeypatch):
    """the lowered CIFAR-10 sampling program keeps its 221 ops of the pinned kinds, and the kind of store is the library's own
    choice in it (no launch carries SSDE_CONVF_XFORM_PLAIN unless the environment of an A/B run asks for it: SSDE_XFORM_NT=0)"""
    from score_sde_pytorch_amd import configs, engine as E, _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    monkeypatch.setenv("SSDE_WINOGRAD", "1")
    monkeypatch.delenv("SSDE_XFORM_NT", raising=False)
    cfg = configs.get_config("ve/cifar10_ncsnpp_continuous")
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    prog = E.UNetEngine(model, 2, 32, 32, "cpu").program
    kinds = [int(prog.ops[i].kind) for i in range(prog.n)]
    assert len(kinds) == 221
    assert (kinds.count(L.OP_CONV), kinds.count(L.OP_UPFIRDN), kinds.count(L.OP_ATTN), kinds.count(L.OP_GN_FINALIZE)) == (108, 9, 6, 95)
    convs = [prog.ops[i].u.conv for i in range(prog.n) if prog.ops[i].kind == L.OP_CONV]
    assert not [c for c in convs if c.flags & L.CONVF_XFORM_PLAIN]
    monkeypatch.setenv("SSDE_XFORM_NT", "0")
    prog = E.UNetEngine(model, 2, 32, 32, "cpu").program
    convs = [prog.ops[i].u.conv for i in range(prog.n) if prog.ops[i].kind == L.OP_CONV]
    assert prog.n == 221 and all(c.flags & L.CONVF_XFORM_PLAIN for c in convs)
