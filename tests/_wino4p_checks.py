"""Checks of the position-batched F(4x4,3x3) convolution (conv_wino4p.hip, SSDE_TILE_WINOGRAD4P), shared by the emulator
(test_emulated_wino4p.py) and the GPU (test_wino4p_gpu.py) suites."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

import _util

TOL = 2e-5      # the F(4x4,3x3) op tolerance (_train_checks.check_conv_winograd4): it rounds ~5x coarser than the direct kernel


def run_case(dev, ops, n, c0, c1, cout, h, pro, resid_post, ks, seed=0):
    """One launch through ssde_conv2d: concatenated source (c1 > 0) with the GroupNorm + SiLU prologue (pro), bias, per-sample
    addend, residual (resid_post 0 / 1), out_scale = 1/sqrt(2), GroupNorm partials of the result; ks = 1 / 2 / 4 reduction shares
    (forced by flags).  Checked against an fp64 torch convolution and fp64 statistics; returns (dst, partials)."""
    from score_sde_pytorch_amd import _lib as L
    from score_sde_pytorch_amd.engine import pack_wino4p_weight
    lib = L.load()
    g = torch.Generator().manual_seed(1000 + seed)
    cin = c0 + c1
    x0 = torch.randn(n, h, h, c0, generator=g) * 1.5 + 0.3
    x1 = torch.randn(n, h, h, c1, generator=g) if c1 else None
    xcat = torch.cat([x0, x1], -1) if c1 else x0
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b, gamma, beta = torch.randn(cout, generator=g), torch.randn(cin, generator=g), torch.randn(cin, generator=g)
    resid, ca = torch.randn(n, h, h, cout, generator=g), torch.randn(n, cout, generator=g)
    G = 32 if cin % 128 == 0 else cin // 4
    x0d, x1d = x0.to(dev), (x1.to(dev) if c1 else None)
    a = L.ConvArgs()
    keep = []
    if pro:
        mean, rstd = ops.groupnorm_stats(x0d, G, 1e-6, x2=x1d)
        gn = (mean, rstd, gamma.to(dev), beta.to(dev), G)
        keep.append(gn)
        ops._fill_src(a.main, x0d, x1d, L.PRO_GN_SILU, gn)
    else:
        ops._fill_src(a.main, x0d, x1d)
    wp, bd, cad, rd = pack_wino4p_weight(w).to(dev), b.to(dev), ca.to(dev), resid.to(dev)
    dst = torch.full((n, h, h, cout), float("nan"), device=dev)
    a.w_main, a.ksize, a.stride, a.pad, a.h_in, a.w_in = wp.data_ptr(), 3, 1, 1, h, h
    a.n, a.h_out, a.w_out, a.c_out, a.out_scale, a.dst, a.tile = n, h, h, cout, 1 / math.sqrt(2), dst.data_ptr(), L.TILE_WINOGRAD4P
    a.bias, a.chan_add, a.chan_add_ld, a.resid, a.resid_post = bd.data_ptr(), cad.data_ptr(), cout, rd.data_ptr(), resid_post
    a.flags = {1: L.CONVF_NO_KSPLIT, 2: L.CONVF_KSPLIT2, 4: L.CONVF_KSPLIT4}[ks]
    need = int(lib.ssde_conv_ws_floats(C.byref(a)))
    T, np_ = n * (h // 4) ** 2, -(-cout // 64) * 64
    assert need == 36 * T * cin + ks * 36 * T * np_, (need, ks)          # the shares asked for are the shares taken
    ws = torch.full((need,), float("nan"), device=dev)
    a.wino_ws, a.wino_ws_floats = ws.data_ptr(), need
    sl = lib.ssde_conv_gn_slices(C.byref(a))
    assert sl == (h // 4) ** 2
    part = torch.full((n, sl, cout // 4, 3), float("nan"), device=dev)
    a.gn_part = part.data_ptr()
    L.check(lib.ssde_conv2d(C.byref(a), ops._stream()), "ssde_conv2d")
    xn = xcat.double().permute(0, 3, 1, 2)
    if pro:
        xn = F.silu(F.group_norm(xn, G, gamma.double(), beta.double(), 1e-6))
    conv = (F.conv2d(xn, w.double(), b.double(), padding=1) + ca.double()[:, :, None, None]).permute(0, 2, 3, 1)
    ref = (conv + resid.double()) / math.sqrt(2) if resid_post == 0 else conv / math.sqrt(2) + resid.double()
    err = _util.rel_err(dst, ref)
    assert err < TOL, (n, c0, c1, cout, h, pro, resid_post, ks, err)
    # the partials merged by ssde_gn_finalize against fp64 statistics of the reference output, 4 channels per group
    Go = cout // 4
    f = L.GnFinalizeArgs()
    m2, r2 = torch.zeros(n, Go, device=dev), torch.zeros(n, Go, device=dev)
    f.part0, f.c0, f.slices0, f.n, f.groups, f.eps = part.data_ptr(), cout, sl, n, Go, 1e-6
    f.mean, f.rstd = m2.data_ptr(), r2.data_ptr()
    L.check(lib.ssde_gn_finalize(C.byref(f), ops._stream()), "ssde_gn_finalize")
    rg = ref.reshape(n, h * h, Go, 4).permute(0, 2, 1, 3).reshape(n, Go, -1)
    mr, rr = rg.mean(-1), 1.0 / torch.sqrt(rg.var(-1, unbiased=False) + 1e-6)
    assert (m2.cpu().double() - mr).abs().max().item() < 1e-5 * max(1.0, mr.abs().max().item())
    assert ((r2.cpu().double() - rr).abs() / rr).max().item() < 1e-4
    # a second launch on the same arguments: bit for bit (fixed-order slab sum, no atomics)
    d1, p1 = dst.clone(), part.clone()
    L.check(lib.ssde_conv2d(C.byref(a), ops._stream()), "ssde_conv2d")
    assert torch.equal(dst, d1) and torch.equal(part, p1)
    return d1, p1


def check_packer():
    """pack_wino4p_weight against U = G g G^T formed in fp64 by explicit matrix products, and its zero padding"""
    from score_sde_pytorch_amd.engine import pack_wino4p_weight
    G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                      [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=torch.float64)
    g = torch.Generator().manual_seed(7)
    cout, cin = 70, 36
    w = torch.randn(cout, cin, 3, 3, generator=g)
    p = pack_wino4p_weight(w)
    assert p.shape == (36, 9, 128, 4)
    U = G @ w.double() @ G.t()                                           # [cout, cin, 6, 6]
    ref = torch.zeros(36, 9, 128, 4, dtype=torch.float64)
    ref[:, :, :cout] = U.reshape(cout, 9, 4, 36).permute(3, 1, 0, 2)
    assert (p.double() - ref).abs().max().item() <= 1e-7 * ref.abs().max().item()
    assert p[:, :, cout:].abs().max().item() == 0.0
