"""Checks of the input gradient (dx) as the backward lowering composes it (backward.TrainEngine._bwd_branch): a FORWARD
convolution launch on the output gradient g with the layer's weight in its input-gradient packing -- WeightStore.conv3 /
.matrix, then .derived (in / out swapped and the taps rotated by 180 degrees; a matrix transposed), then refresh(), which on
the GPU is the device re-pack (ssde_pack_weights) -- never a hand-made permute / flip.  Shared by the emulator suite
(tests/test_dgrad_cpu.py) and the GPU suite (tests/test_dgrad_gpu.py, both matrix modes).

  stride 1   every row of engine.CONV3_ROUTES: g [n, h, w, cout] -> dx [n, h, w, cin], 3x3 / pad 1 on the route's tile, with
             cin != cout in both orientations and neither a multiple of 64: (96, 40) and (40, 96) where the route's plan
             accepts the launch, else the nearest counts it accepts (found with the plan query, ssde_conv_lds_bytes).
  stride 2   the transposed form: zero insertion (ssde_upfirdn2d, up = 2, a 1x1 kernel), then a pad 2 / stride 1 launch whose
             output is cropped to the forward input (out_hw); end-padded and plain forward geometries, odd maps, a map whose
             last column no output reads (its gradient is zero and must be written), a padded stored channel.
  1x1        the derived matrix of a plain [out, in] matrix, of a NIN [in, out] entry and of a row-concatenated entry of three
             NIN parts (q / k / v), each at a shape the GEMM of conv1x1.hip takes (189 rows onto 96 channels) and at one it
             leaves to the 1x1 half of the direct kernel (40 channels).

Every case runs twice: written into NaN with scale 1 (every pixel must be written, also where the gradient is exactly zero),
and accumulated in place onto a base (resid == dst, resid_post = 1, scale 0.7: the launch _bwd_branch issues).
Reference: fp64 autograd through F.conv2d / einsum.  The weights are random and asymmetric, so a transposed or unrotated
image fails.  Error: _util.rel_err against TOL_OP = 2e-5; one seed per case.

Largest errors seen (every check prints its own); the bound is 2e-5:
                                        emulator (exact fp32)         MI355X
  stride 1   direct / f2                8.2e-7 / 2.9e-7               not measured yet
             f4 / f4r / f4p             6.1e-6 / 6.4e-6 / 6.1e-6      not measured yet
  stride 2                              4.6e-7                        not measured yet
  1x1        GEMM / direct kernel       5.1e-7 / 3.5e-7               not measured yet
(f4p takes input counts that are multiples of 32: its 40 -> 96 case runs as 32 -> 96.)
"""
import ctypes as C
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import _train_checks as T
from _util import rel_err
from score_sde_pytorch_amd import _lib as L

TOL_OP = T.TOL_OP
assert TOL_OP == 2e-5
ACC_SCALE = 0.7
N = 3


def _ops():
    from score_sde_pytorch_amd import hipops as ops
    return ops, L.load()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _param(t, dev):
    return torch.nn.Parameter(t.to(dev))


def _store(dev):
    from score_sde_pytorch_amd import engine as E
    return E.WeightStore(torch.device(dev))


# ------------------------------------------------------------------------------------------------ the launch
def conv_args(tile, n, c_in, h_in, w_in, c_out, h_out, w_out, ksize, pad, src=None, w=None, dst=None, alias=False, scale=1.0):
    """the ssde_conv_args of an input-gradient launch as Lowering.conv fills them for _bwd_branch: no bias, no per-image
    addend, no partials; src / w / dst None: dummies, which is all a plan query reads"""
    a = L.ConvArgs()
    dummy = 0x1000
    s = a.main if ksize == 3 else a.aux
    s.p0, s.c0, s.p1, s.c1, s.pro_mode = (src.data_ptr() if src is not None else dummy), c_in, None, 0, L.PRO_NONE
    wp = w.data_ptr() if w is not None else dummy
    if ksize == 3:
        a.w_main, a.ksize, a.stride, a.pad, a.h_in, a.w_in = wp, 3, 1, pad, h_in, w_in
    else:
        a.w_aux, a.ksize, a.stride, a.pad = wp, 0, 1, 0
    a.n, a.h_out, a.w_out, a.c_out, a.tile = n, h_out, w_out, c_out, tile
    a.dst = dst.data_ptr() if dst is not None else dummy
    a.flags = L.conv_route_flags()
    a.out_scale = scale
    if alias:
        a.resid, a.resid_post = a.dst, 1
    return a


def plan_accepts(tile, n, c_in, h, w, c_out):
    """does the plan of the route take the in-place 3x3 / pad 1 launch c_in -> c_out on an h x w map?"""
    _, lib = _ops()
    return all(lib.ssde_conv_lds_bytes(C.byref(conv_args(tile, n, c_in, h, w, c_out, h, w, 3, 1, alias=alias))) > 0 for alias in (False, True))


def accepted_counts(route, n, h, w, c_in, c_out):
    """(c_in, c_out) of the launch: the wanted counts if the route's plan accepts them, else the nearest it accepts (steps of 4
    channels, the input count first), still different from each other and no multiple of 64"""
    cands = sorted(((abs(di) + abs(do), abs(do), di, do) for di in range(-32, 33, 4) for do in range(-32, 33, 4)))
    for _, _, di, do in cands:
        ci, co = c_in + di, c_out + do
        if ci > 0 and co > 0 and ci != co and ci % 64 and co % 64 and plan_accepts(route.tile, n, ci, h, w, co):
            return ci, co
    raise AssertionError("%s: no channel counts near %d -> %d that its plan accepts on %dx%d" % (route.name, c_in, c_out, h, w))


def run_twice(what, make_args, shape, ref, dev, base_seed, more=None):
    """the launch into NaN with scale 1, then in place onto a base with ACC_SCALE; `ref`: the fp64 gradient [n, h, w, c] of
    the channels it covers (dx may store more: they must be written with zeros).  Returns the larger error."""
    ops, lib = _ops()
    errs = []
    base = torch.randn(shape, generator=_gen("base", base_seed))
    c_ref = ref.shape[-1]
    for alias in (False, True):
        dst = (base.clone() if alias else torch.full(shape, float("nan"))).to(dev)
        a, keep = make_args(dst, alias, ACC_SCALE if alias else 1.0)
        assert lib.ssde_conv_lds_bytes(C.byref(a)) > 0, (what, lib.ssde_last_error())
        if more is not None:
            keep.append(more(a, lib))
        L.check(lib.ssde_conv2d(C.byref(a), ops._stream()), "ssde_conv2d")
        got = dst.cpu()
        assert bool(torch.isfinite(got).all()), (what, "part of dx was not written")
        want = (ACC_SCALE * ref + base[..., :c_ref].double()) if alias else ref
        err = rel_err(got[..., :c_ref], want)
        if c_ref < shape[-1]:                     # padded stored channels: a zero weight, so exactly the base / exactly zero
            assert torch.equal(got[..., c_ref:], base[..., c_ref:] if alias else torch.zeros_like(got[..., c_ref:])), (what, "padded channel")
        print("dgrad %s %s vs fp64: %.3g" % (what, "accumulated in place" if alias else "written into NaN", err))
        assert err < TOL_OP, (what, alias, err)
        errs.append(err)
    return max(errs)


# ------------------------------------------------------------------------------------------------ stride 1, every route
def stride1_cases():
    from score_sde_pytorch_amd import engine as E
    return [(r.name, cin, cout) for r in E.CONV3_ROUTES for (cin, cout) in ((96, 40), (40, 96))]


def stride1_id(case):
    return "%s-%dto%d" % case


def check_stride1(dev, case):
    from score_sde_pytorch_amd import engine as E
    name, cin, cout = case
    route = next(r for r in E.CONV3_ROUTES if r.name == name)
    h, w = (4, 8) if route is E.F4P else (8, 12)
    # the launch reads g (cout channels) and writes dx (cin channels)
    cout, cin = accepted_counts(route, N, h, w, cout, cin)
    g_ = _gen("stride1", name, cin, cout)
    wt = torch.randn(cout, cin, 3, 3, generator=g_) / np.sqrt(9 * cout)
    gy = torch.randn(N, h, w, cout, generator=g_) + 0.25
    x = torch.zeros(N, cin, h, w, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wt.double(), padding=1).backward(gy.double().permute(0, 3, 1, 2))
    ref = x.grad.permute(0, 2, 3, 1).contiguous()
    ws = _store(dev)
    wd = ws.derived(ws.conv3(_param(wt, dev), route=route), route)
    ws.refresh()
    gyd = gy.to(dev)

    def make_args(dst, alias, scale):
        return conv_args(route.tile, N, cout, h, w, cin, h, w, 3, 1, src=gyd, w=wd, dst=dst, alias=alias, scale=scale), [gyd, wd]

    def more(a, lib):
        keep = []
        if route.takes_v and route is E.F4R:
            v = torch.full((E.wino4_v_floats(N, h, w, cout),), float("nan")).to(dev)
            a.wino_v = v.data_ptr()
            keep.append(v)
        if route.needs_ws:
            need = int(lib.ssde_conv_ws_floats(C.byref(a)))
            assert need > 0, lib.ssde_last_error()
            wsb = torch.full((need,), float("nan")).to(dev)
            a.wino_ws, a.wino_ws_floats = wsb.data_ptr(), need
            keep.append(wsb)
        return keep

    return run_twice("stride 1 %s %d -> %d on %dx%d" % (name, cout, cin, h, w), make_args, (N, h, w, cin), ref, dev, case, more)


# ------------------------------------------------------------------------------------------------ stride 2, transposed
# (h_in, w_in, pad_end, cin, stored cin, cout): the forward is 3x3 / stride 2 / pad 0 with pad_end zero rows and columns at the end
STRIDE2_CASES = [(12, 20, 1, 8, 8, 40), (7, 9, 1, 8, 8, 40), (7, 9, 0, 8, 8, 40),
                 (9, 12, 0, 8, 8, 40),          # column 11 is read by no output (5 outputs read columns 0..10): a zero gradient
                 (7, 9, 1, 3, 4, 24)]           # an image of 3 channels stored in 4 (check_backward_ops): the 4th gets zeros


def stride2_id(case):
    return "%dx%d-e%d-%din%d-%d" % case


def check_stride2(dev, case):
    from score_sde_pytorch_amd import engine as E
    ops, _ = _ops()
    h, w, pad_end, cin, cstore, cout = case
    ho, wo = (h + pad_end - 3) // 2 + 1, (w + pad_end - 3) // 2 + 1
    g_ = _gen("stride2", case)
    wt = torch.randn(cout, cin, 3, 3, generator=g_) / np.sqrt(9 * cout)
    gy = torch.randn(N, ho, wo, cout, generator=g_) + 0.25
    x = torch.zeros(N, cin, h, w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (0, pad_end, 0, pad_end)), wt.double(), stride=2)
    assert tuple(y.shape[2:]) == (ho, wo)
    y.backward(gy.double().permute(0, 3, 1, 2))
    ref = x.grad.permute(0, 2, 3, 1).contiguous()
    if case[:3] == (9, 12, 0):
        assert float(ref[:, :, 11].abs().max()) == 0.0 and float(ref[:, :, 10].abs().max()) > 0.0
    ws = _store(dev)
    wd = ws.derived(ws.conv3(_param(wt, dev), cin_pad=cstore if cstore != cin else None), E.DIRECT)
    ws.refresh()
    # zero insertion as Lowering.upfirdn emits it for _bwd_branch: up = 2, a 1x1 kernel of one, no padding
    gz = ops.upfirdn2d_nhwc(gy.to(dev), torch.ones(1, 1), up=2, pad=(0, 0))
    hz, wz = gz.shape[1], gz.shape[2]
    assert (hz, wz) == (2 * ho, 2 * wo) and hz + 2 >= h and wz + 2 >= w

    def make_args(dst, alias, scale):
        return conv_args(E.DIRECT.tile, N, cout, hz, wz, cstore, h, w, 3, 2, src=gz, w=wd, dst=dst, alias=alias, scale=scale), [gz, wd]

    return run_twice("stride 2 %s" % stride2_id(case), make_args, (N, h, w, cstore), ref, dev, case)


# ------------------------------------------------------------------------------------------------ 1x1: the derived matrix
# (kind, channels in, channels out of the forward layer).  dx has `in` channels: 96 -> the GEMM (189 rows, >= 96 channels),
# 40 -> the 1x1 half of the direct kernel
MATRIX_CASES = [(kind, cin, cout) for kind in ("plain", "nin", "qkv") for (cin, cout) in ((96, 40), (40, 96))]
H1, W1 = 7, 9


def matrix_id(case):
    return "%s-%dto%d" % case


def check_matrix(dev, case):
    kind, cin, cout = case
    g_ = _gen("matrix", case)
    if kind == "plain":
        params, parts = [torch.randn(cout, cin, generator=g_) / np.sqrt(cout)], [False]
    elif kind == "nin":
        params, parts = [torch.randn(cin, cout, generator=g_) / np.sqrt(cout)], [True]
    else:                                           # q / k / v: three NIN [in, out] matrices, rows concatenated
        cout = cin
        params, parts = [torch.randn(cin, cout, generator=g_) / np.sqrt(3 * cout) for _ in range(3)], [True] * 3
    rows = cout * len(params)
    gy = torch.randn(N, H1, W1, rows, generator=g_) + 0.25
    x = torch.zeros(N, H1, W1, cin, dtype=torch.float64, requires_grad=True)
    y = torch.cat([torch.einsum("nhwi,io->nhwo", x, p.double()) if tr else torch.einsum("nhwi,oi->nhwo", x, p.double())
                   for p, tr in zip(params, parts)], dim=-1)
    y.backward(gy.double())
    ref = x.grad
    ws = _store(dev)
    wd = ws.derived(ws.matrix([(_param(p, dev), tr) for p, tr in zip(params, parts)]))
    ws.refresh()
    gyd = gy.to(dev)
    gemm = cin >= 96 and N * H1 * W1 >= 128        # (ssde_conv1x1_wants restated)
    assert gemm == (cin == 96)

    def make_args(dst, alias, scale):
        return conv_args(L.TILE_AUTO, N, rows, H1, W1, cin, H1, W1, 0, 0, src=gyd, w=wd, dst=dst, alias=alias, scale=scale), [gyd, wd]

    return run_twice("1x1 %s %d -> %d (%s)" % (kind, rows, cin, "GEMM" if gemm else "direct kernel"), make_args, (N, H1, W1, cin), ref, dev, case)
