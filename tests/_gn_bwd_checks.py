"""Checks of the GroupNorm backward of the 4-channel-multiple path -- gn_bwd_fused_kernel, gn_bwd_reduce_kernel,
gn_bwd_finalize_kernel, gn_bwd_finish_kernel and prologue_bwd_kernel of csrc/backward.hip, behind ssde_gn_bwd_reduce,
ssde_gn_bwd_finish and ssde_prologue_bwd -- shared by the emulator suite (tests/test_gn_bwd_cpu.py) and the GPU suite
(tests/test_gn_bwd_gpu.py).

The reference is fp64 autograd over the same arithmetic (_gn_width_checks._ref64; the dropout mask is the numpy restatement of
the hash, _train_checks.hash_keep), the error is max-abs error over max-abs reference value (_util.rel_err), taken separately
for dx of source 0, dx of source 1, dgamma and dbeta.  Tolerances are the project's: 2e-5 for the GroupNorm
backward (a contraction: sums over a group's pixels and channels), 2e-6 for ssde_prologue_bwd in its SiLU-only and plain
modes (element-wise).  The kernels are handed the fp32 rounding of the fp64 statistics, so the figures are the backward
kernels' own.

Largest errors seen (every check prints its own):
                                                       emulator (exact fp32)   MI355X
  GroupNorm backward, 12 shapes x 4 modes x 3 routes   4.9e-7                  4.9e-7   (both at 16 channels, 1 group, 48x48)
  call forms                                           3.6e-7                  3.4e-7
  ssde_prologue_bwd alone                              2.9e-7                  2.8e-7
Before prologue_bwd_kernel applied the mask outside its GroupNorm branch, the dropout cases of check_prologue_bwd failed with
errors of 0.50 .. 0.82 in SiLU-only mode and 0.59 .. 0.86 in plain mode (emulator); every other check passed.
"""
import contextlib
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import _gn_width_checks as W
import _train_checks as T
from _util import rel_err

TOL_OP, TOL_ELEM = T.TOL_OP, 2e-6
assert TOL_OP == 2e-5
DROP_P, SALT, SEED_WORD = 0.25, 0x1234567, 77

# (c0, c1, groups, h, w, n, SSDE_NUM_CUS of the ragged one-pass run, slices of the three-kernel run, one-pass kernel fits).
# One-pass kernel: a workgroup of 1024 threads owns gpc whole groups = clc channel quads (<= 256) of one sample, on
# pl = 1024 / clc pixel lanes of <= 8 pixels each.  SSDE_NUM_CUS=1 gives the longest run that fits; 2 or 3 ask for two
# workgroups per sample (runs of G - 1 groups and 1 group); 256 ends at one group per workgroup.
# Three kernels: the slices are ceil(hw / slices) pixels long, so 3 and 5 leave a short last slice or slices with no pixel.
GN_CASES = [
    (32, 16, 12, 8, 8, 3, 2, 3, True),        # 4 per group (check_backward_ops' shape); runs of 11 + 1 groups; slices 22, 22, 20
    (64, 0, 8, 4, 4, 3, 256, 5, True),        # 8 per group; one source; the fifth slice is empty
    (20, 20, 5, 4, 4, 3, 3, 3, True),         # 8 per group; group 2 = channels 16..23 straddles the concat boundary
    (36, 28, 4, 3, 3, 3, 2, 5, True),         # 16 per group; group 2 = channels 32..47 straddles; 9 pixels; runs of 3 + 1 groups
    (8, 24, 2, 5, 5, 3, 256, 3, True),        # 16 per group; the boundary lies inside group 0; 25 pixels
    (48, 0, 4, 1, 1, 3, 3, 5, True),          # 12 per group; a 1x1 map: four of five slices are empty
    (64, 64, 8, 3, 7, 3, 256, 5, True),       # non-square; 21 pixels on 32 pixel lanes (8 groups = 32 quads per workgroup)
    (132, 60, 16, 2, 3, 3, 2, 5, True),       # 12 per group; 33 + 15 channel quads: the boundary is a group's (132 = 11 x 12)
    (512, 0, 32, 2, 2, 3, 3, 3, True),        # the networks' widest single source: 128 quads in one workgroup, 8 pixel lanes
    (1024, 1024, 32, 2, 1, 3, 256, 3, True),  # 64 per group: 32 groups are 512 quads, the 256-quad limit cuts them into 16 + 16
    (96, 32, 32, 6, 6, 3, 2, 5, True),        # 4 per group over a concat; 32 quads, 36 pixels on 32 lanes: two pixels on four lanes
    (16, 0, 1, 48, 48, 1, 3, 5, False),       # one group of 4 quads: 2304 pixels > 8 x 256, the shape itself takes the three kernels
]
# the straddling cases and the widest one
CALL_FORM_CASES = [GN_CASES[2], GN_CASES[3], GN_CASES[4], GN_CASES[9]]

# (n, h, w, c0, c1, dp_ld, dp_off): 5, 8, 3, 2 and 9 channel quads against the 256-thread blocks; 1, 3, 126, 20 and 1023 pixels
# for the two-pixels-per-trip loop
PROLOGUE_CASES = [(1, 1, 1, 20, 0, 28, 4), (3, 1, 3, 20, 12, 40, 8), (2, 7, 9, 12, 0, 12, 0), (5, 2, 2, 4, 4, 8, 0),
                  (1, 33, 31, 36, 0, 36, 0)]


def case_id(c):
    return "%d+%d-g%d-%dx%d" % tuple(c[:5])


def _ops():
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    return ops, L


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _keep(n, h, w, C):
    """the mask the kernels regenerate: the hash of the element's index in the [n, h, w, C] concat tensor"""
    thresh = min(int(round(DROP_P * 2.0 ** 32)), 2 ** 32 - 1)
    keep = T.hash_keep(np.arange(n * h * w * C, dtype=np.uint64), SEED_WORD ^ SALT, thresh, 1.0 / (1.0 - DROP_P))
    keep = torch.from_numpy(keep).reshape(n, h, w, C)
    frac = float((keep > 0).float().mean())
    assert 0.6 < frac < 0.9, frac
    return keep


def _drop(dev):
    return (DROP_P, torch.tensor([SEED_WORD], dtype=torch.int32).to(dev), SALT)


@functools.lru_cache(maxsize=None)
def gn_case(case):
    """inputs that make a dropped term visible (x off centre, gamma of both signs, dy with a mean) and the fp64 reference of
    every mode, computed once per shape and shared (nothing writes to them)"""
    c0, c1, G, h, w, n = case[:6]
    C = c0 + c1
    g = torch.Generator().manual_seed(1000 * c0 + 10 * c1 + h * w)
    xc = torch.randn(n, h, w, C, generator=g) * 1.5 + 2.0 + torch.randn(1, 1, 1, C, generator=g)
    gamma, beta = torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    dy = torch.randn(n, h, w, C, generator=g) + 0.5
    keep = _keep(n, h, w, C)
    ref = {}
    for silu in (False, True):
        for drop in (False, True):
            mean, rstd, _, dx, dga, dbe = W._ref64(xc, G, gamma, beta, silu, keep if drop else None, dy)
            ref[silu, drop] = (dx[..., :c0], dx[..., c0:], dga, dbe)
    return dict(xc=xc, gamma=gamma, beta=beta, dy=dy, mean=mean.float(), rstd=rstd.float(), ref=ref)


def _device_inputs(dev, case):
    c0, c1, G = case[:3]
    k = gn_case(case)
    d = lambda t: t.to(dev)  # noqa: E731
    xa = d(k["xc"][..., :c0].contiguous())
    xb = d(k["xc"][..., c0:].contiguous()) if c1 else None
    gn = (d(k["mean"]), d(k["rstd"]), d(k["gamma"]), d(k["beta"]), G)
    return k, xa, xb, gn, d(k["dy"])


def _errors(got, ref, c1):
    """(dx0, dx1, dgamma, dbeta), each over its own largest reference value; dx1 only with a second source"""
    return [rel_err(a, b) for a, b, on in zip(got, ref, (True, c1 > 0, True, True)) if on]


def _scratch_rows(case, slices):
    """what the library says this call leaves in scratch: n on the one-pass path, n * slices on the three-kernel path"""
    import ctypes as C
    ops, L = _ops()
    c0, c1, G, h, w, n = case[:6]
    a = L.GnBwdReduceArgs()
    a.src.c0, a.src.c1, a.src.pro_mode, a.src.gn_groups = c0, c1, L.PRO_GN_SILU, G
    a.n, a.hw, a.slices, a.flags = n, h * w, slices, L.gn_bwd_route_flags()
    a.g0 = 0x1000                                  # shape-only query: the pointer is not dereferenced
    return int(L.load().ssde_gn_bwd_scratch_rows(C.byref(a)))


def routes(case):
    """(name, environment, slices, rows the route must report)"""
    n, cus, sl3, fits = case[5], case[6], case[7], case[8]
    assert cus in (2, 3, 256) and sl3 in (3, 5)
    return [("one pass, longest runs", {"SSDE_NUM_CUS": "1"}, 2, n if fits else 2 * n),
            ("one pass, %d CUs" % cus, {"SSDE_NUM_CUS": str(cus)}, 2, n if fits else 2 * n),
            ("three kernels, %d slices" % sl3, {"SSDE_GN_BWD_FUSED": "0"}, sl3, sl3 * n)]


def check_gn_backward(dev, case):
    """GroupNorm and GroupNorm + SiLU, with and without dropout, on the one-pass kernel with whole and with ragged runs of groups
    and on the three kernels with ragged slices: dx of both sources, dgamma and dbeta against fp64; the route is asserted"""
    ops, L = _ops()
    c1 = case[1]
    k, xa, xb, gn, dy = _device_inputs(dev, case)
    worst = 0.0
    for name, env, slices, rows in routes(case):
        with _env(env):
            assert _scratch_rows(case, slices) == rows, (case, name, _scratch_rows(case, slices), rows)
            for (silu, drop), ref in k["ref"].items():
                got = ops.gn_backward(xa, dy, gn, L.PRO_GN_SILU if silu else L.PRO_GN, x2=xb, dropout=_drop(dev) if drop else None,
                                      slices=slices)
                errs = _errors(got, ref, c1)
                worst = max(worst, max(errs))
                assert max(errs) < TOL_OP, (case, name, "silu" if silu else "plain", "dropout" if drop else "no dropout", errs)
    print("gn backward %s vs fp64: largest error %.3g" % (case_id(case), worst))
    return worst


def check_gn_call_forms(dev, case):
    """SiLU and dropout armed, on the one-pass kernel and on the three kernels: accumulation onto bases with a scale; one source
    wanted (the other's memory stays untouched); dgamma / dbeta deferred to ssde_gn_bwd_finish; the reduction and
    ssde_prologue_bwd as two calls; a second launch"""
    ops, L = _ops()
    c0, c1, G, h, w, n = case[:6]
    assert c1 > 0
    k, xa, xb, gn, dy = _device_inputs(dev, case)
    ref = k["ref"][True, True]
    kw = dict(x2=xb, dropout=_drop(dev))
    run = lambda **more: ops.gn_backward(xa, dy, gn, L.PRO_GN_SILU, **kw, **more)      # noqa: E731
    worst = 0.0
    for name, env, slices, rows in (routes(case)[0], routes(case)[2]):
        with _env(env):
            assert _scratch_rows(case, slices) == rows, (case, name)
            direct = run(slices=slices)
            # a second launch: the same bits
            assert all(torch.equal(a, b) for a, b in zip(direct, run(slices=slices))), (case, name, "second launch")
            # dgamma / dbeta by the finishing launch: the same bits
            assert all(torch.equal(a, b) for a, b in zip(direct, run(slices=slices, defer_params=True))), (case, name, "deferred")
            # accumulated onto bases, scaled
            g = torch.Generator().manual_seed(7)
            b0, b1 = torch.randn(n, h, w, c0, generator=g), torch.randn(n, h, w, c1, generator=g)
            dx0, dx1, dga, dbe = run(slices=slices, scale=0.25, acc=(True, True), dx=b0.clone().to(dev), dx2=b1.clone().to(dev))
            errs = _errors((dx0.cpu() - b0, dx1.cpu() - b1, dga, dbe), (0.25 * ref[0], 0.25 * ref[1], ref[2], ref[3]), c1)
            worst = max(worst, max(errs))
            assert max(errs) < TOL_OP, (case, name, "accumulate", errs)
            # one source wanted: both gradients' memory is one NaN-filled buffer, the wanted half is handed over and written,
            # the other half has to stay NaN
            for want in ((True, False), (False, True)):
                buf = torch.full((n * h * w * (c0 + c1),), float("nan")).to(dev)
                half0, half1 = buf[:n * h * w * c0].view(n, h, w, c0), buf[n * h * w * c0:].view(n, h, w, c1)
                dx0, dx1, dga, dbe = run(slices=slices, want=want, dx=half0 if want[0] else None, dx2=half1 if want[1] else None)
                wanted, other, r = (half0, half1, ref[0]) if want[0] else (half1, half0, ref[1])
                assert (dx1 if want[0] else dx0) is None
                assert bool(torch.isnan(other).all()), (case, name, want, "the unwanted source's memory was written")
                errs = [rel_err(wanted, r), rel_err(dga, ref[2]), rel_err(dbe, ref[3])]
                worst = max(worst, max(errs))
                assert max(errs) < TOL_OP, (case, name, want, errs)
            # the reduction, then ssde_prologue_bwd
            errs = _errors(run(slices=slices, one_call=False), ref, c1)
            worst = max(worst, max(errs))
            assert max(errs) < TOL_OP, (case, name, "two calls", errs)
    print("gn backward call forms %s vs fp64: largest error %.3g" % (case_id(case), worst))
    return worst


def _ref64_elementwise(x, silu, mask, dy):
    """fp64 gradient of  mask * act(x)  for the output gradient dy; act = SiLU or the identity"""
    x = x.double().requires_grad_()
    y = F.silu(x) if silu else x * 1.0
    if mask is not None:
        y = y * mask.double()
    y.backward(dy.double())
    return x.grad


def check_prologue_bwd(dev, case, dropout):
    """ssde_prologue_bwd on its own in SiLU-only and plain mode (the latter without any x) on a column slice of dp, the columns
    around it NaN.  Without dropout: source 0 accumulates onto a base, source 1 is written into NaN, scale 0.3.  With dropout:
    both written into NaN; the zeros of the result are the zeros of the restated mask, exactly"""
    ops, L = _ops()
    n, h, w, c0, c1, dp_ld, dp_off = case
    C = c0 + c1
    g = torch.Generator().manual_seed(31 * n + 7 * h * w + C)
    xc = torch.randn(n, h, w, C, generator=g) * 1.5 + 2.0 + torch.randn(1, 1, 1, C, generator=g)
    dy = torch.randn(n, h, w, C, generator=g) + 0.5
    dp = torch.full((n, h, w, dp_ld), float("nan"))
    dp[..., dp_off:dp_off + C] = dy
    base = torch.randn(n, h, w, c0, generator=g)
    keep = _keep(n, h, w, C) if dropout else None
    d = lambda t: t.to(dev)  # noqa: E731
    xa, xb = d(xc[..., :c0].contiguous()), d(xc[..., c0:].contiguous()) if c1 else None
    scale, worst = 0.3, 0.0
    for silu in (True, False):
        ref = scale * _ref64_elementwise(xc, silu, keep, dy)
        g0 = d(torch.full((n, h, w, c0), float("nan")) if dropout else base.clone())
        g1 = d(torch.full((n, h, w, c1), float("nan"))) if c1 else None
        common = dict(dropout=_drop(dev) if dropout else None, scale=scale, acc=(not dropout, False), dp_off=dp_off)
        if silu:
            ops.prologue_bwd(xa, d(dp), L.PRO_SILU, g0, g1, x2=xb, **common)
        else:
            ops.prologue_bwd(None, d(dp), L.PRO_NONE, g0, g1, c0=c0, c1=c1, **common)
        got = torch.cat([g0.cpu() if dropout else g0.cpu() - base] + ([g1.cpu()] if c1 else []), -1)
        assert bool(torch.isfinite(got).all()), (case, silu)
        errs = [rel_err(got[..., :c0], ref[..., :c0])] + ([rel_err(got[..., c0:], ref[..., c0:])] if c1 else [])
        worst = max(worst, max(errs))
        assert max(errs) < TOL_ELEM, (case, "silu" if silu else "plain", "dropout" if dropout else "no dropout", errs)
        if dropout:
            unmasked_zero = _ref64_elementwise(xc, silu, None, dy) == 0
            assert bool((got[keep == 0] == 0).all()), (case, silu, "a dropped element has a gradient")
            assert torch.equal(got == 0, (keep == 0) | unmasked_zero), (case, silu, "zeros are not the mask's")
    print("prologue_bwd %s %s vs fp64: largest error %.3g" % (case, "dropout" if dropout else "no dropout", worst))
    return worst
