"""FIR resampling with any kernel (up to 16 x 16 taps, negative pads, any `fir_kernel`): checks shared by the CPU-emulated
suite (tests/test_fir_wide_cpu.py) and the GPU suite (tests/test_fir_wide_gpu.py).

Reference: oracle/unet_oracle.upfirdn2d / upsample_2d / downsample_2d (the restatement of upfirdn2d_native) in float64.

Op-level bound, derived: an output is a sum of T = kh * kw fp32 products accumulated in fp32 (with or without fused
multiply-add), so |y - ref| <= gamma_T * sum |w| |x| with gamma_T < (T + 2) * 2^-24 for T <= 256 (the + 2 covers the rounding
of the accumulate-into-destination add and the second-order terms); sum |w| |x| is the same oracle call on |x| with |taps|.
Launches with the GroupNorm + SiLU prologue use positive normalised taps and the suite's 1e-5 rel_err
(_train_checks.check_upfirdn_tiles): the prologue's own rounding is not part of the sum above.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import _util
import _fir_util as FU
from _util import rel_err
from _train_checks import nhwc, nchw

U24 = 2.0 ** -24

TAPS = [(5, 5), (6, 6), (7, 3), (16, 16), (3, 3)]
UPDOWN = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2)]
CHANNELS = [32, 64, 36, 4]                     # tiled, two channel chunks, general, general (the image pyramids)
SIZES = [(5, 5), (9, 9), (9, 17)]              # (h, w): smaller than the taps; one tile; ragged, rows of 2x cross a 16-row tile
FIXED_PADS = [(0, 0), (-1, -2), (-1, 3)]


def model_pads(k, up, down):
    """the pads the networks use with a k-tap kernel (models/up_or_down_sampling.py:144-257): upsample_2d where the launch
    upsamples, downsample_2d where it only decimates, conv_downsample_2d's (in front of a 3x3) at stride 1"""
    if up > 1:
        p = k - up
        return ((p + 1) // 2 + up - 1, p // 2)
    if down > 1:
        p = k - down
        return ((p + 1) // 2, p // 2)
    p = k - 2 + 2
    return ((p + 1) // 2, p // 2)


def out_size(n, k, up, down, pad):
    return (n * up + pad[0] + pad[1] - k) // down + 1


def grid(taps):
    """(up, down, (h, w), pad) of one taps size; the cases whose output size is not positive are left out and counted"""
    kh, kw = taps
    cases, skipped = [], 0
    for (up, down), (h, w) in itertools.product(UPDOWN, SIZES):
        for pad in [model_pads(kw, up, down)] + FIXED_PADS:
            if out_size(h, kh, up, down, pad) < 1 or out_size(w, kw, up, down, pad) < 1:
                skipped += 1
                continue
            cases.append((up, down, (h, w), pad))
    return cases, skipped


def check_grid_is_mostly_runnable():
    total = skipped = 0
    for taps in TAPS:
        cases, s = grid(taps)
        total, skipped = total + len(cases) + s, skipped + s
    # the (5, 5)-pad cases of the 4x4 kernel all run
    assert total == len(TAPS) * len(UPDOWN) * len(SIZES) * (1 + len(FIXED_PADS))
    assert skipped * 4 < total, (skipped, total)
    return skipped, total


def random_taps(g, kh, kw):
    """asymmetric and signed: a missing flip or a swapped axis changes the result"""
    return torch.randn(kh, kw, generator=g) + 0.25


def bound(x64, k, up, down, pad, extra=0.0):
    from oracle import unet_oracle as uo
    a = uo.upfirdn2d(x64.abs(), k.double().abs(), up=up, down=down, pad=pad)
    return (k.numel() + 2) * U24 * (a + extra)


def tile_shape(c, up, down):
    return c % 32 == 0 and up <= 2 and down <= 2 and not (up == 2 and down == 2)


def check_op_grid(dev, taps, pad55=False):
    """every case of the grid for one taps size, every channel count, on the default route; on the shapes the tiled kernels take
    also with SSDE_FIRF_GENERAL and SSDE_FIRF_TILED, each against the reference and against each other"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    from oracle import unet_oracle as uo
    kh, kw = taps
    g = torch.Generator().manual_seed(1000 * kh + kw + (7 if pad55 else 0))
    k = random_taps(g, kh, kw)
    if pad55:        # 4x4 taps with pad (5, 5): the gradient pads of such a launch are negative (op/upfirdn2d.py:111-116)
        cases = [(up, down, hw, (5, 5)) for (up, down), hw in itertools.product(UPDOWN, SIZES)]
    else:
        cases, _ = grid(taps)
    launches = 0
    for up, down, (h, w), pad in cases:
        x = torch.randn(2, max(CHANNELS), h, w, generator=g)
        x64 = x.double()
        ref = uo.upfirdn2d(x64, k.double(), up=up, down=down, pad=pad)
        tol = bound(x64, k, up, down, pad)
        for c in CHANNELS:
            xd = nhwc(x[:, :c]).to(dev)
            routes = [0] + ([L.FIRF_GENERAL, L.FIRF_TILED] if tile_shape(c, up, down) else [])
            ys = []
            for flags in routes:
                y = nchw(ops.upfirdn2d_nhwc(xd, k, up=up, down=down, pad=pad, flags=flags).cpu()).double()
                launches += 1
                assert tuple(y.shape) == tuple(ref[:, :c].shape), (taps, up, down, (h, w), pad, c, flags)
                err = (y - ref[:, :c]).abs()
                assert bool((err <= tol[:, :c]).all()), (taps, up, down, (h, w), pad, c, flags, float((err / tol[:, :c].clamp_min(1e-300)).max()))
                ys.append(y)
            for y in ys[1:]:          # the tiled kernels and the one-lane-per-output kernel agree within the same bound
                assert bool(((y - ys[0]).abs() <= tol[:, :c]).all()), (taps, up, down, (h, w), pad, c)
    return launches


def check_prologue_dual_accumulate(dev):
    """dst2, accumulate and the GroupNorm + SiLU prologue on a 6x6 down-2 and a 6x6 up-2 launch, on the tiled kernel and on the
    one-lane-per-output kernel.  The fused prologue needs channels-per-group % 4 == 0 (include/ssde.h), so 32 channels in 16 groups
    cannot run: the launches take 32 channels in 8 groups (one channel chunk) and 64 channels in 16 groups (two)."""
    for c, groups in [(32, 8), (64, 16)]:
        _check_prologue_dual_accumulate(dev, c, groups)


def _check_prologue_dual_accumulate(dev, c, groups):
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    from oracle import unet_oracle as uo
    g = torch.Generator().manual_seed(66)
    k1 = torch.tensor(uo.setup_fir_kernel(FU.FIR_KERNELS["fir6"]))
    x = torch.randn(2, c, 12, 20, generator=g) + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    xd = nhwc(x).to(dev)
    mean, rstd = ops.groupnorm_stats(xd, groups)
    act = F.silu(F.group_norm(x.double(), groups, gamma.double(), beta.double(), 1e-6))
    for up, down, gain in [(1, 2, 1.0), (2, 1, 4.0)]:
        k = k1 * gain
        pad = model_pads(6, up, down)
        ref_act = uo.upfirdn2d(act, k.double(), up=up, down=down, pad=pad)
        ref_raw = uo.upfirdn2d(x.double(), k.double(), up=up, down=down, pad=pad)
        tol_raw = bound(x.double(), k, up, down, pad)
        for flags in (0, L.FIRF_GENERAL):
            y, y2 = ops.upfirdn2d_nhwc(xd, k, up=up, down=down, pad=pad, pro=L.PRO_GN_SILU,
                                       gn=(mean, rstd, gamma.to(dev), beta.to(dev), groups), dual=True, flags=flags)
            e = rel_err(nchw(y.cpu()), ref_act)
            assert e < 1e-5, (up, down, flags, e)
            assert bool(((nchw(y2.cpu()).double() - ref_raw).abs() <= tol_raw).all()), (up, down, flags)
            base = torch.randn(y.shape, generator=g)
            acc = base.clone().to(dev)
            ops.upfirdn2d_nhwc(xd, k, up=up, down=down, pad=pad, accumulate_into=acc, flags=flags)
            # one more rounding, of |base + result| <= |base| + sum |w| |x|
            tol_acc = bound(x.double(), k, up, down, pad, extra=nchw(base).double().abs())
            assert bool(((nchw(acc.cpu()).double() - (nchw(base).double() + ref_raw)).abs() <= tol_acc).all()), (up, down, flags)


def check_refusals(dev):
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    import ctypes as C
    x = torch.randn(1, 9, 9, 32).to(dev)
    for shape in [(17, 17), (17, 3), (3, 17)]:
        try:
            ops.upfirdn2d_nhwc(x, torch.ones(*shape))
        except ValueError as e:
            assert "16" in str(e)
        else:
            raise AssertionError("a %dx%d kernel must be refused" % shape)
    for kw in [dict(pad=(0, 0)), dict(pad=(-5, -5), up=1), dict(pad=(2, 2), down=2)]:      # 9 (+ pads) < 16 taps
        try:
            ops.upfirdn2d_nhwc(x, torch.ones(16, 16), **kw)
        except (ValueError, L.SsdeError):
            pass
        else:
            raise AssertionError("a non-positive output size must be refused")
    # the library's own guards, below the Python wrapper: the tap limit is named, a non-positive size is an error before any launch
    taps = torch.ones(17 * 17).to(dev)
    dst = torch.zeros(1, 9, 9, 32).to(dev)
    a = L.UpfirdnArgs()
    a.src.p0, a.src.c0, a.dst, a.taps = x.data_ptr(), 32, dst.data_ptr(), taps.data_ptr()
    a.n, a.h_in, a.w_in, a.c, a.up, a.down = 1, 9, 9, 32, 1, 1
    a.kh, a.kw, a.pad0, a.pad1, a.h_out, a.w_out = 17, 17, 8, 8, 9, 9
    lib = L.load()
    assert lib.ssde_upfirdn2d(C.byref(a), ops._stream()) != 0 and b"16" in lib.ssde_last_error()
    a.kh, a.kw, a.pad0, a.pad1, a.h_out, a.w_out = 16, 16, 3, 3, 0, 0          # 9 + 6 - 16 < 0: C division would call it 1 x 1
    assert lib.ssde_upfirdn2d(C.byref(a), ops._stream()) != 0 and b"not positive" in lib.ssde_last_error()
    a.pad0, a.pad1, a.h_out, a.w_out, a.taps = 8, 8, 10, 10, None                # past 4x4 without the taps array
    assert lib.ssde_upfirdn2d(C.byref(a), ops._stream()) != 0 and b"taps" in lib.ssde_last_error()
    assert float(dst.abs().max()) == 0.0


def check_op_package(dev, upfirdn2d):
    """score_sde_pytorch_amd.op.upfirdn2d (NCHW, 3 channels, 6x6 taps): forward, torch.autograd.grad and the double backward
    against the oracle's autograd in float64, a negative-pad case, and the refused backward of a rectangular kernel"""
    from oracle import unet_oracle as uo
    g = torch.Generator().manual_seed(606)
    k = random_taps(g, 6, 6)
    for up, down, pad in [(2, 1, model_pads(6, 2, 1)), (1, 2, model_pads(6, 1, 2)), (1, 1, model_pads(6, 1, 1)), (1, 1, (-1, -2)),
                          (2, 1, (-1, 3))]:
        x = torch.randn(2, 3, 10, 10, generator=g)
        xr = x.double().requires_grad_()
        ref = uo.upfirdn2d(xr, k.double(), up=up, down=down, pad=pad)
        go = torch.randn(ref.shape, generator=g)
        ggx = torch.randn(x.shape, generator=g)
        gor = go.double().requires_grad_()
        (gx_ref,) = torch.autograd.grad(ref, xr, gor, create_graph=True)
        (ggo_ref,) = torch.autograd.grad((gx_ref * ggx.double()).sum(), gor)
        # bounds: the same sums over |.|
        xa = x.double().abs().requires_grad_()
        ra = uo.upfirdn2d(xa, k.double().abs(), up=up, down=down, pad=pad)
        (gx_abs,) = torch.autograd.grad(ra, xa, go.double().abs())
        scale = (k.numel() + 2) * U24
        xd = x.to(dev).requires_grad_()
        gd = go.to(dev).requires_grad_()
        y = upfirdn2d(xd, k.to(dev), up=up, down=down, pad=pad)
        assert tuple(y.shape) == tuple(ref.shape)
        assert bool(((y.detach().cpu().double() - ref.detach()).abs() <= scale * ra.detach()).all()), (up, down, pad)
        (gx,) = torch.autograd.grad(y, xd, gd, create_graph=True)
        assert bool(((gx.detach().cpu().double() - gx_ref.detach()).abs() <= scale * gx_abs).all()), (up, down, pad)
        (ggo,) = torch.autograd.grad((gx * ggx.to(dev)).sum(), gd)
        # d/d(go) of <gx, ggx> is the forward op applied to ggx
        tol = scale * uo.upfirdn2d(ggx.double().abs(), k.double().abs(), up=up, down=down, pad=pad)
        assert bool(((ggo.cpu().double() - ggo_ref).abs() <= tol).all()), (up, down, pad)
    # a rectangular kernel: the forward works, its backward needs one pad pair per axis
    k73 = random_taps(g, 7, 3)
    x = torch.randn(2, 3, 10, 10, generator=g)
    xd = x.to(dev).requires_grad_()
    y = upfirdn2d(xd, k73.to(dev), up=1, down=1, pad=(3, 3))
    ref = uo.upfirdn2d(x.double(), k73.double(), pad=(3, 3))
    assert bool(((y.detach().cpu().double() - ref).abs() <= bound(x.double(), k73, 1, 1, (3, 3))).all())
    try:
        y.sum().backward()
    except NotImplementedError:
        pass
    else:
        raise AssertionError("the backward of a 7x3 kernel must be refused")


# ---- model level ----------------------------------------------------------------------------------------------------------
TOL_FWD = 1e-4          # tests/test_unet_gpu.py


def _model(cfg, dev):
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    _util.load_seeded(model, seed=1)
    return model.to(dev).eval()


def check_forward_golden(dev, fir, net):
    """one forward of a small net with a 3-tap / 6-tap fir_kernel against the reference's (tools/gen_golden_fir.py)"""
    from score_sde_pytorch_amd import engine as E
    import os
    gold = np.load(os.path.join(_util.GOLDEN, "unet_small_%s.npz" % fir))
    x, cond, y_ref = (torch.from_numpy(gold["%s/%s" % (net, k)]) for k in ("x", "cond", "y"))
    model = _model(FU.forward_config(net, fir), dev)
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    y = eng.forward(x.to(dev), cond.to(dev)).cpu()
    assert y.shape == y_ref.shape and torch.isfinite(y).all()
    e, ps = rel_err(y, y_ref), _util.per_sample_err(y, y_ref)
    print("forward %s %s: rel_err %.3g per-sample %.3g" % (fir, net, e, ps))
    assert e < TOL_FWD, e
    assert ps < 2 * TOL_FWD, ps


def check_dry_lowering_cifar():
    """ve/cifar10_ncsnpp_continuous with the 6-tap kernel lowers at batch 256; every FIR launch carries the 6x6 taps by pointer"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    cfg = _util.cfgs.get_config("ve/cifar10_ncsnpp_continuous")
    cfg.model.fir_kernel = list(FU.FIR_KERNELS["fir6"])
    model = _model(cfg, "cpu")
    eng = E.UNetEngine(model, 256, 32, 32, torch.device("cpu"))
    lds = eng.validate_plans()
    assert len(lds) > 0 and min(lds) > 0
    firs = [eng.program.ops[i].u.fir for i in range(eng.program.n) if eng.program.ops[i].kind == L.OP_UPFIRDN]
    assert len(firs) > 0 and all(f.kh == 6 and f.kw == 6 and f.taps for f in firs)
    # upsample_2d, downsample_2d and conv_downsample_2d (the residual input pyramid) with six taps
    assert {(f.up, f.down, f.pad0, f.pad1) for f in firs} == {(2, 1, 3, 2), (1, 2, 2, 2), (1, 1, 3, 3)}
    assert all(bool(f.dst2) == (f.up + f.down == 3) for f in firs)          # act(GroupNorm(x)) and x still share one launch
    assert len(eng.b.fir_taps) == 2           # one kept tensor per distinct kernel (gain 4 up, gain 1 down)


def check_too_long_fir_kernel_raises():
    from score_sde_pytorch_amd import engine as E
    cfg = _util.small_config("ncsnpp")
    cfg.model.fir_kernel = [1.0] * 17
    model = _model(cfg, "cpu")
    try:
        E.UNetEngine(model, 2, 16, 16, torch.device("cpu"))
    except ValueError as e:
        assert "16" in str(e)
    else:
        raise AssertionError("a 17-tap fir_kernel must be refused at lowering time")


def check_unet_plan_round_trip(dev, net="ffhq"):
    """a U-Net plan of a 6-tap small net exports, reloads through plan_export.LoadedPlan and reproduces the engine's bits: the
    taps tensors travel as constant regions and their pointers are relocated"""
    from score_sde_pytorch_amd import engine as E, plan_export as P, _lib as L
    cfg = FU.forward_config(net, "fir6")
    model = _model(cfg, dev)
    x, cond = FU.forward_inputs(cfg, 2, seed=5)
    eng = E.UNetEngine(model, 2, x.shape[2], x.shape[3], torch.device(dev))
    y = eng.forward(x.to(dev), cond.to(dev)).clone()
    blob = P.export_unet_plan(eng)
    n_big = sum(1 for i in range(eng.program.n) if eng.program.ops[i].kind == L.OP_UPFIRDN and eng.program.ops[i].u.fir.taps)
    assert n_big > 0
    del eng                                    # the plan owns its copy of the taps
    plan = P.LoadedPlan(blob)
    try:
        y2 = plan.unet_forward(x.to(dev).contiguous(), cond.to(dev).contiguous())
    finally:
        plan.close()
    assert torch.equal(y.cpu(), y2.cpu())


def check_pc_plan_matches_python_sampler():
    """ssde_pc_reset / ssde_pc_run / ssde_pc_state on the exported sampler plan of the 6-tap small net: same seed word, same
    iterations -> the Python-driven FusedPCSampler's state bit for bit (op-by-op launch and graph replay).  GPU only, as the
    plan test of the 4-tap net it follows (tests/test_plan_c_host.py)."""
    import ctypes as C
    from score_sde_pytorch_amd import sde_lib, sampling, plan_export, _lib as L
    model = _model(FU.forward_config("ncsnpp", "fir6"), "cuda")
    N, B = 6, 4
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=N)
    sampler = sampling.get_pc_sampler(sde, (B, 3, 16, 16), sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector,
                                      lambda v: v, snr=0.16, n_steps=1, continuous=True, denoise=False, eps=1e-5, device="cuda")
    x_T = torch.randn(B, 3, 16, 16, generator=torch.Generator().manual_seed(3)) * 50
    ref, _ = sampler(model, x_init=x_T, seed=77, use_graph=False)
    assert torch.isfinite(ref).all()
    blob = plan_export.export_pc_plan(sampler.engine)
    plan = plan_export.LoadedPlan(blob)
    try:
        assert plan.header.kind == plan_export.PLAN_PC and plan.header.sde_steps == N
        lib = plan.lib
        xd = x_T.cuda().contiguous()
        out = torch.empty_like(xd)
        for use_graph in (0, 1):
            st = torch.cuda.Stream()
            L.check(lib.ssde_pc_reset(plan.handle, C.c_void_p(xd.data_ptr()), 77, C.c_void_p(st.cuda_stream)))
            L.check(lib.ssde_pc_run(plan.handle, N, use_graph, C.c_void_p(st.cuda_stream)))
            L.check(lib.ssde_pc_state(plan.handle, C.c_void_p(out.data_ptr()), None, C.c_void_p(st.cuda_stream)))
            st.synchronize()
            assert torch.equal(out.cpu(), ref.cpu()), use_graph
    finally:
        plan.close()
