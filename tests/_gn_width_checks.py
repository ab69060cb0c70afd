"""Checks of the GroupNorm fallback for channels-per-group that are no multiple of 4 (ssde_groupnorm_stats on any width,
ssde_gn_apply, ssde_gn_apply_bwd and their lowering), shared by the emulator suite (tests/test_gn_width_cpu.py) and the GPU
suite (tests/test_gn_width_gpu.py).  Tolerances are the project's: element-wise 2e-6, contraction 2e-5, a whole
forward 1e-4 (2e-6 for the small nets on the emulator's exact-fp32 arithmetic), gradients 2e-4."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import _util
import _gn_width_util as W
import _train_checks as T
from _util import rel_err

TOL_ELEM, TOL_CONTRACT, TOL_FWD, TOL_GRAD = 2e-6, 2e-5, 1e-4, 2e-4

# (c0, c1, groups): 6 per group with groups that straddle the two halves (group 21 = channels 126..131), 5, 7, and 5 with a
# last quad that ends a group mid-quad
KERNEL_SHAPES = [(128, 64, 32), (160, 0, 32), (96, 128, 32), (20, 0, 4)]
KERNEL_MAPS = [4, 8]
KERNEL_BATCH = 3


def _case(c0, c1, hw_side, seed):
    g = torch.Generator().manual_seed(seed)
    n, C = KERNEL_BATCH, c0 + c1
    xc = torch.randn(n, hw_side, hw_side, C, generator=g) * 1.5 + 2.0 + torch.randn(1, 1, 1, C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(n, hw_side, hw_side, C, generator=g)
    return xc, gamma, beta, dy


def _ref64(xc, groups, gamma, beta, silu, mask, dy, eps=1e-6):
    """fp64: statistics, y = mask * act(GroupNorm(x)) and its gradients, NHWC"""
    x = xc.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    ga, be = gamma.double().requires_grad_(), beta.double().requires_grad_()
    n, C = x.shape[0], x.shape[1]
    xg = x.detach().reshape(n, groups, -1)
    mean, var = xg.mean(2), xg.var(2, unbiased=False)
    y = F.group_norm(x, groups, ga, be, eps)
    if silu:
        y = F.silu(y)
    if mask is not None:
        y = y * mask.double().permute(0, 3, 1, 2)
    y.backward(dy.double().permute(0, 3, 1, 2))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()      # noqa: E731
    return mean, 1.0 / torch.sqrt(var + eps), nhwc(y.detach()), nhwc(x.grad), ga.grad, be.grad


def check_kernels(dev, c0, c1, groups, side):
    """statistics, apply (GroupNorm and GroupNorm + SiLU, with and without dropout) and the adjoint (dx into both halves,
    accumulated and written; dgamma, dbeta) against fp64"""
    from score_sde_pytorch_amd import hipops as ops
    d = lambda t: t.to(dev)  # noqa: E731
    xc, gamma, beta, dy = _case(c0, c1, side, seed=100 * c0 + c1 + side)
    n, C, hw = xc.shape[0], c0 + c1, side * side
    xa = d(xc[..., :c0].contiguous())
    xb = d(xc[..., c0:].contiguous()) if c1 else None
    drop_p, salt, seed_word = 0.25, 0x1234567, 77
    seed_t = torch.tensor([seed_word], dtype=torch.int32).to(dev)
    thresh = min(int(round(drop_p * 2.0 ** 32)), 2 ** 32 - 1)
    keep = torch.from_numpy(T.hash_keep(np.arange(n * hw * C, dtype=np.uint64), seed_word ^ salt, thresh, 1.0 / (1.0 - drop_p))
                            ).reshape(n, side, side, C)
    assert 0.6 < float((keep > 0).float().mean()) < 0.9
    for slices in (1, 2):
        mean, rstd = ops.groupnorm_stats(xa, groups, 1e-6, xb, slices=slices)
        m64, r64 = _ref64(xc, groups, gamma, beta, False, None, dy)[:2]
        assert rel_err(mean, m64) < TOL_ELEM and rel_err(rstd, r64) < TOL_ELEM, (slices, rel_err(mean, m64), rel_err(rstd, r64))
    gn = (mean, rstd, d(gamma), d(beta), groups)
    for silu in (False, True):
        for mask in (None, keep):
            drop = (drop_p, seed_t, salt) if mask is not None else None
            _, _, y64, dx64, dg64, db64 = _ref64(xc, groups, gamma, beta, silu, mask, dy)
            y = ops.groupnorm_apply(xa, gn, xb, silu=silu, drop=drop)
            assert tuple(y.shape) == (n, side, side, C)
            if mask is not None:            # the mask itself is exact
                assert torch.equal(y.cpu() == 0, (keep == 0) | (y64 == 0).to(torch.bool))
            assert rel_err(y, y64) < TOL_ELEM, ("apply", silu, mask is not None, rel_err(y, y64))
            # adjoint: p0's gradient accumulated onto a base, p1's written
            base = torch.randn(n, side, side, c0, generator=torch.Generator().manual_seed(1))
            g0 = d(base.clone())
            slices = 2 if hw >= 64 else 1
            dx0, dx1, dga, dbe = ops.groupnorm_apply_bwd(d(dy), xa, gn, xb, silu=silu, drop=drop, slices=slices, g0=g0)
            assert rel_err(dx0.cpu() - base, dx64[..., :c0]) < TOL_CONTRACT, ("dx0", silu, rel_err(dx0.cpu() - base, dx64[..., :c0]))
            if c1:
                assert rel_err(dx1, dx64[..., c0:]) < TOL_CONTRACT, ("dx1", silu, rel_err(dx1, dx64[..., c0:]))
            assert rel_err(dga, dg64) < TOL_CONTRACT and rel_err(dbe, db64) < TOL_CONTRACT, (rel_err(dga, dg64), rel_err(dbe, db64))
            # bit-reproducible
            again = ops.groupnorm_apply_bwd(d(dy), xa, gn, xb, silu=silu, drop=drop, slices=slices, g0=d(base.clone()))
            assert all(torch.equal(a, b) for a, b in zip((dx0, dga, dbe), (again[0], again[2], again[3])))


def check_any_width_kernel_has_the_quad_kernels_bits(dev):
    """4 channels per group, 64 + 32 channels: the any-width statistics kernel (forced) against the quad kernel, bit for bit"""
    from score_sde_pytorch_amd import hipops as ops
    xc, _, _, _ = _case(64, 32, 8, seed=5)
    xa, xb = xc[..., :64].contiguous().to(dev), xc[..., 64:].contiguous().to(dev)
    for slices in (1, 2):
        m0, r0 = ops.groupnorm_stats(xa, 24, 1e-6, xb, slices=slices)
        m1, r1 = ops.groupnorm_stats(xa, 24, 1e-6, xb, slices=slices, any_width=True)
        assert torch.equal(m0, m1) and torch.equal(r0, r1), slices


def small_model(dev, dropout=0.0, cfg=None):
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = cfg or W.small_config(dropout=dropout)
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    sd = {k: v.clone() for k, v in _util.load_seeded(model, seed=1).items()}
    sd["sigmas"] = model.sigmas.clone()
    return cfg, model.to(dev), sd


def program_facts(prog):
    """(op kinds, widths of every GroupNorm a consumer applies itself)"""
    from score_sde_pytorch_amd import _lib as L
    kinds, fused = [], []
    for i in range(prog.n):
        op = prog.ops[i]
        kinds.append(int(op.kind))
        srcs = {L.OP_CONV: lambda u: (u.conv.main, u.conv.aux), L.OP_UPFIRDN: lambda u: (u.fir.src,),
                L.OP_WGRAD: lambda u: (u.wgrad.src,), L.OP_GN_BWD_REDUCE: lambda u: (u.gn_bwd.src,),
                L.OP_PROLOGUE_BWD: lambda u: (u.pro_bwd.src,)}.get(int(op.kind), lambda u: ())(op.u)
        for s in srcs:
            if s.p0 and s.gn_groups and s.pro_mode in (L.PRO_GN, L.PRO_GN_SILU):
                fused.append((s.c0 + s.c1) // s.gn_groups)
    return kinds, fused


def check_small_net_forward(dev, tol):
    """the nf = 16 network against the REFERENCE's forward (tests/golden/unet_small_nf16.npz)"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    gold = np.load(os.path.join(_util.GOLDEN, "unet_small_nf16.npz"))
    cfg, model, _ = small_model(dev)
    x, sig, y_ref = (torch.from_numpy(gold[k]) for k in ("x", "cond", "y"))
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    kinds, fused = program_facts(eng.program)
    assert kinds.count(L.OP_GN_APPLY) >= 1 and all(w % 4 == 0 for w in fused), (kinds.count(L.OP_GN_APPLY), fused)
    y = eng.forward(x.to(dev), sig.to(dev))
    err = rel_err(y, y_ref)
    print("small nf16 forward vs reference: rel err %.3g" % err)
    assert err < tol, err
    y2 = eng.forward(x.to(dev), sig.to(dev))
    assert torch.equal(y, y2)
    return eng, y


def check_small_net_grads(dev, fwd_tol=TOL_FWD):
    """every parameter gradient and the input gradient against autograd through the CPU oracle"""
    from score_sde_pytorch_amd import backward as B, _lib as L
    cfg, model, sd = small_model(dev)
    x, sig = W.forward_inputs(cfg)
    gout = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
    y_ref, gx_ref, ref = T.oracle_grads(cfg, sd, x, sig, gout)
    R = cfg.data.image_size
    eng = B.TrainEngine(model, x.shape[0], R, R, torch.device(dev), input_grad=True, dropout=False)
    kinds, fused = program_facts(eng.program)
    assert kinds.count(L.OP_GN_APPLY) >= 1 and kinds.count(L.OP_GN_APPLY_BWD) >= 1 and all(w % 4 == 0 for w in fused)
    y = eng.forward_train(x.to(dev), sig.to(dev)).clone()
    assert rel_err(y, y_ref) < fwd_tol, rel_err(y, y_ref)
    eng.backward(gout.to(dev))
    e = rel_err(eng.gx_view(), gx_ref)
    assert e < TOL_GRAD, e
    worst = T.compare_param_grads(model, eng.flat, ref, tol=TOL_GRAD)
    print("small nf16 gradients vs oracle autograd: input %.3g, worst parameter %.3g" % (e, worst))
    g1, gx1 = eng.flat.grad.clone(), eng.gx_view().clone()
    eng.forward_train(x.to(dev), sig.to(dev))
    eng.backward(gout.to(dev))
    assert torch.equal(g1, eng.flat.grad) and torch.equal(gx1, eng.gx_view())


def check_small_net_dropout(dev):
    """the dropout = 0.1 copy in train mode: Dropout_0 of the blocks whose GroupNorm_1 is materialised goes through ssde_gn_apply;
    the seed word decides the mask (same seed: same bits, another seed: another result), gradients stay finite and reproducible"""
    from score_sde_pytorch_amd import backward as B
    cfg, model, _ = small_model(dev, dropout=0.1)
    x, sig = W.forward_inputs(cfg)
    gout = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
    R = cfg.data.image_size
    eng = B.TrainEngine(model, x.shape[0], R, R, torch.device(dev), input_grad=True, dropout=True)
    outs = {}
    for tag, seed in (("a", 5), ("b", 5), ("c", 6)):
        y = eng.forward_train(x.to(dev), sig.to(dev), seed=seed).clone()
        eng.backward(gout.to(dev))
        outs[tag] = (y, eng.flat.grad.clone(), eng.gx_view().clone())
    assert all(torch.equal(p, q) for p, q in zip(outs["a"], outs["b"]))
    assert not torch.equal(outs["a"][0], outs["c"][0])
    assert all(bool(torch.isfinite(t).all()) for t in outs["a"])


def check_train_steps_against_reference_run(dev):
    """three steps of losses.get_step_fn on the nf = 16 network against the REFERENCE's run (tests/golden/train_small_nf16.npz)"""
    gold = np.load(os.path.join(_util.GOLDEN, "train_small_nf16.npz"))
    name, case = W.TRAIN_NAME, W.TRAIN_CASE
    from score_sde_pytorch_amd.models import utils as mutils, ema as ema_mod
    from score_sde_pytorch_amd import losses, sde_lib
    _, _, _, continuous, reduce_mean, lw = case
    cfg = W.train_config()
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    init = {k: v.clone() for k, v in _util.load_seeded(model, seed=1).items()}
    model = model.to(dev)
    sde = _util.train_case_sde(sde_lib, case, cfg)
    opt = losses.get_optimizer(cfg, model.parameters())
    ema = ema_mod.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    optimize_fn = losses.optimization_manager(cfg)
    train_step = losses.get_step_fn(sde, train=True, optimize_fn=optimize_fn, reduce_mean=reduce_mean, continuous=continuous,
                                    likelihood_weighting=lw)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    inputs = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)
    ref_loss = gold[name + "/loss"]
    losses_ = []
    for step in range(_util.TRAIN_STEPS):
        batch, u, labels, z = inputs[step]
        with _util.inject_rng(u, labels, z):
            loss = train_step(state, batch.to(dev))
        losses_.append(float(loss))
        assert abs(float(loss) - ref_loss[step]) <= 1e-5 * abs(ref_loss[step]), (step, float(loss), ref_loss[step])
        T._compare_with_reference_step(gold, name, step, state, init, last=step == _util.TRAIN_STEPS - 1)
    return losses_, model


def check_plan_round_trip(dev):
    """export a plan blob of the nf = 16 network, load and run it through the plan entries: the engine's bits"""
    from score_sde_pytorch_amd import engine as E, plan_export as P, _lib as L
    cfg, model, _ = small_model(dev)
    x, sig = W.forward_inputs(cfg)
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    y = eng.forward(x.to(dev), sig.to(dev))
    blob = P.export_unet_plan(eng)
    hdr = P.PlanHeader.from_buffer_copy(blob[: __import__("ctypes").sizeof(P.PlanHeader)])
    assert hdr.abi_version == L.ABI_VERSION == 13
    plan = P.LoadedPlan(blob)
    try:
        y2 = plan.unet_forward(x.to(dev).contiguous(), sig.to(dev).contiguous())
    finally:
        plan.close()
    assert torch.equal(y, y2)
