"""Checks of the NCSN++ constructor switches beyond the shipped configs (models/ncsnpp.py of the reference): resblock_type = 'ddpm'
(ResnetBlockDDPMpp with layerspp.Downsample / Upsample), progressive_combine = 'cat' (layerspp.Combine, materialised by
ssde_concat), and the residual input pyramid without FIR (progressive_input = 'residual') -- as far as the reference itself can
run them (UNRUNNABLE below: what it builds and then raises on is refused by the constructor here).  Shared by the
emulator suite (tests/test_arch_cpu.py) and the GPU suite (tests/test_arch_gpu.py); the cases at the top are also what
tools/gen_golden_arch.py records from the reference.  Tolerances are the project's (tests/_gn_width_checks.py): a whole forward
1e-4, gradients 2e-4; the concatenation is a copy and is compared bit for bit."""
import ctypes as C
import json
import os
import types

import numpy as np
import torch

import _util
import _gn_width_checks as K
import _train_checks as T
from _util import rel_err
from _act_checks import model_of, pytest_raises

TOL_FWD, TOL_GRAD = K.TOL_FWD, K.TOL_GRAD
SSDE_EINVAL = -22

# ---- the recorded cases (tools/gen_golden_arch.py) -----------------------------------------------------------------
# name -> (small-config kind, small_config keywords, config.model overrides); 16-px images, dropout 0
CASES = {
    # FIR up / down without convolution between DDPM blocks; the base's residual input pyramid (FIR) stays
    "ddpmblk_fir": ("ncsnpp", {}, dict(resblock_type="ddpm", resamp_with_conv=False)),
    # maps 16, 8, 4: two concatenations of different widths, and the 4x4 route.  (Combine exists only under input_skip; the
    # base's input pyramid is 'residual', under which progressive_combine is never read)
    "cat": ("ncsnpp", dict(ch_mult=(1, 2, 2)), dict(progressive_input="input_skip", progressive_combine="cat")),
    # Downsample(with_conv, no FIR) on the input pyramid: one end-padded stride-2 launch with the sum in its epilogue
    "resid_in": ("ddpmpp", {}, dict(progressive_input="residual")),
    # the new blocks, a concatenation behind a FIR Downsample, and an activation the fused prologues do not know
    "cat_ddpmblk_fir_elu": ("ncsnpp", {}, dict(resblock_type="ddpm", resamp_with_conv=False, progressive_input="input_skip",
                                               progressive_combine="cat", nonlinearity="elu")),
}
# What the reference CONSTRUCTS but cannot run: every non-FIR layerspp.Upsample calls F.interpolate(x, size, 'nearest') -- the mode
# lands in scale_factor and torch raises "only one of size or scale_factor should be defined" (models/layerspp.py:117) -- so DDPM
# blocks without FIR and progressive = 'residual' have no reference forward to record (tools/gen_golden_arch.py asserts exactly
# this failure); the constructor here refuses them, as it refuses the FIR forms that reach the broken upsample_conv_2d.
UNRUNNABLE = {
    "ddpmblk_conv": ("ddpmpp", {}, dict(resblock_type="ddpm", resamp_with_conv=True)),
    "cat_ddpmblk_elu": ("ddpmpp", {}, dict(progressive_input="input_skip", progressive_combine="cat", resblock_type="ddpm",
                                           resamp_with_conv=True, nonlinearity="elu")),
    "resid_out": ("ddpmpp", dict(ch_mult=(1, 2, 2)), dict(progressive="residual")),
    "resid_all": ("ddpmpp", {}, dict(resblock_type="ddpm", resamp_with_conv=True, progressive_input="residual",
                                     progressive="residual")),
}
FORWARD_BATCH = 3
# the training cases: name -> the SDE of the base config (tests/_util.train_case_sde), continuous loss
TRAIN_CASES = {"cat": "vesde", "resid_in": "subvpsde"}
TRAIN_PROBE_LIMIT = 5000
COT_SEED = 321
# (n, hw, c0, c1) of the concatenation launch: two blocks' worth, a ragged pixel count with the narrowest halves, one pixel with
# halves of different width, a wide half next to the narrowest
CONCAT_SHAPES = [(3, 256, 32, 64), (3, 35, 4, 4), (1, 1, 20, 12), (2, 16, 128, 4)]


def config(case):
    kind, kw, over = CASES[case] if case in CASES else UNRUNNABLE[case]
    cfg = _util.small_config(kind, **kw)
    for k, v in over.items():
        cfg.model[k] = v
    assert cfg.data.image_size == 16 and float(cfg.model.dropout) == 0.0
    return cfg


def forward_inputs(case):
    """drawn as tests/_act_checks.forward_inputs draws them: batch 3, generator seed 123"""
    cfg = config(case)
    g = torch.Generator().manual_seed(123)
    R, batch = cfg.data.image_size, FORWARD_BATCH
    x = torch.rand(batch, 3, R, R, generator=g) if not cfg.data.centered else torch.rand(batch, 3, R, R, generator=g) * 2 - 1
    if cfg.model.embedding_type == "fourier":
        cond = torch.exp(torch.rand(batch, generator=g) * (np.log(50.0) - np.log(0.01)) + np.log(0.01)).float()
        x = x + cond[:, None, None, None] * torch.randn(batch, 3, R, R, generator=g)
    else:
        cond = (torch.rand(batch, generator=g) * 999).float()
    return x, cond


def cotangent(case):
    x, _ = forward_inputs(case)
    return torch.randn(x.shape, generator=torch.Generator().manual_seed(COT_SEED))


def train_case(case):
    """the layout of a tests/_util.TRAIN_CASES entry"""
    return (CASES[case][0], {}, TRAIN_CASES[case], True, False, False)


def train_config(case):
    cfg = config(case)
    cfg.training.continuous = True
    cfg.optim.warmup = _util.TRAIN_WARMUP
    return cfg


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


# ---- 1. the concatenation launch ----------------------------------------------------------------------------------------
def _concat_case(shape):
    n, hw, c0, c1 = shape
    g = torch.Generator().manual_seed(1000 * c0 + 10 * c1 + hw)
    return torch.randn(n, hw, c0, generator=g), torch.randn(n, hw, c1, generator=g), torch.randn(n, hw, c0 + c1, generator=g)


def check_concat_launch(dev, shape):
    """ssde_concat through its wrapper against torch.cat: the same bits"""
    from score_sde_pytorch_amd import hipops as ops
    a, b, _ = _concat_case(shape)
    out = ops.concat(a.to(dev), b.to(dev))
    assert tuple(out.shape) == (shape[0], shape[1], shape[2] + shape[3])
    assert torch.equal(out.cpu(), torch.cat([a, b], -1))


def check_concat_program(dev, shape):
    """a program of one SSDE_OP_CONCAT"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    n, hw, c0, c1 = shape
    a, b, _ = _concat_case(shape)
    a, b = a.to(dev), b.to(dev)
    out = torch.full((n, hw, c0 + c1), 12345.0).to(dev)
    prog = E.Program.of([L.make(L.OP_CONCAT, p0=a, p1=b, dst=out, n=n, hw=hw, c0=c0, c1=c1)], owner=(a, b, out))
    assert prog.n == 1 and int(prog.ops[0].kind) == L.OP_CONCAT == 35
    rec = L.args_of(prog.ops[0])                         # the record as the library will read it: the head of the union
    assert isinstance(rec, L.ConcatArgs) and (rec.p0, rec.p1, rec.dst) == (a.data_ptr(), b.data_ptr(), out.data_ptr())
    assert (rec.n, rec.hw, rec.c0, rec.c1) == shape
    assert [addr for _, addr in L.op_pointers(prog.ops[0])] == [a.data_ptr(), b.data_ptr(), out.data_ptr()]
    prog.run()
    _sync(dev)
    assert torch.equal(out.cpu(), torch.cat([a.cpu(), b.cpu()], -1))


def check_concat_adjoint(dev, shape):
    """the backward program of one concatenation (backward.TrainEngine._bwd_concat: two gradient slices, no kernel of its own)
    against slicing the gradient of dst: written, and accumulated onto what the sources' gradients held"""
    from score_sde_pytorch_amd import engine as E, backward as B, _lib as L
    n, hw, c0, c1 = shape
    _, _, dy = _concat_case(shape)
    base = torch.randn(n, hw, c1, generator=torch.Generator().manual_seed(5))
    eng = B.TrainEngine.__new__(B.TrainEngine)
    eng.b, eng._G, eng._nograd = E.ProgramBuilder(torch.device(dev)), {}, set()
    p0, p1, dst = eng.b.buf(n, hw, c0, name="p0"), eng.b.buf(n, hw, c1, name="p1"), eng.b.buf(n, hw, c0 + c1, name="dst")
    g = {id(t): eng.b.buf(*t.shape, name="g_" + t.name, persistent=True) for t in (p0, p1, dst)}
    eng._G = {id(p0): [g[id(p0)], False], id(p1): [g[id(p1)], True], id(dst): [g[id(dst)], True]}     # p1's gradient: accumulated
    eng._bwd_concat(dict(p0=p0, p1=p1, dst=dst, n=n, hw=hw, c0=c0, c1=c1))
    assert [k for k, _, _, _ in eng.b.specs] == [L.OP_PROLOGUE_BWD, L.OP_PROLOGUE_BWD]
    assert [(f["dp_ld"], f["dp_off"], f["src"]["c0"]) for _, f, _, _ in eng.b.specs] == [(c0 + c1, 0, c0), (c0 + c1, c0, c1)]
    prog = eng.b.finalize()
    g[id(dst)].tensor[: dy.numel()].copy_(dy.reshape(-1))
    g[id(p1)].tensor[: base.numel()].copy_(base.reshape(-1))
    prog.run()
    _sync(dev)
    g0 = g[id(p0)].tensor[: n * hw * c0].cpu().view(n, hw, c0)
    g1 = g[id(p1)].tensor[: n * hw * c1].cpu().view(n, hw, c1)
    assert torch.equal(g0, dy[..., :c0])
    assert torch.equal(g1, base + dy[..., c0:])
    # an eng without a gradient of dst emits nothing
    eng._G.pop(id(dst))
    before = len(eng.b.specs)
    eng._bwd_concat(dict(p0=p0, p1=p1, dst=dst, n=n, hw=hw, c0=c0, c1=c1))
    assert len(eng.b.specs) == before


def check_concat_refusals(dev):
    """c0 = 6, c1 = 0 and hw = 0: SSDE_EINVAL with a message, decided on the host -- dst keeps its sentinel"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    lib = L.load()
    a, b = torch.zeros(2, 4, 8).to(dev), torch.zeros(2, 4, 8).to(dev)
    for bad in (dict(c0=6), dict(c1=0), dict(hw=0)):
        out = torch.full((2, 4, 16), 12345.0).to(dev)
        args = L.ConcatArgs()
        args.p0, args.p1, args.dst = ops._p(a), ops._p(b), ops._p(out)
        args.n, args.hw, args.c0, args.c1 = 2, 4, 8, 8
        for k, v in bad.items():
            setattr(args, k, v)
        rc = lib.ssde_concat(C.byref(args), ops._stream())
        msg = lib.ssde_last_error().decode()
        assert rc == SSDE_EINVAL, (bad, rc)
        assert msg.startswith("concat:") and len(msg) > len("concat: "), (bad, msg)
        _sync(dev)
        assert bool((out == 12345.0).all()), bad
    msg = pytest_raises(L.SsdeError, lambda: ops.concat(torch.zeros(1, 2, 6).to(dev), torch.zeros(1, 2, 4).to(dev)))
    assert "ssde_concat" in msg and "multiples of 4" in msg, msg
    # the same refusal from inside a program names the op
    from score_sde_pytorch_amd import engine as E
    out = torch.full((2, 4, 16), 12345.0).to(dev)
    prog = E.Program.of([L.make(L.OP_CONCAT, p0=a, p1=b, dst=out, n=2, hw=4, c0=6, c1=8)], owner=(a, b, out))
    msg = pytest_raises(L.SsdeError, prog.run)
    assert "op 0 (kind %d)" % L.OP_CONCAT in msg and "concat:" in msg, msg


def check_abi_unchanged():
    """the additions are additive: ABI number and op size as before (the new record fits the union)"""
    from score_sde_pytorch_amd import _lib as L
    lib = L.load()
    assert lib.ssde_abi_version() == L.ABI_VERSION == 13
    assert lib.ssde_sizeof_op() == C.sizeof(L.Op)
    assert C.sizeof(L.ConcatArgs) < max(C.sizeof(a) for k, a in L.ARGS.items() if k != L.OP_CONCAT)
    assert L.OP_CONCAT == 35 == max(L.ARGS)


# ---- 2. the constructor -------------------------------------------------------------------------------------------------
def _build(cfg):
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    return mutils.get_model("ncsnpp")(cfg)


def check_state_dict_names(case):
    """names and shapes equal the reference's (tests/golden/ncsnpp_arch_state_dict_names.json), and a state dict round trip"""
    with open(os.path.join(_util.GOLDEN, "ncsnpp_arch_state_dict_names.json")) as f:
        names = json.load(f)
    model = _build(config(case))
    mine = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert mine == names[case], [(a, b) for a, b in zip(mine, names[case]) if a != b][:5]
    sd = _util.load_seeded(model, seed=1)
    other = _build(config(case))
    res = other.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(other.state_dict()[k], v) for k, v in sd.items())


def check_constructor_refusals():
    cfg = config("ddpmblk_fir")
    cfg.model.resblock_type = "nope"
    assert pytest_raises(ValueError, lambda: _build(cfg)) == "resblock type nope unrecognized."
    cfg = _util.small_config("ncsnpp")                       # fir = True
    cfg.model.progressive = "residual"
    assert "upsample_conv_2d" in pytest_raises(NotImplementedError, lambda: _build(cfg))
    for case in UNRUNNABLE:                                  # no reference forward exists for these (see UNRUNNABLE)
        assert "layerspp.py:117" in pytest_raises(NotImplementedError, lambda: _build(config(case))), case
    cfg = _util.small_config("ncsnpp")
    cfg.model.resblock_type, cfg.model.resamp_with_conv = "ddpm", True
    assert "Upsample(with_conv=True, fir=True)" in pytest_raises(NotImplementedError, lambda: _build(cfg))
    model = _build(config("cat"))
    msg = pytest_raises(RuntimeError, lambda: model(torch.zeros(1, 3, 16, 16), torch.ones(1)))
    assert "no CPU fallback" in msg


def check_lowering_shapes():
    """dry lowering: the ops the new forms are made of"""
    from score_sde_pytorch_amd import engine as E, backward as B, _lib as L

    def specs(case, train=False):
        model, _ = model_of(config(case), "cpu")
        eng = (B.TrainEngine(model, 2, 16, 16, "cpu", input_grad=True) if train else E.UNetEngine(model, 2, 16, 16, "cpu"))
        return eng.b.specs
    cat = specs("cat")
    joins = [f for k, f, _, _ in cat if k == L.OP_CONCAT]
    assert [(f["hw"], f["c0"], f["c1"]) for f in joins] == [(64, 32, 32), (16, 64, 64)]       # two concatenations of different widths
    assert sum(k == L.OP_CONCAT for k, _, _, _ in specs("cat_ddpmblk_fir_elu")) == 1
    # the adjoint of a concatenation is two slices: no op kind of its own in the backward half
    trn = specs("cat", train=True)
    assert sum(k == L.OP_CONCAT for k, _, _, _ in trn) == 2
    # Downsample(with_conv, no FIR) with the pyramid's sum in its epilogue: ONE end-padded stride-2 launch
    down = [f for k, f, _, _ in specs("resid_in") if k == L.OP_CONV and f["stride"] == 2]
    assert len(down) == 1 and down[0]["pad_end"] == 1 and down[0]["pad"] == 0 and down[0]["resid"] is not None
    assert abs(down[0]["out_scale"] - E.INV_SQRT2) < 1e-7
    # DDPM blocks with FIR resampling and no convolution: downsample_2d at nf channels and upsample_2d at 2 nf, beside the FIR of
    # the residual input pyramid (4 channels, no rate change: its stride is the convolution's)
    fir = [f for k, f, _, _ in specs("ddpmblk_fir") if k == L.OP_UPFIRDN]
    assert sorted((f["up"], f["down"], f["kh"], f["c"]) for f in fir) == [(1, 1, 4, 4), (1, 2, 4, 32), (2, 1, 4, 64)]


# ---- 3. whole forward ---------------------------------------------------------------------------------------------------
def check_forward(dev, case, tol=TOL_FWD):
    """one forward against the REFERENCE's (tests/golden/unet_arch_<case>.npz)"""
    from score_sde_pytorch_amd import engine as E
    gold = np.load(os.path.join(_util.GOLDEN, "unet_arch_%s.npz" % case))
    model, _ = model_of(config(case), dev)
    x, cond, y_ref = (torch.from_numpy(gold[k]) for k in ("x", "cond", "y"))
    xi, ci = forward_inputs(case)
    assert torch.equal(x, xi) and torch.equal(cond, ci)
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    y = eng.forward(x.to(dev), cond.to(dev))
    err = rel_err(y, y_ref)
    print("%s (SSDE_WINOGRAD=%s) forward vs reference: rel err %.3g" % (case, os.environ.get("SSDE_WINOGRAD", "1"), err))
    assert err < tol, (case, err)
    assert torch.equal(y, eng.forward(x.to(dev), cond.to(dev)))


# ---- 4. gradients -------------------------------------------------------------------------------------------------------
def _train_state(dev, case):
    from score_sde_pytorch_amd.models import ema as ema_mod
    from score_sde_pytorch_amd import losses, sde_lib
    tc = train_case(case)
    cfg = train_config(case)
    model, init = model_of(cfg, dev)
    sde = _util.train_case_sde(sde_lib, tc, cfg)
    opt = losses.get_optimizer(cfg, model.parameters())
    ema = ema_mod.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    kw = dict(optimize_fn=losses.optimization_manager(cfg), reduce_mean=False, continuous=True, likelihood_weighting=False)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    return cfg, state, losses.get_step_fn(sde, train=True, **kw)


def check_loss_and_gradients(dev, case):
    """the continuous loss of the first batch through losses.FusedTrainStep: the loss, the norm of EVERY parameter gradient and
    the probe tensors in full against the reference's loss.backward() (tests/golden/train_arch_<case>.npz); twice, same bits"""
    gold = np.load(os.path.join(_util.GOLDEN, "train_arch_%s.npz" % case))
    cfg, state, train_step = _train_state(dev, case)
    batch, u, labels, z = _util.train_case_inputs("arch_" + case, cfg.model.num_scales, size=cfg.data.image_size)[0]
    fs = train_step.fused_for(state, batch.to(dev))
    assert fs is not None
    sde_eps = 1e-5                                                # losses.py:84: t = u (T - eps) + eps, T = 1
    t = u * (1 - sde_eps) + sde_eps
    loss = float(fs.loss_and_grads(batch.to(dev), t=t.to(dev), z=z.to(dev), seed=0))
    ref_loss = float(gold[case + "/grad_loss"])
    print("%s: loss %.8g, reference %.8g" % (case, loss, ref_loss))
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    params = [(n, p) for n, p in state["model"].named_parameters() if p.requires_grad]
    gnorms = gold[case + "/gnorms"]
    assert len(params) == gnorms.shape[0]
    worst = 0.0
    for (n, p), ref in zip(params, gnorms):
        got = float(fs.flat.grad_view(p).double().norm())
        if ref < 1e-4:                   # analytically-zero gradients (the key bias of attention): compared absolutely
            assert got < 1e-4, (n, got)
            continue
        worst = max(worst, abs(got - ref) / ref)
        assert abs(got - ref) <= TOL_GRAD * ref, (n, got, ref)
    probes = {k.split("/", 2)[2]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(case + "/g/")}
    assert len(probes) >= 10
    worst_p = T.compare_param_grads(types.SimpleNamespace(named_parameters=lambda: [(n, p) for n, p in params if n in probes]),
                                    fs.flat, probes, tol=TOL_GRAD)
    print("%s training gradients: worst norm error %.3g over %d tensors, worst probe %.3g over %d"
          % (case, worst, len(params), worst_p, len(probes)))
    g1 = fs.flat.grad.clone()
    loss2 = float(fs.loss_and_grads(batch.to(dev), t=t.to(dev), z=z.to(dev), seed=0))
    assert loss2 == loss and torch.equal(g1, fs.flat.grad)


def check_input_gradient(dev, case):
    """d sum(y * cot) / d x through the autograd bridge with every parameter frozen -- a backward program without weight
    gradients, the path likelihood.py takes -- against the reference's autograd.grad"""
    from score_sde_pytorch_amd import autograd as AG, _lib as L
    gold = np.load(os.path.join(_util.GOLDEN, "train_arch_%s.npz" % case))
    model, _ = model_of(config(case), dev)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    x, cond = forward_inputs(case)
    cot, dx_ref = torch.from_numpy(gold[case + "/cot"]), torch.from_numpy(gold[case + "/dx"])
    assert torch.equal(cot, cotangent(case))
    xd = x.to(dev).requires_grad_()
    # (the model itself refuses a CPU tensor; under the emulator the bridge is entered directly)
    y = model(xd, cond.to(dev)) if dev != "cpu" else AG.unet_apply(model, xd, cond.to(dev))
    dx, = torch.autograd.grad((y * cot.to(dev)).sum(), xd)
    eng = next(e for k, e in model._engines.items() if k[0] == "train")
    kinds = [int(eng.program.ops[i].kind) for i in range(eng.program.n)]
    assert not eng.param_grads and L.OP_WGRAD not in kinds
    err = rel_err(dx, dx_ref)
    print("%s: d sum(y cot) / dx vs reference: rel err %.3g" % (case, err))
    assert err < TOL_GRAD, (case, err)


def run_train_steps(dev, case, steps=2):
    """`steps` steps of losses.get_step_fn with injected draws; returns (losses, parameters)"""
    cfg, state, train_step = _train_state(dev, case)
    inputs = _util.train_case_inputs("arch_" + case, cfg.model.num_scales, size=cfg.data.image_size)
    out = []
    for step in range(steps):
        batch, u, labels, z = inputs[step]
        with _util.inject_rng(u, labels, z):
            out.append(float(train_step(state, batch.to(dev))))
    fs = train_step.fused_for(state, inputs[0][0].to(dev))
    assert fs.steps_done == steps, "the steps must have run as the fused step"
    assert all(np.isfinite(out))
    return out, [p.detach().clone() for p in state["model"].parameters()]


# ---- 5. the sampler -----------------------------------------------------------------------------------------------------
def check_sampler(dev, steps=3, B=4):
    """three iterations of the stock PC sampler (reverse diffusion + Langevin) on the 'cat' network with injected noise, op by
    op; on the GPU the same iterations as hipGraph replays give the same bits, and the sampler's own graph path is taken"""
    from score_sde_pytorch_amd import sampling, sde_lib
    cfg = config("cat")
    model, _ = model_of(cfg, dev)
    model.eval()
    R = cfg.data.image_size
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=steps)
    sampler = sampling.get_pc_sampler(sde, (B, 3, R, R), sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, lambda v: v,
                                      snr=0.16, n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-5, device=dev)
    x_T, noises = _util.pc_case_inputs(B, steps, 50.0, R, seed=29)
    if dev == "cpu":
        # (the sampler asks whether x is HIP memory; under the emulator the engine is driven directly)
        from score_sde_pytorch_amd import pc_engine
        plan = pc_engine.plan_fused(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, model, True,
                                    types.SimpleNamespace(is_cuda=True))
        eng = pc_engine.FusedPCSampler(model, sde, plan, (B, 3, R, R), snr=0.16, n_steps=1, probability_flow=False, eps=1e-5,
                                       device=torch.device(dev))
        x, x_mean = eng.run(x_T, noises=noises)
    else:
        x_mean, nfe = sampler(model, x_init=x_T, noises=noises)
        assert nfe == 2 * steps and sampler.last_path == "fused-eager"
        eng = sampler.engine
    from score_sde_pytorch_amd import _lib as L
    prog = eng.step_program(with_rng=False)
    assert sum(int(prog.ops[i].kind) == L.OP_CONCAT for i in range(prog.n)) == 4          # two per U-Net evaluation
    assert bool(torch.isfinite(x_mean).all())
    again = eng.run(x_T.to(dev), noises=noises)[1]
    assert torch.equal(again, x_mean)
    if dev == "cpu":
        return
    # the same program as graph replays, fed the same noise
    eng.reset(x_T.to(dev))
    nz = noises.to(dev)
    side = torch.cuda.Stream()
    for i in range(steps):
        eng.z_c.copy_(nz[i, 0].reshape(-1))
        eng.z_p.copy_(nz[i, 1].reshape(-1))
        prog.replay_from_current(side)
    torch.cuda.synchronize()
    assert torch.equal(eng.x_mean.view(x_mean.shape), x_mean)
    # and the sampler as users run it: its own noise, the whole loop as one graph replayed per step
    a, _ = sampler(model, x_init=x_T, seed=11, use_graph=True)
    assert sampler.last_path == "fused-graph"
    b, _ = sampler(model, x_init=x_T, seed=11, use_graph=False)
    assert sampler.last_path == "fused-eager"
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- 6. plans -----------------------------------------------------------------------------------------------------------
def check_unet_plan_round_trip(dev, case="cat"):
    """a U-Net plan of the 'cat' network through plan_export and LoadedPlan: the engine's bits"""
    from score_sde_pytorch_amd import engine as E, plan_export as P, _lib as L
    model, _ = model_of(config(case), dev)
    x, cond = forward_inputs(case)
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    assert any(int(eng.program.ops[i].kind) == L.OP_CONCAT for i in range(eng.program.n))
    y = eng.forward(x.to(dev), cond.to(dev)).clone()
    blob = P.export_unet_plan(eng)
    hdr = P.PlanHeader.from_buffer_copy(blob[: C.sizeof(P.PlanHeader)])
    assert hdr.abi_version == L.ABI_VERSION == 13
    del eng
    plan = P.LoadedPlan(blob)
    try:
        y2 = plan.unet_forward(x.to(dev).contiguous(), cond.to(dev).contiguous())
    finally:
        plan.close()
    assert torch.equal(y.cpu(), y2.cpu())


def check_train_plan_round_trip(dev, case="cat", n_steps=2):
    """a training plan of the 'cat' network: whole steps through ssde_train_step against the Python-driven fused step (the
    pattern of _act_checks.check_train_plan_round_trip)"""
    from score_sde_pytorch_amd import plan_export, losses
    cfg, state, train_step = _train_state(dev, case)
    R, Bn = cfg.data.image_size, _util.TRAIN_BATCH
    opt, ema = state["optimizer"], state["ema"]
    cfg.optim.warmup = 0                                  # (the first step already moves the parameters)
    optimize_fn = losses.optimization_manager(cfg)
    fs = train_step.fused_for(state, torch.zeros(Bn, 3, R, R, device=dev))
    blob = plan_export.export_train_plan(fs, opt, ema)
    g = torch.Generator().manual_seed(21)
    steps = [(torch.rand(Bn, 3, R, R, generator=g), torch.rand(Bn, generator=g) * 0.9 + 0.05, torch.randn(Bn, 3, R, R, generator=g))
             for _ in range(n_steps)]
    ref_loss, hypers, coefs = [], [], []
    for i, (b, t, z) in enumerate(steps):
        ref_loss.append(float(fs.loss_and_grads(b.to(dev), t=t.to(dev), z=z.to(dev), seed=40 + i)))
        coefs.append((fs.a.clone(), fs.s.clone(), fs.eng.cond.tensor[:Bn].clone()))
        fs.optimizer_step(opt, ema, state["step"], optimize_fn.ssde_hyper)
        state["step"] += 1
        hypers.append(fs.hyper.detach().cpu()[:9].tolist())
    ref_params = fs.flat.data.clone()
    plan = plan_export.LoadedPlan(blob)
    try:
        assert plan.header.kind == plan_export.PLAN_TRAIN and plan.header.n_flat == fs.flat.numel
        for i, (b, t, z) in enumerate(steps):
            a_, s_, lab = coefs[i]
            loss = plan.train_step(b.to(dev), z.to(dev), a_, s_, lab, hypers[i], 40 + i)
            assert abs(float(loss) - ref_loss[i]) <= (0.0 if dev != "cpu" else 1e-6 * abs(ref_loss[i])), (i, float(loss), ref_loss[i])
        got = plan.read_io(plan_export.IO_PARAMS, ref_params)
    finally:
        plan.close()
    if dev != "cpu":
        assert torch.equal(got, ref_params), float((got - ref_params).abs().max())
    else:       # (the emulator's Python path re-packs Winograd weights with the torch packers: _train_checks.check_train_plan)
        assert rel_err(got, ref_params) < 1e-5
