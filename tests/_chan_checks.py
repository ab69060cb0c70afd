"""Checks of config.data.num_channels = C for any C >= 1: the image travels through a program padded to whole quads
(engine.image_cpad), the image heads of more than four channels run on conv_small.hip's 2- and 4-quad instantiations
(SSDE_CONVF_SMALL_COUT_WIDE), and everything around the network -- training, samplers, inpainting, plans, likelihood -- follows
the model's count.  Shared by the emulator suite (tests/test_chan_cpu.py) and the GPU suite (tests/test_chan_gpu.py); the cases
are in tests/_chan_cases.py, the reference's outputs come from tools/gen_golden_channels.py.

Tolerances are the project's: a whole forward 1e-4 and gradients 2e-4 (tests/_gn_width_checks.py), a single head launch 2e-5
relative (the direct kernel's tolerance, _train_checks.check_conv_small_cout), a sampler against its restatement 2e-4
(tests/test_emulated_sampler.py)."""
import ctypes as C
import functools
import json
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

import _util
import _gn_width_checks as K
import _train_checks as T
import _arch_checks as A
import _chan_cases as CC
from _util import rel_err
from _act_checks import pytest_raises

TOL_FWD, TOL_GRAD, TOL_HEAD, TOL_SAMPLER = K.TOL_FWD, K.TOL_GRAD, 2e-5, 2e-4

# ---- 1. head launches ---------------------------------------------------------------------------------------------------
HEAD_COUTS = (5, 8, 12, 13, 16)
# (n, h, w): partial tiles on both axes in one and in several tiles per axis, a map smaller than the tile, one whole-tile map
HEAD_MAPS = ((1, 6, 10), (1, 12, 20), (2, 4, 4), (1, 32, 32))
# (c0, c1): one chunk, a ragged second chunk, two full chunks, a pair source
HEAD_SOURCES = ((8, 0), (136, 0), (256, 0), (96, 64))
HEAD_SCALE, DROP_P, SEED_WORD, SALT = 0.7, 0.25, 0x1234ABCD, 0x9E3779B1 * 3 & 0xFFFFFFFF


def head_shapes(source):
    """every map with this source; the 32x32 map once (one chunk)"""
    return [(m, source) for m in HEAD_MAPS if m[1] != 32 or source == HEAD_SOURCES[0]]


@functools.lru_cache(maxsize=None)
def head_case(shape):
    """inputs of one (map, source) and the fp64 convolutions onto 16 channels, plain and behind the full prologue, computed
    once and shared by every c_out (which takes the leading rows of the weight; nothing writes to them)"""
    (n, h, w), (c0, c1) = shape
    cin = c0 + c1
    g = torch.Generator().manual_seed(7 + 1000 * cin + 10 * h + w)
    x = torch.randn(n, h, w, cin, generator=g) * 1.5 + 0.3
    wt = torch.randn(16, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    bias, gamma, beta = torch.randn(16, generator=g), torch.randn(cin, generator=g), torch.randn(cin, generator=g)
    resid, ca = torch.randn(n, h, w, 16, generator=g), torch.randn(n, 16, generator=g)
    G = 32 if cin % 32 == 0 and (cin // 32) % 4 == 0 else cin // 4
    thresh = min(int(round(DROP_P * 2.0 ** 32)), 2 ** 32 - 1)
    keep = torch.from_numpy(T.hash_keep(np.arange(n * h * w * cin, dtype=np.uint64), SEED_WORD ^ SALT, thresh, 1.0 / (1.0 - DROP_P)))
    keep = keep.reshape(n, h, w, cin).double()
    x64 = x.double().permute(0, 3, 1, 2)
    xn = F.silu(F.group_norm(x64, G, gamma.double(), beta.double(), 1e-6)) * keep.permute(0, 3, 1, 2)
    plain = F.conv2d(x64, wt.double(), None, padding=1).permute(0, 2, 3, 1)
    fused = F.conv2d(xn, wt.double(), None, padding=1).permute(0, 2, 3, 1)
    return dict(x=x, wt=wt, bias=bias, gamma=gamma, beta=beta, resid=resid, ca=ca, G=G, plain=plain, fused=fused)


def _head_args(dev, case, shape, cout, mode, flags, keep_alive):
    """ssde_conv_args of one head launch; mode: 'plain', or ('fused', resid_post)"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    from score_sde_pytorch_amd.engine import pack_conv_weight
    (n, h, w), (c0, c1) = shape
    x = case["x"]
    x0d = x[..., :c0].contiguous().to(dev)
    x1d = x[..., c0:].contiguous().to(dev) if c1 else None
    wp, bd = pack_conv_weight(case["wt"][:cout].to(dev)), case["bias"][:cout].contiguous().to(dev)
    dst = torch.full((n, h, w, cout), float("nan")).to(dev)
    a = L.ConvArgs()
    keep_alive += [x0d, x1d, wp, bd, dst]
    if mode == "plain":
        ops._fill_src(a.main, x0d, x1d, L.PRO_NONE, None)
        a.out_scale = 1.0
    else:
        mean, rstd = ops.groupnorm_stats(x0d, case["G"], 1e-6, x2=x1d)
        gam, bet = case["gamma"].to(dev), case["beta"].to(dev)
        seed = torch.tensor([SEED_WORD], dtype=torch.int32).to(dev)
        ops._fill_src(a.main, x0d, x1d, L.PRO_GN_SILU, (mean, rstd, gam, bet, case["G"]))
        ops._fill_drop(a.main, (DROP_P, seed, SALT))
        cad, rd = case["ca"][:, :cout].contiguous().to(dev), case["resid"][..., :cout].contiguous().to(dev)
        keep_alive += [mean, rstd, gam, bet, seed, cad, rd]
        a.chan_add, a.chan_add_ld, a.resid, a.resid_post, a.out_scale = cad.data_ptr(), cout, rd.data_ptr(), mode[1], HEAD_SCALE
    a.w_main, a.ksize, a.stride, a.pad, a.h_in, a.w_in = wp.data_ptr(), 3, 1, 1, h, w
    a.n, a.h_out, a.w_out, a.c_out, a.dst, a.tile = n, h, w, cout, dst.data_ptr(), L.TILE_AUTO
    a.bias, a.flags = bd.data_ptr(), L.conv_route_flags() | flags
    return a, dst


def _head_ref(case, cout, mode):
    b = case["bias"][:cout].double()
    if mode == "plain":
        return case["plain"][..., :cout] + b
    core = case["fused"][..., :cout] + b + case["ca"][:, None, None, :cout].double()
    r = case["resid"][..., :cout].double()
    return (core + r) * HEAD_SCALE if not mode[1] else core * HEAD_SCALE + r


def small_lds_bytes(cout):
    """conv_small.hip's allocation (its header: halo + one quad's weights + GroupNorm tables): the same for every quad count,
    the quads take turns in the weights area -- two workgroups per CU"""
    return (100 * 128 + 9 * 16 * 36 + 64 + 2 * 128) * 4


def check_head_launches(dev, cout, source):
    """c_out channels onto every shape of head_shapes(source), plain and fully fused (GroupNorm + SiLU prologue, dropout with a seed
    word, bias, per-image addend, residual before and after the scale, scale 0.7): with the flag (conv_small.hip, its plan says
    so) and without (the direct kernel), both against fp64 F.conv2d and against each other"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    lib = L.load()
    worst = 0.0
    for shape in head_shapes(source):
        case = head_case(shape)
        for mode in ("plain", ("fused", 0), ("fused", 1)):
            ref, outs, lds = _head_ref(case, cout, mode), [], []
            for flags in (L.CONVF_SMALL_COUT_WIDE, 0):
                keep = []
                a, dst = _head_args(dev, case, shape, cout, mode, flags, keep)
                lds.append(lib.ssde_conv_lds_bytes(C.byref(a)))
                assert lds[-1] > 0, lib.ssde_last_error()
                L.check(lib.ssde_conv2d(C.byref(a), ops._stream()))
                A._sync(dev)
                outs.append(dst.cpu())
            assert lds[0] == small_lds_bytes(cout) and lds[1] != lds[0], (shape, lds)        # which kernel each launch took
            errs = (rel_err(outs[0], ref), rel_err(outs[1], ref), rel_err(outs[0], outs[1]))
            worst = max(worst, *errs)
            assert all(e < TOL_HEAD for e in errs), (shape, cout, mode, errs)
    print("head launches %s -> %d: worst rel err %.3g (flagged vs fp64, direct vs fp64, flagged vs direct)" % (source, cout, worst))


def check_head_routing(dev):
    """c_out <= 4: the same bits with and without the flag; 17 with it and 5 without it: the direct kernel's plan (as today);
    16 with SSDE_CONVF_NO_SMALL_COUT on top: the direct kernel's; the ABI number and the op size are what they were"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    lib = L.load()
    shape = (HEAD_MAPS[0], HEAD_SOURCES[1])
    case = head_case(shape)

    def plan(cout, flags):
        keep = []
        a, _ = _head_args(dev, case, shape, min(cout, 16), "plain", flags, keep)
        a.c_out = cout                               # (plan only: nothing is launched)
        return lib.ssde_conv_lds_bytes(C.byref(a)), lib.ssde_conv_gn_slices(C.byref(a))
    for cout in (1, 3, 4):
        for mode in ("plain", ("fused", 1)):
            outs = []
            for flags in (0, L.CONVF_SMALL_COUT_WIDE):
                keep = []
                a, dst = _head_args(dev, case, shape, cout, mode, flags, keep)
                assert lib.ssde_conv_lds_bytes(C.byref(a)) == small_lds_bytes(cout) == 73216
                L.check(lib.ssde_conv2d(C.byref(a), ops._stream()))
                A._sync(dev)
                outs.append(dst.cpu())
            assert torch.equal(outs[0], outs[1]) and rel_err(outs[0], _head_ref(case, cout, mode)) < TOL_HEAD
    # a channel's bits do not depend on the quad count: the leading quad of an 8- and of a 16-channel launch (the 2- and the
    # 4-quad instantiation) against the 4-channel launch (one quad) of the same leading weight rows, bias, addend and residual
    for mode in ("plain", ("fused", 0)):
        outs = {}
        for cout in (4, 8, 16):
            keep = []
            a, dst = _head_args(dev, case, shape, cout, mode, L.CONVF_SMALL_COUT_WIDE, keep)
            assert lib.ssde_conv_lds_bytes(C.byref(a)) == small_lds_bytes(cout)
            L.check(lib.ssde_conv2d(C.byref(a), ops._stream()))
            A._sync(dev)
            outs[cout] = dst.cpu()
        assert torch.equal(outs[8][..., :4], outs[4]) and torch.equal(outs[16][..., :4], outs[4])
        assert torch.equal(outs[16][..., :8], outs[8])
    W = L.CONVF_SMALL_COUT_WIDE
    assert W == 16384
    direct5 = plan(5, L.CONVF_NO_SMALL_COUT)
    assert plan(5, 0) == direct5 and plan(5, W)[0] == small_lds_bytes(5) != direct5[0]
    assert plan(5, W | L.CONVF_NO_SMALL_COUT) == direct5
    assert plan(16, W)[0] == small_lds_bytes(16) and plan(16, W | L.CONVF_NO_SMALL_COUT) == plan(16, 0)
    assert plan(17, W) == plan(17, 0) == plan(17, L.CONVF_NO_SMALL_COUT) and plan(17, W)[0] > 0
    assert plan(32, W) == plan(32, 0)
    assert plan(8, W)[1] == 0                         # (the image heads are not normalised by anybody: no partials)
    assert lib.ssde_abi_version() == L.ABI_VERSION == 13
    assert lib.ssde_sizeof_op() == C.sizeof(L.Op)
    A.check_abi_unchanged()


# ---- 2. dry lowering ----------------------------------------------------------------------------------------------------
def _model(case_or_cfg, dev="cpu", fam=None):
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = CC.config(case_or_cfg) if isinstance(case_or_cfg, str) else case_or_cfg
    fam = fam or (CC.family(case_or_cfg) if isinstance(case_or_cfg, str) else "ncsnpp")
    torch.manual_seed(0)
    model = mutils.get_model(fam)(cfg)
    _util.load_seeded(model, seed=1)
    return model.to(dev)


def _op_summary(specs):
    """kinds and shapes of a spec list: every integer field of every spec, every source's channel counts"""
    out = []
    for kind, f, _, _ in specs:
        row = [kind]
        for k in sorted(f):
            v = f[k]
            if isinstance(v, bool) or isinstance(v, (int, float)):
                row.append((k, v))
            elif isinstance(v, dict) and "c0" in v:
                row.append((k, v["c0"], v["c1"], v["pro_mode"]))
            elif hasattr(v, "shape"):
                row.append((k, tuple(v.shape)))
        out.append(tuple(row))
    return out


def _lower(kind, c, literal4=False, over=None):
    from score_sde_pytorch_amd import engine as E
    cfg = _util.small_config(kind)
    for k, v in (over or {}).items():
        cfg.model[k] = v
    cfg.data.num_channels = c
    model = _model(cfg)
    if not literal4:
        return E.UNetEngine(model, 2, 16, 16, "cpu")
    real = E.image_cpad
    E.image_cpad = lambda channels: 4                 # the rule the lowering had: "three channels padded to four"
    try:
        return E.UNetEngine(model, 2, 16, 16, "cpu")
    finally:
        E.image_cpad = real


def check_lowering_small_counts(c):
    """C <= 4: the op list (kinds and shapes) equals the one built with the literal-4 rule, and no launch carries the new flag"""
    from score_sde_pytorch_amd import _lib as L
    for kind in ("ncsnpp", "ffhq"):
        eng, old = _lower(kind, c), _lower(kind, c, literal4=True)
        assert _op_summary(eng.b.specs) == _op_summary(old.b.specs)
        assert eng.program.n == old.program.n
        for i in range(eng.program.n):
            a, b = eng.program.ops[i], old.program.ops[i]
            assert int(a.kind) == int(b.kind)
            if int(a.kind) == L.OP_CONV:
                assert a.u.conv.flags == b.u.conv.flags and not a.u.conv.flags & L.CONVF_SMALL_COUT_WIDE
                assert (a.u.conv.c_out, a.u.conv.main.c0, a.u.conv.aux.c0) == (b.u.conv.c_out, b.u.conv.main.c0, b.u.conv.aux.c0)


def check_lowering_wide_counts(c):
    """C > 4: the input, pyramid, head and output ops carry cpad = (C + 3) // 4 * 4, and the head launches carry the flag
    wherever the lowering adopted it (engine.HEAD_WIDE_QUADS)"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    cpad = (c + 3) // 4 * 4
    assert E.image_cpad(c) == cpad
    want_flag = L.CONVF_SMALL_COUT_WIDE if cpad // 4 in E.HEAD_WIDE_QUADS and cpad <= 16 else 0
    assert E.head_flags(cpad) == want_flag
    # residual input pyramid with FIR, one head
    eng = _lower("ncsnpp", c)
    sp = eng.b.specs
    nhwc = [f for k, f, _, _ in sp if k == L.OP_TO_NHWC]
    nchw = [f for k, f, _, _ in sp if k == L.OP_TO_NCHW]
    assert len(nhwc) == 1 and (nhwc[0]["c"], nhwc[0]["c_pad"]) == (c, cpad)
    assert len(nchw) == 1 and (nchw[0]["c"], nchw[0]["c_src"]) == (c, cpad)
    convs = [f for k, f, _, _ in sp if k == L.OP_CONV]
    first = next(f for f in convs if f["ksize"] == 3)
    assert first["main"]["c0"] == cpad and first["c_out"] == 32
    fir = [f for k, f, _, _ in sp if k == L.OP_UPFIRDN and f["c"] == cpad]
    assert len(fir) == 1 and (fir[0]["up"], fir[0]["down"]) == (1, 1)                 # the FIR in front of the pyramid's stride-2 conv
    down = [f for f in convs if f["stride"] == 2 and f["main"]["c0"] == cpad]
    assert len(down) == 1 and down[0]["resid"] is not None
    heads = [f for f in convs if f["c_out"] == cpad and f["ksize"] == 3]
    assert len(heads) == 1 and heads[0]["dst"] is nchw[0]["src"]
    assert heads[0].get("flags", 0) & L.CONVF_SMALL_COUT_WIDE == want_flag
    assert all(not f.get("flags", 0) & L.CONVF_SMALL_COUT_WIDE for f in convs if f is not heads[0])
    lds = eng.validate_plans()
    ops = [eng.program.ops[i] for i in range(eng.program.n) if int(eng.program.ops[i].kind) == L.OP_CONV]
    head_lds = [b for o, b in zip(ops, lds) if o.u.conv.c_out == cpad and o.u.conv.ksize == 3]
    assert head_lds == [small_lds_bytes(cpad)] if want_flag else head_lds[0] != small_lds_bytes(cpad)
    # input skip + output skip: a head per level, the pyramid's FIR up and down at cpad channels, combine GEMMs with K = cpad
    eng = _lower("ffhq", c)
    sp = eng.b.specs
    convs = [f for k, f, _, _ in sp if k == L.OP_CONV]
    heads = [f for f in convs if f["c_out"] == cpad and f["ksize"] == 3]
    assert len(heads) == 2 and heads[0]["resid"] is None and heads[1]["resid"] is not None
    assert all(f.get("flags", 0) & L.CONVF_SMALL_COUT_WIDE == want_flag for f in heads)
    fir = sorted((f["up"], f["down"]) for k, f, _, _ in sp if k == L.OP_UPFIRDN and f["c"] == cpad)
    assert fir == [(1, 2), (2, 1)]
    comb = [f for f in convs if f["ksize"] == 0 and f["aux"]["c0"] == cpad]
    assert len(comb) == 1
    nchw = [f for k, f, _, _ in sp if k == L.OP_TO_NCHW]
    assert nchw[0]["src"] is heads[1]["dst"] and nchw[0]["c_src"] == cpad
    eng.validate_plans()
    # the `ddpm` family's head
    cfg = CC.config("ddpm_c6")
    cfg.data.num_channels = c
    eng = E.UNetEngine(_model(cfg, fam="ddpm"), 2, 16, 16, "cpu")
    heads = [f for k, f, _, _ in eng.b.specs if k == L.OP_CONV and f["c_out"] == cpad and f["ksize"] == 3]
    assert len(heads) == 1 and heads[0].get("flags", 0) & L.CONVF_SMALL_COUT_WIDE == want_flag
    # a training program: the backward half is derived from the recorded frames
    from score_sde_pytorch_amd import backward as B
    trn = B.TrainEngine(_model(CC.config("ncsnpp_c6") if c == 6 else _cfg_with(c)), 2, 16, 16, "cpu", input_grad=True)
    assert sum(1 for k, f, _, _ in trn.b.specs if k == L.OP_TO_NHWC and f["c_pad"] == cpad) == 2       # x, and the gradient of out
    assert sum(1 for k, f, _, _ in trn.b.specs if k == L.OP_TO_NCHW and f["c_src"] == cpad) == 2       # out, and the gradient of x


def _cfg_with(c):
    cfg = _util.small_config("ncsnpp")
    cfg.data.num_channels = c
    return cfg


def check_refusals():
    """a count nothing can lower is refused at construction, by name; the colorizer refuses every count but 3 before any launch"""
    from score_sde_pytorch_amd import engine as E, sde_lib, sampling, controllable_generation as cg
    model = _model(_cfg_with(6))
    model.channels = 0
    msg = pytest_raises(ValueError, lambda: E.UNetEngine(model, 2, 16, 16, "cpu"))
    assert "num_channels" in msg, msg
    model = _model(_cfg_with(6))
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=3)
    fn = cg.get_pc_colorizer(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, lambda v: v, snr=0.16, n_steps=1,
                             probability_flow=False, continuous=True, denoise=True, eps=1e-5)
    launches = []
    real = E.Program._launch
    E.Program._launch = lambda self, *a, **kw: launches.append(1) or real(self, *a, **kw)
    try:
        msg = pytest_raises(ValueError, lambda: fn(model, torch.zeros(2, 6, 16, 16)))
        assert "6 channels" in msg and "num_channels" in msg, msg
        msg = pytest_raises(ValueError, lambda: fn.engine(model, (2, 6, 16, 16), device="cpu"))
        assert "6 channels" in msg, msg
    finally:
        E.Program._launch = real
    assert not launches and not getattr(model, "_engines", None)


# ---- 3. whole forward ---------------------------------------------------------------------------------------------------
def check_forward(dev, case, tol=TOL_FWD, batch=None):
    """one forward against the REFERENCE's (tests/golden/unet_chan_<case>.npz); twice, the same bits.  batch: only the leading
    images of the fixture (the emulator suite runs one image of the nf = 128 `ddpm` network; nothing crosses the batch)"""
    from score_sde_pytorch_amd import engine as E
    gold = np.load(os.path.join(_util.GOLDEN, "unet_chan_%s.npz" % case))
    model = _model(case, dev)
    x, cond, y_ref = (torch.from_numpy(gold[k]) for k in ("x", "cond", "y"))
    xi, ci = CC.forward_inputs(case)
    assert torch.equal(x, xi) and torch.equal(cond, ci) and x.shape[1] == CC.channels(case)
    x, cond, y_ref = x[:batch].contiguous(), cond[:batch].contiguous(), y_ref[:batch]
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    y = eng.forward(x.to(dev), cond.to(dev))
    err = rel_err(y, y_ref)
    print("%s (SSDE_WINOGRAD=%s) forward vs reference: rel err %.3g" % (case, os.environ.get("SSDE_WINOGRAD", "1"), err))
    assert tuple(y.shape) == tuple(y_ref.shape) and err < tol, (case, err)
    assert torch.equal(y, eng.forward(x.to(dev), cond.to(dev)))


# ---- 4. gradients -------------------------------------------------------------------------------------------------------
def _train_state(dev, case):
    from score_sde_pytorch_amd.models import ema as ema_mod
    from score_sde_pytorch_amd import losses, sde_lib
    tc = CC.train_case(case)
    cfg = CC.train_config(case)
    model = _model(cfg, dev)
    sde = _util.train_case_sde(sde_lib, tc, cfg)
    opt = losses.get_optimizer(cfg, model.parameters())
    ema = ema_mod.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    kw = dict(optimize_fn=losses.optimization_manager(cfg), reduce_mean=False, continuous=True, likelihood_weighting=False)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    return cfg, state, losses.get_step_fn(sde, train=True, **kw)


def check_loss_and_gradients(dev, case):
    """the continuous loss of the first batch through losses.FusedTrainStep: the loss, the norm of EVERY parameter gradient and
    the probe tensors in full against the reference's loss.backward() (tests/golden/train_chan_<case>.npz); twice, same bits"""
    gold = np.load(os.path.join(_util.GOLDEN, "train_chan_%s.npz" % case))
    cfg, state, train_step = _train_state(dev, case)
    batch, u, labels, z = CC.train_inputs(case)[0]
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
    """d sum(y * cot) / d x through the autograd bridge with every parameter frozen against the reference's autograd.grad"""
    from score_sde_pytorch_amd import autograd as AG, _lib as L
    gold = np.load(os.path.join(_util.GOLDEN, "train_chan_%s.npz" % case))
    model = _model(case, dev)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    x, cond = CC.forward_inputs(case)
    cot, dx_ref = torch.from_numpy(gold[case + "/cot"]), torch.from_numpy(gold[case + "/dx"])
    assert torch.equal(cot, CC.cotangent(case))
    xd = x.to(dev).requires_grad_()
    # (the model itself refuses a CPU tensor; under the emulator the bridge is entered directly)
    y = model(xd, cond.to(dev)) if dev != "cpu" else AG.unet_apply(model, xd, cond.to(dev))
    dx, = torch.autograd.grad((y * cot.to(dev)).sum(), xd)
    eng = next(e for k, e in model._engines.items() if k[0] == "train")
    kinds = [int(eng.program.ops[i].kind) for i in range(eng.program.n)]
    assert not eng.param_grads and L.OP_WGRAD not in kinds
    err = rel_err(dx, dx_ref)
    print("%s: d sum(y cot) / dx vs reference: rel err %.3g" % (case, err))
    assert tuple(dx.shape) == tuple(dx_ref.shape) and err < TOL_GRAD, (case, err)


# ---- 5. state dict ------------------------------------------------------------------------------------------------------
def check_state_dict_names(case):
    """names and shapes equal the reference's (tests/golden/chan_state_dict_names.json), and a strict state-dict round trip"""
    from score_sde_pytorch_amd.models import utils as mutils
    with open(os.path.join(_util.GOLDEN, "chan_state_dict_names.json")) as f:
        names = json.load(f)
    model = _model(case)
    mine = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert mine == names[case], [(a, b) for a, b in zip(mine, names[case]) if a != b][:5]
    torch.manual_seed(0)
    other = mutils.get_model(CC.family(case))(CC.config(case))
    res = other.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(other.state_dict()[k], v) for k, v in model.state_dict().items())


# ---- 6. samplers --------------------------------------------------------------------------------------------------------
SAMPLER_C = 6


def _pc_args():
    return dict(snr=0.16, n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-5)


def check_sampler(dev, steps=3, B=2):
    """three iterations of the stock PC sampler (reverse diffusion + Langevin) at C = 6 with injected noise, op by op, against
    the restatement of the loop (oracle/sampler_oracle.py) around the package's own forward; on the GPU the same iterations as
    hipGraph replays give the same bits, and the sampler's own graph path is taken"""
    from score_sde_pytorch_amd import sampling, sde_lib, pc_engine, engine as E
    from oracle import sampler_oracle
    c = SAMPLER_C
    cfg = CC.config("ncsnpp_c6")
    model = _model(cfg, dev).eval()
    R = cfg.data.image_size
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=steps)
    kw = _pc_args()
    sampler = sampling.get_pc_sampler(sde, (B, c, R, R), sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, lambda v: v,
                                      device=dev, **kw)
    x_T, noises = CC.pc_inputs(B, steps, 50.0, R, c)
    if dev == "cpu":
        plan = pc_engine.plan_fused(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, model, True,
                                    types.SimpleNamespace(is_cuda=True))
        eng = pc_engine.FusedPCSampler(model, sde, plan, (B, c, R, R), snr=0.16, n_steps=1, probability_flow=False, eps=1e-5,
                                       device=torch.device(dev))
        x, x_mean = eng.run(x_T, noises=noises)
    else:
        x_mean, nfe = sampler(model, x_init=x_T, noises=noises)
        assert nfe == 2 * steps and sampler.last_path == "fused-eager"
        eng = sampler.engine
    assert tuple(x_mean.shape) == (B, c, R, R) and bool(torch.isfinite(x_mean).all())
    # the loop restated in torch, the score from a U-Net program of the same model
    unet = E.UNetEngine(model, B, R, R, torch.device(dev))
    real = sampler_oracle.score_fn
    sampler_oracle.score_fn = lambda cfg_, sd_, sde_, x_, t_, cont=True: unet.forward(
        x_.to(dev), sde_.marginal_prob(torch.zeros_like(x_), t_)[1].to(dev)).cpu()
    try:
        ref = sampler_oracle.pc_sample(cfg, None, "vesde", dict(sigma_min=0.01, sigma_max=50, N=steps), x_T, noises, snr=0.16, n_steps=1,
                                       eps=1e-5, denoise=True)["samples"]
    finally:
        sampler_oracle.score_fn = real
    err = rel_err(x_mean, ref)
    print("PC sampler at C = %d: against the restated loop rel err %.3g" % (c, err))
    assert err < TOL_SAMPLER, err
    again = eng.run(x_T.to(dev), noises=noises)[1]
    assert torch.equal(again, x_mean)
    if dev == "cpu":
        return
    prog = eng.step_program(with_rng=False)
    eng.reset(x_T.to(dev))
    nz = noises.to(dev)
    side = torch.cuda.Stream()
    for i in range(steps):
        eng.z_c.copy_(nz[i, 0].reshape(-1))
        eng.z_p.copy_(nz[i, 1].reshape(-1))
        prog.replay_from_current(side)
    torch.cuda.synchronize()
    assert torch.equal(eng.x_mean.view(x_mean.shape), x_mean)
    a, _ = sampler(model, x_init=x_T, seed=11, use_graph=True)
    assert sampler.last_path == "fused-graph"
    b, _ = sampler(model, x_init=x_T, seed=11, use_graph=False)
    assert sampler.last_path == "fused-eager"
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def check_inpainting(dev, steps=2, B=2):
    """get_pc_inpainter at C = 6 with a mask over some channels only (channels 0, 2 and 5 known everywhere, channel 1 on the left
    half): against the restated loop with the data-consistency step (oracle/sampler_oracle.inpaint) around the package's own forward"""
    from score_sde_pytorch_amd import sampling, sde_lib, pc_engine, engine as E, controllable_generation as cg
    from oracle import sampler_oracle
    c = SAMPLER_C
    cfg = CC.config("ncsnpp_c6")
    model = _model(cfg, dev).eval()
    R = cfg.data.image_size
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=steps)
    prior, noises = CC.pc_inputs(B, steps, 50.0, R, c, seed=31, streams=4)
    data = torch.rand(B, c, R, R, generator=torch.Generator().manual_seed(5))
    mask = torch.zeros(B, c, R, R)
    mask[:, [0, 2, 5]] = 1.0
    mask[:, 1, :, : R // 2] = 1.0
    fn = cg.get_pc_inpainter(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, lambda v: v, **_pc_args())
    real_plan = pc_engine.plan_fused
    if dev == "cpu":                                   # host tensors are only acceptable under the emulator
        pc_engine.plan_fused = lambda sde_, p, c_, m, cont, x, pf=False: real_plan(sde_, p, c_, m, cont, types.SimpleNamespace(is_cuda=True), pf)
    try:
        out = fn(model, data.to(dev), mask.to(dev), prior=prior.to(dev), noises=noises.to(dev))
    finally:
        pc_engine.plan_fused = real_plan
    assert fn.last_path == "fused-eager" and tuple(out.shape) == (B, c, R, R)
    unet = E.UNetEngine(model, B, R, R, torch.device(dev))
    real = sampler_oracle.score_fn
    sampler_oracle.score_fn = lambda cfg_, sd_, sde_, x_, t_, cont=True: unet.forward(
        x_.to(dev), sde_.marginal_prob(torch.zeros_like(x_), t_)[1].to(dev)).cpu()
    try:
        ref = sampler_oracle.inpaint(cfg, None, "vesde", dict(sigma_min=0.01, sigma_max=50, N=steps), data, mask, prior, noises,
                                     snr=0.16, n_steps=1, eps=1e-5, denoise=True)["samples"]
    finally:
        sampler_oracle.score_fn = real
    err = rel_err(out, ref)
    print("inpainting at C = %d: against the restated loop rel err %.3g" % (c, err))
    assert err < TOL_SAMPLER, err
    # the known part of the result is the data (VE: the mean of the perturbation kernel is the data itself)
    assert rel_err(out.cpu() * mask, data * mask) < 1e-6
    assert float(((out.cpu() - data) * (1 - mask)).abs().max()) > 1e-2


# ---- 7. plans -----------------------------------------------------------------------------------------------------------
def check_unet_plan_round_trip(dev, case="ncsnpp_c6"):
    """a U-Net plan through plan_export and LoadedPlan: the header's shape, the engine's bits"""
    from score_sde_pytorch_amd import engine as E, plan_export as P, _lib as L
    model = _model(case, dev)
    x, cond = CC.forward_inputs(case)
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    y = eng.forward(x.to(dev), cond.to(dev)).clone()
    blob = P.export_unet_plan(eng)
    hdr = P.PlanHeader.from_buffer_copy(blob[: C.sizeof(P.PlanHeader)])
    assert hdr.abi_version == L.ABI_VERSION == 13
    assert (hdr.batch, hdr.channels, hdr.height, hdr.width) == tuple(x.shape)
    del eng
    plan = P.LoadedPlan(blob)
    try:
        y2 = plan.unet_forward(x.to(dev).contiguous(), cond.to(dev).contiguous())
    finally:
        plan.close()
    assert tuple(y2.shape) == tuple(x.shape) and torch.equal(y.cpu(), y2.cpu())


def check_train_plan_round_trip(dev, case="ncsnpp_c6", n_steps=2):
    """a training plan at C = 6: whole steps through ssde_train_step against the Python-driven fused step (the pattern of
    _arch_checks.check_train_plan_round_trip)"""
    from score_sde_pytorch_amd import plan_export, losses
    cfg, state, train_step = _train_state(dev, case)
    c, R, Bn = CC.channels(case), cfg.data.image_size, CC.BATCH
    opt, ema = state["optimizer"], state["ema"]
    cfg.optim.warmup = 0                                  # (the first step already moves the parameters)
    optimize_fn = losses.optimization_manager(cfg)
    fs = train_step.fused_for(state, torch.zeros(Bn, c, R, R, device=dev))
    blob = plan_export.export_train_plan(fs, opt, ema)
    g = torch.Generator().manual_seed(21)
    steps = [(torch.rand(Bn, c, R, R, generator=g), torch.rand(Bn, generator=g) * 0.9 + 0.05, torch.randn(Bn, c, R, R, generator=g))
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
        assert (plan.header.batch, plan.header.channels, plan.header.height, plan.header.width) == (Bn, c, R, R)
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


def check_sampler_plan_round_trip(dev, steps=2, B=2):
    """a sampler plan with the inpainting projection at C = 6 (the device's own noise, seed word 5): the iterations through
    LoadedPlan give the bits of the Python-driven engine (the pattern of tests/_plan_control_checks.py, check 2)"""
    from score_sde_pytorch_amd import sampling, sde_lib, hipops, plan_export, controllable_generation as cg
    c = SAMPLER_C
    cfg = CC.config("ncsnpp_c6")
    model = _model(cfg, dev).eval()
    R = cfg.data.image_size
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=steps)
    fn = cg.get_pc_inpainter(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, lambda v: v, **_pc_args())
    eng = fn.engine(model, (B, c, R, R), device="cpu" if dev == "cpu" else None)
    assert eng is not None
    prior, _ = CC.pc_inputs(B, steps, 50.0, R, c, seed=31, streams=4)
    data = torch.rand(B, c, R, R, generator=torch.Generator().manual_seed(5)).to(dev).contiguous()
    mask = torch.zeros(B, c, R, R)
    mask[:, [0, 2, 5]] = 1.0
    mask[:, 1, :, : R // 2] = 1.0
    mask, prior = mask.to(dev).contiguous(), prior.to(dev).contiguous()
    known, m, x0 = hipops.project_prepare(data, mask, prior, None, None)
    eng.set_projection_inputs(known, m)
    x_py, xm_py = eng.run(x0, seed=5, use_graph=False)
    x_py, xm_py = x_py.cpu().clone(), xm_py.cpu().clone()
    blob = plan_export.export_pc_plan(eng)
    plan = plan_export.LoadedPlan(blob)
    try:
        h = plan.header
        assert (h.batch, h.channels, h.height, h.width) == (B, c, R, R)
        side = stream = None
        if dev != "cpu":
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            stream = side.cuda_stream
        plan.pc_set_known(data, mask, stream=stream)
        plan.pc_reset_known(prior, 5, stream=stream)
        plan.pc_run(steps, use_graph=False, stream=stream)
        x, xm = plan.pc_state(data, stream=stream)
        if side is not None:
            side.synchronize()
    finally:
        plan.close()
    assert bool(torch.isfinite(x).all()) and torch.equal(x.cpu(), x_py) and torch.equal(xm.cpu(), xm_py)
    keep = mask.cpu() == 1
    assert torch.equal(xm.cpu()[keep], data.cpu()[keep])        # VE: on mask == 1 the last projection writes the data


def _ode_model(dev, c, size=16):
    from score_sde_pytorch_amd import sde_lib
    cfg = _util.small_config("ddpmpp", image_size=size, attn=(size // 2,))
    cfg.data.num_channels = c
    model = _model(cfg, dev).eval()
    return cfg, model, sde_lib.subVPSDE(**_util.ODE_CASE["sde_kwargs"])


def check_ode_plan_round_trip(dev, c=6):
    """an ODE plan (the probability-flow drift) at C = 6: one evaluation of the right-hand side through LoadedPlan gives the
    bits of ode.FusedDrift, and a short solve through the C driver agrees with ode.solve_rk45 (tests/_plan_ode_checks.py's bounds)"""
    import _plan_ode_checks as P
    from score_sde_pytorch_amd import ode, plan_export
    cfg, model, sde = _ode_model(dev, c)
    B, R = 2, cfg.data.image_size
    z = torch.randn(B, c, R, R, generator=torch.Generator().manual_seed(77)).to(dev)
    rhs = ode.FusedDrift(model, sde, z.shape, torch.device(dev))
    blob = plan_export.export_ode_plan(rhs)
    plan = plan_export.LoadedPlan(blob)
    try:
        h = plan.header
        assert (h.batch, h.channels, h.height, h.width) == (B, c, R, R)
        # one evaluation of the right-hand side: the plan gives the bits of the engine's program (ode.FusedDrift)
        sc = ode.scalars_fn(rhs)
        ref = torch.empty(z.numel(), dtype=torch.float64, device=z.device)
        rhs.x32.copy_(z.reshape(-1))
        rhs(0.5, None, out=ref)
        A._sync(dev)
        plan.ode_reset(z, None)
        got = plan.ode_eval(0.5, sc, z)
        A._sync(dev)
        assert got.shape == (B * c * R * R,) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
        assert torch.equal(got, ref), float((got - ref).abs().max())
        t0, t1, tol = 1.0, 0.99, 1e-3
        y0 = z.reshape(-1).to(torch.float64)
        if dev != "cpu":
            y_py, nfev_py = ode.integrate_ode(rhs, (t0, t1), y0, tol, tol, "RK45")
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            stream = side.cuda_stream
        else:
            stages = ode._HipStages(y0.numel(), y0, x32=rhs.x32, n32=rhs.n32)
            y_py, nfev_py = ode.solve_rk45(rhs, (t0, t1), y0, rtol=tol, atol=tol, stages=stages)
            stream = None
        plan.ode_reset(z, None, stream=stream)
        nfev = plan.ode_solve(t0, t1, tol, tol, sc, use_graph=False, max_nfev=0, stream=stream)
        x, dl = plan.ode_state(z, stream=stream)
        if dev != "cpu":
            side.synchronize()
    finally:
        plan.close()
    assert dl is None and tuple(x.shape) == (B, c, R, R)
    P.assert_drivers_agree("sample", x, dl, nfev, y_py, nfev_py)


# ---- 8. likelihood ------------------------------------------------------------------------------------------------------
def check_likelihood(dev, c=2):
    """one likelihood.get_likelihood_fn evaluation at C = 2 (8-px images and a short span, t = 0.999 .. 1 at rtol = atol = 0.5: one
    step, 8 evaluations -- the emulator runs one in about a second) against the same
    composition through the autograd bridge -- scipy's RK45 around drift and Hutchinson divergence from torch.autograd.grad of
    the model's score -- and the bits/dim normaliser over C * H * W"""
    from scipy import integrate
    from score_sde_pytorch_amd import likelihood, autograd as AG
    cfg, model, sde = _ode_model(dev, c, size=8)
    for p in model.parameters():
        p.requires_grad_(False)
    B, R = 2, cfg.data.image_size
    g = torch.Generator().manual_seed(78)
    data = (torch.rand(B, c, R, R, generator=g) * 2 - 1)
    eps = torch.randint(0, 2, data.shape, generator=g).float() * 2 - 1.
    tol, t_eps = 0.5, 0.999
    lik = likelihood.get_likelihood_fn(sde, _util.ode_inverse_scaler, rtol=tol, atol=tol, eps=t_eps)
    real = torch.randint_like
    torch.randint_like = lambda t, **kw: ((eps.to(t.device) + 1) / 2).to(t.dtype)          # likelihood.py: randint_like(...) * 2 - 1
    from score_sde_pytorch_amd import ode
    real_applies = ode.FusedLikelihoodRhs.applies
    if dev == "cpu":                                   # host tensors are only acceptable under the emulator
        ode.FusedLikelihoodRhs.applies = staticmethod(lambda m, s, x: real_applies(m, s, types.SimpleNamespace(is_cuda=True)))
    try:
        bpd, zfin, nfe = lik(model, data.to(dev))
    finally:
        torch.randint_like = real
        ode.FusedLikelihoodRhs.applies = staticmethod(real_applies)
    assert lik.last_path == "fused"
    # the same composition through the autograd bridge
    shape = data.shape

    def score(x, t):
        std = sde.marginal_prob(torch.zeros_like(x), t)[1]
        y = model(x, t * 999) if dev != "cpu" else AG.unet_apply(model, x, t * 999)
        return -y / std[:, None, None, None]

    def rhs(t, y):
        x = torch.from_numpy(y[: data.numel()].reshape(shape)).float().to(dev)
        vt = torch.ones(B, device=dev) * t
        with torch.enable_grad():
            xg = x.clone().requires_grad_()
            drift, diff = sde.sde(xg, vt)
            f = drift - 0.5 * diff[:, None, None, None] ** 2 * score(xg, vt)
            gr, = torch.autograd.grad((f * eps.to(dev)).sum(), xg)
        div = (gr * eps.to(dev)).reshape(B, -1).sum(1)
        return np.concatenate([f.detach().cpu().numpy().reshape(-1), div.cpu().numpy().reshape(-1)]).astype(np.float64)
    y0 = np.concatenate([data.numpy().reshape(-1), np.zeros(B)]).astype(np.float64)
    sol = integrate.solve_ivp(rhs, (t_eps, sde.T), y0, rtol=tol, atol=tol, method="RK45")
    zp = torch.from_numpy(sol.y[: data.numel(), -1].reshape(shape)).float()
    dlp = torch.from_numpy(sol.y[data.numel():, -1]).float()
    N = c * R * R                                             # the normaliser: C * H * W
    bpd_ref = -(sde.prior_logp(zp) + dlp) / np.log(2) / N + 7.0
    off = -(sde.prior_logp(zp) + dlp) / np.log(2) / (3 * R * R) + 7.0
    err = rel_err(bpd, bpd_ref)
    print("likelihood at C = %d: bits/dim %s, through the bridge %s, rel err %.3g, nfe %d / %d" % (c, bpd.tolist(), bpd_ref.tolist(), err, nfe, sol.nfev))
    assert err < TOL_GRAD and rel_err(zfin, zp) < TOL_GRAD, err
    assert rel_err(bpd, off) > 100 * TOL_GRAD                 # (a normaliser over 3 * H * W would show)

