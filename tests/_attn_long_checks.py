"""Checks of attention over more than 256 tokens (attn_stream_kernel and the three streaming backward kernels of
attention.hip, ssde_attention_route, SSDE_ATTNF_STREAM and their lowering), shared by the emulator suite
(tests/test_attn_long_cpu.py) and the GPU suite (tests/test_attn_long_gpu.py).  Tolerances are the project's, max-abs error
over max-abs value: a kernel against fp64 2e-5 (TOL_GEMM forward, TOL_OP backward), a whole forward against the reference
golden 1e-4, network gradients against oracle autograd 2e-4."""
import ctypes as C
import os

import numpy as np
import torch

import _util
import _attn_long_util as A
import _train_checks as T
from _util import rel_err

TOL_GEMM, TOL_OP, TOL_FWD, TOL_GRAD = 2e-5, 2e-5, 1e-4, 2e-4

# (n, L, C).  272: a second key block of 16 valid keys, L % 32 != 0, a last query block of 16 rows; 320 x 96: C % 64 != 0;
# 576: three key blocks, nine row blocks; 1024 x 256: the 32 x 32 map
KERNEL_CASES = [(2, 272, 32), (1, 320, 96), (2, 576, 64), (1, 1024, 256)]
KERNEL_CASES_GPU_ONLY = [(1, 4096, 64), (1, 320, 512)]
FORCED_CASES = [(2, 64, 32), (2, 256, 64)]

_REF = {}


def _inputs(n, l, c):
    """the inputs of test_attention (queries sharpened x2, one row x6: row 3, or the last one where l < 4) and an output gradient"""
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(n, l, 3 * c, generator=g)
    qkv[:, :, :c] *= 2.0
    qkv[0, min(3, l - 1), :c] *= 6.0
    d_o = torch.randn(n, l, c, generator=g)
    return qkv, d_o


def _ref64(qkv, d_o, c):
    x = qkv.double().requires_grad_()
    q, k, v = x[..., :c], x[..., c:2 * c], x[..., 2 * c:]
    y = torch.softmax(q @ k.transpose(1, 2) * (c ** -0.5), dim=-1) @ v
    y.backward(d_o.double())
    return y.detach(), x.grad


def reference(n, l, c):
    """(qkv, d_o, fp64 output, fp64 gradient), computed once per shape and left unchanged"""
    key = (n, l, c)
    if key not in _REF:
        qkv, d_o = _inputs(n, l, c)
        _REF[key] = (qkv, d_o) + _ref64(qkv, d_o, c)
    return _REF[key]


def check_kernel(dev, n, l, c):
    """forward and backward against fp64; two runs agree to the bit"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    qkv, d_o, y64, g64 = reference(n, l, c)
    assert ops.attention_route(n, l, c) == L.ATTN_ROUTE_STREAM
    qd, dd = qkv.to(dev), d_o.to(dev)
    y = ops.attention(qd, c)
    e = rel_err(y, y64)
    print("attention %s forward vs fp64: %.3g" % ((n, l, c), e))
    assert e < TOL_GEMM, e
    assert torch.equal(y, ops.attention(qd, c))
    g = ops.attention_bwd(qd, y, dd, c)
    eg = [rel_err(g[..., i * c:(i + 1) * c], g64[..., i * c:(i + 1) * c]) for i in range(3)]
    print("attention %s backward vs fp64 autograd: dq %.3g dk %.3g dv %.3g" % ((n, l, c), *eg))
    assert max(eg) < TOL_OP and rel_err(g, g64) < TOL_OP, eg
    assert torch.equal(g, ops.attention_bwd(qd, y, dd, c))


def check_forced_stream(dev, n, l, c, monkeypatch):
    """SSDE_ATTN_STREAM=1 at l <= 256: the route query reports STREAM, the result is within tolerance of fp64 and of the default
    route's, which the query reports as F32 or X6"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    qkv, d_o, y64, _ = reference(n, l, c)
    monkeypatch.delenv("SSDE_ATTN_STREAM", raising=False)
    assert ops.attention_route(n, l, c) in (L.ATTN_ROUTE_F32, L.ATTN_ROUTE_X6)
    y_def = ops.attention(qkv.to(dev), c)
    monkeypatch.setenv("SSDE_ATTN_STREAM", "1")
    assert ops.attention_route(n, l, c) == L.ATTN_ROUTE_STREAM
    y = ops.attention(qkv.to(dev), c)
    assert rel_err(y, y64) < TOL_GEMM and rel_err(y_def, y64) < TOL_GEMM, (rel_err(y, y64), rel_err(y_def, y64))
    assert rel_err(y, y_def) < TOL_GEMM


def check_rescale_directions(dev):
    """L = 320, two key blocks.  Batch 0: every row's largest score lies in the LAST key block (the running maximum rises:
    O and l are scaled down); batch 1: in the FIRST (alpha = 1, the second block's terms are small); one row of all-equal scores"""
    from score_sde_pytorch_amd import hipops as ops
    n, l, c = 2, 320, 32
    g = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn(n, l, c, generator=g) for _ in range(3))
    q[..., 0] = 4.0
    k[0, 310, 0], k[1, 5, 0] = 12.0, 12.0
    q[1, 7, :] = 0.0                                  # ties: every score of this row is 0
    s = q.double() @ k.double().transpose(1, 2)
    am = s.argmax(-1)
    assert bool((am[0] == 310).all()) and bool((am[1][torch.arange(l) != 7] == 5).all()) and float(s[1, 7].abs().max()) == 0.0
    qkv = torch.cat([q, k, v], -1)
    d_o = torch.randn(n, l, c, generator=g)
    y64, g64 = _ref64(qkv, d_o, c)
    y = ops.attention(qkv.to(dev), c)
    assert rel_err(y, y64) < TOL_GEMM, rel_err(y, y64)
    assert rel_err(y[1, 7], v[1].double().mean(0)) < TOL_GEMM       # the tie row: the plain mean of v
    gr = ops.attention_bwd(qkv.to(dev), y, d_o.to(dev), c)
    assert rel_err(gr, g64) < TOL_OP, rel_err(gr, g64)


def check_transpose_detecting(dev):
    """test_attention_transpose_detecting at L = 320 (C = 320: one channel per token, two channel passes): query i selects key
    perm[i], the selected keys cross the block boundary, the output must be v[perm]"""
    from score_sde_pytorch_amd import hipops as ops
    n, l, c = 1, 320, 320
    q, k = torch.zeros(n, l, c), torch.zeros(n, l, c)
    perm = torch.randperm(l, generator=torch.Generator().manual_seed(10))
    assert int(((perm >= 256) != (torch.arange(l) >= 256)).sum()) > 32      # many pairs cross the 256-key boundary
    for i in range(l):
        q[0, i, i] = 400.0
        k[0, perm[i], i] = 1.0
    v = torch.arange(l * c, dtype=torch.float32).reshape(1, l, c) / 100.0
    qkv = torch.cat([q, k, v], -1)
    y = ops.attention(qkv.to(dev), c)
    assert rel_err(y, v[:, perm]) < 1e-5, rel_err(y, v[:, perm])
    # backward: the same permutation with a softer selection (q = 100: the selected key holds about half of the row's weight)
    # and values of order 10 -- at q = 400 the true dq and dk are ~1e-8 while dP - D cancels from ~1e4, which measures fp32
    # cancellation and not the kernel; all three gradients against fp64 autograd
    qkv_b = torch.cat([q * 0.25, k, v * 0.01], -1)
    d_o = torch.randn(n, l, c, generator=torch.Generator().manual_seed(11))
    y64, g64 = _ref64(qkv_b, d_o, c)
    assert 0.3 < float(torch.softmax(qkv_b[..., :c].double() @ k.double().transpose(1, 2) * c ** -0.5, -1).max()) < 0.7
    yb = ops.attention(qkv_b.to(dev), c)
    assert rel_err(yb, y64) < TOL_GEMM
    gr = ops.attention_bwd(qkv_b.to(dev), yb, d_o.to(dev), c)
    eg = [rel_err(gr[..., i * c:(i + 1) * c], g64[..., i * c:(i + 1) * c]) for i in range(3)]
    assert max(eg) < TOL_OP and rel_err(gr, g64) < TOL_OP, eg


def _raw(dev, qkv_buf, dst_buf, l, c, bwd=None):
    """one image through the C ABI on caller-owned allocations that are LARGER than the launch (n = 1, l rows)"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    scale = float(c ** -0.5)
    if bwd is None:
        a = L.AttnArgs()
        a.qkv, a.dst, a.n, a.l, a.c, a.scale, a.flags = ops._p(qkv_buf), ops._p(dst_buf), 1, l, c, scale, L.attn_route_flags()
        L.check(L.load().ssde_attention(C.byref(a), ops._stream()), "ssde_attention")
    else:
        o_buf, do_buf, stats_buf = bwd
        a = L.AttnBwdArgs()
        a.qkv, a.o, a.d_o, a.dqkv, a.stats = ops._p(qkv_buf), ops._p(o_buf), ops._p(do_buf), ops._p(dst_buf), ops._p(stats_buf)
        a.n, a.l, a.c, a.scale = 1, l, c, scale
        L.check(L.load().ssde_attention_bwd(C.byref(a), ops._stream()), "ssde_attention_bwd")
    if dev != "cpu":
        torch.cuda.synchronize()


def check_padding_is_inert(dev):
    """L = 272 inside allocations of 336 rows whose tail is NaN (inputs) or a sentinel (outputs): the results are finite and
    equal to the bits of the run on exact-size tensors, and no row beyond L is written"""
    from score_sde_pytorch_amd import hipops as ops
    n, l, c, pad = 1, 272, 32, 64
    qkv, d_o, _, _ = reference(2, 272, 32)
    qkv, d_o = qkv[:1].contiguous(), d_o[:1].contiguous()
    y0 = ops.attention(qkv.to(dev), c)
    g0 = ops.attention_bwd(qkv.to(dev), y0, d_o.to(dev), c)

    def padded(t, fill):
        buf = torch.full((l + pad, t.shape[-1]), fill)
        buf[:l] = t[0].cpu()
        return buf.to(dev)
    SENT = -12345.0
    qb = padded(qkv, float("nan"))
    yb = torch.full((l + pad, c), SENT).to(dev)
    _raw(dev, qb, yb, l, c)
    assert bool(torch.isfinite(yb[:l]).all()) and torch.equal(yb[:l], y0[0])
    assert bool((yb[l:] == SENT).all())
    ob, dob = padded(y0, float("nan")), padded(d_o, float("nan"))
    gb = torch.full((l + pad, 3 * c), SENT).to(dev)
    sb = torch.full((l + pad, 4), SENT).to(dev)
    _raw(dev, qb, gb, l, c, bwd=(ob, dob, sb))
    assert bool(torch.isfinite(gb[:l]).all()) and torch.equal(gb[:l], g0[0])
    assert bool((gb[l:] == SENT).all()) and bool((sb[l:] == SENT).all())


# ---- routing (no device) ------------------------------------------------------------------------------------------------------

def parent_route(l, c, flags):
    """the dispatch of ssde_attention before the streaming kernels existed (l <= 256)"""
    from score_sde_pytorch_amd import _lib as L
    return L.ATTN_ROUTE_X6 if (flags & L.ATTNF_BF16X6) and l == 256 and c <= 256 and c % 64 == 0 else L.ATTN_ROUTE_F32


def check_routes():
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    for flags in (0, L.ATTNF_BF16X6):
        for l in (1, 16, 64, 100, 255, 256):
            for c in (32, 64, 96, 128, 192, 256, 320, 512, 1024):
                assert ops.attention_route(2, l, c, flags) == parent_route(l, c, flags), (l, c, flags)
                if c <= 512:
                    assert ops.attention_route(2, l, c, flags | L.ATTNF_STREAM) == L.ATTN_ROUTE_STREAM
        for l in (257, 272, 1024, 4096, L.ATTN_L_MAX):
            for c in (32, 96, 256, 512):
                assert ops.attention_route(1, l, c, flags) == L.ATTN_ROUTE_STREAM, (l, c, flags)
    lib = L.load()
    for l, c, word in ((L.ATTN_L_MAX + 1, 64, b"token count"), (0, 64, b"token count"), (1024, 48, b"multiple of 32"),
                       (64, 40, b"multiple of 32"), (1024, 544, b"at most 512")):
        a = L.AttnArgs()
        a.n, a.l, a.c = 1, l, c
        assert lib.ssde_attention_route(C.byref(a)) < 0 and word in lib.ssde_last_error(), (l, c, lib.ssde_last_error())
    assert L.attn_route_flags({"SSDE_ATTN_STREAM": "1"}) == L.ATTNF_STREAM
    assert L.attn_route_flags({"SSDE_ATTN_STREAM": "1", "SSDE_MATRIX": "bf16x6"}) == L.ATTNF_STREAM | L.ATTNF_BF16X6
    assert L.attn_route_flags({}) == 0 and L.attn_route_flags({"SSDE_MATRIX": "bf16x6"}) == L.ATTNF_BF16X6


def attention_ops(prog):
    from score_sde_pytorch_amd import _lib as L
    return [prog.ops[i].u.attn for i in range(prog.n) if prog.ops[i].kind == L.OP_ATTN]


# ---- networks -----------------------------------------------------------------------------------------------------------------

def small_model(dev, family="ncsnpp"):
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = A.small_config() if family == "ncsnpp" else A.ddpm_config()
    torch.manual_seed(0)
    model = mutils.get_model(family)(cfg)
    sd = {k: v.clone() for k, v in _util.load_seeded(model, seed=1).items()}
    if hasattr(model, "sigmas"):
        sd["sigmas"] = model.sigmas.clone()
    return cfg, model.to(dev).eval(), sd


def check_net_forward(dev, family="ncsnpp", tol=TOL_FWD):
    """the small net with attention at 32 x 32 against the REFERENCE's forward (tests/golden/unet_small_<family>_attn32.npz)"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    gold = np.load(os.path.join(_util.GOLDEN, "unet_small_%s_attn32.npz" % family))
    cfg, model, _ = small_model(dev, family)
    x, cond, y_ref = (torch.from_numpy(gold[k]) for k in ("x", "cond", "y"))
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    eng.validate_plans()
    routes = [(a.l, L.load().ssde_attention_route(C.byref(a))) for a in attention_ops(eng.program)]
    assert any(l == 1024 for l, _ in routes) and all((r == L.ATTN_ROUTE_STREAM) == (l > 256) for l, r in routes), routes
    y = eng.forward(x.to(dev), cond.to(dev))
    err = rel_err(y, y_ref)
    print("small %s net, attention at 32 x 32, forward vs reference: rel err %.3g" % (family, err))
    assert err < tol, err
    assert torch.equal(y, eng.forward(x.to(dev), cond.to(dev)))
    return eng, y


def check_net_grads(dev):
    """every parameter gradient and the input gradient (what the likelihood uses) against autograd through the CPU oracle"""
    from score_sde_pytorch_amd import backward as B, _lib as L
    cfg, model, sd = small_model(dev)
    x, sig = A.forward_inputs(cfg)
    gout = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
    y_ref, gx_ref, ref = T.oracle_grads(cfg, sd, x, sig, gout)
    R = cfg.data.image_size
    eng = B.TrainEngine(model, x.shape[0], R, R, torch.device(dev), input_grad=True, dropout=False)
    bwd = [eng.program.ops[i].u.attn_bwd.l for i in range(eng.program.n) if eng.program.ops[i].kind == L.OP_ATTN_BWD]
    assert sorted(set(bwd)) == [256, 1024], bwd
    y = eng.forward_train(x.to(dev), sig.to(dev)).clone()
    assert rel_err(y, y_ref) < TOL_FWD, rel_err(y, y_ref)
    eng.backward(gout.to(dev))
    e = rel_err(eng.gx_view(), gx_ref)
    assert e < TOL_GRAD, e
    worst = T.compare_param_grads(model, eng.flat, ref, tol=TOL_GRAD)
    print("small ncsnpp net, attention at 32 x 32, gradients vs oracle autograd: input %.3g, worst parameter %.3g" % (e, worst))
    g1, gx1 = eng.flat.grad.clone(), eng.gx_view().clone()
    eng.forward_train(x.to(dev), sig.to(dev))
    eng.backward(gout.to(dev))
    assert torch.equal(g1, eng.flat.grad) and torch.equal(gx1, eng.gx_view())


def check_train_steps_against_reference_run(dev):
    """three steps of losses.get_step_fn on the net against the REFERENCE's run (tests/golden/train_small_attn32.npz)"""
    gold = np.load(os.path.join(_util.GOLDEN, "train_small_attn32.npz"))
    name, case = A.TRAIN_NAME, A.TRAIN_CASE
    from score_sde_pytorch_amd.models import utils as mutils, ema as ema_mod
    from score_sde_pytorch_amd import losses, sde_lib
    _, _, _, continuous, reduce_mean, lw = case
    cfg = A.train_config()
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


def check_plan_round_trip(dev, tmp_path, link):
    """a plan blob of the net: the Python binding of the plan entries gives the engine's bits, and tests/c_host/plan_host.c
    (built by `link`) reproduces the reference's forward from the blob alone"""
    import subprocess
    from score_sde_pytorch_amd import engine as E, plan_export as P, _lib as L
    gold = np.load(os.path.join(_util.GOLDEN, "unet_small_ncsnpp_attn32.npz"))
    cfg, model, _ = small_model(dev)
    x, sig = torch.from_numpy(gold["x"]), torch.from_numpy(gold["cond"])
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    y = eng.forward(x.to(dev), sig.to(dev))
    blob = P.export_unet_plan(eng)
    hdr = P.PlanHeader.from_buffer_copy(blob[: C.sizeof(P.PlanHeader)])
    assert hdr.abi_version == L.ABI_VERSION
    plan = P.LoadedPlan(blob)
    try:
        y2 = plan.unet_forward(x.to(dev).contiguous(), sig.to(dev).contiguous())
    finally:
        plan.close()
    assert torch.equal(y, y2)
    for k in ("x", "cond", "y"):
        np.ascontiguousarray(gold[k], dtype=np.float32).tofile(str(tmp_path / (k + ".f32")))
    blob_path = str(tmp_path / "plan.blob")
    with open(blob_path, "wb") as f:
        f.write(blob)
    exe = link(str(tmp_path / "plan_host"))
    r = subprocess.run([exe, blob_path] + [str(tmp_path / (k + ".f32")) for k in ("x", "cond", "y")] + ["1e-4"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "plan_host:" in r.stdout, (r.returncode, r.stdout, r.stderr)
