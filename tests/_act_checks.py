"""Checks of the elu / relu / lrelu networks (config.model.nonlinearity, get_act: models/layers.py:29-41): ssde_src.act in
ssde_gn_apply / ssde_gn_apply_bwd, the refusals of every other entry point, the lowering that materialises every
normalise-and-activate site and act(temb), training, plans and the constructor.  Shared by the emulator suite
(tests/test_act_cpu.py) and the GPU suite (tests/test_act_gpu.py); the cases at the top are also what tools/gen_golden_act.py
records.  Tolerances are the project's (tests/_gn_width_checks.py): element-wise 2e-6, contraction 2e-5, a whole
forward 1e-4 (2e-6 for the small nets on the emulator's exact-fp32 arithmetic), gradients 2e-4."""
import ctypes as C
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

import _util
import _gn_width_checks as K
import _train_checks as T
from _util import rel_err

TOL_ELEM, TOL_CONTRACT, TOL_FWD, TOL_GRAD = K.TOL_ELEM, K.TOL_CONTRACT, K.TOL_FWD, K.TOL_GRAD

ACTS = ("elu", "relu", "lrelu")
# (c0, c1, groups): a 6-wide group that straddles the two halves, a concatenation, a group that ends mid-quad
KERNEL_SHAPES = [(128, 64, 32), (96, 128, 32), (20, 0, 4)]
KERNEL_MAPS = [4, 8]
# relu and lrelu have a kink at 0: the inputs are chosen so that the fp64 pre-activation stays this far from it -- 5 times the
# element-wise tolerance at this data's max |u| of about 5 -- and no fp32 u can lie on the other side of 0 (no element is excluded)
KINK_MARGIN = 5e-5
KINK_TRIES = 6
ACT_ONLY_SHAPES = [(3, 1, 128), (3, 16, 20)]          # [n, hw, C]: the time embedding's shape, and a ragged one

# ---- the recorded cases (tools/gen_golden_act.py) ------------------------------------------------------------------
# tests/golden/<name>.npz: x, cond, y of one forward of the reference on _util.small_config(kind) with the activation overridden;
# inputs as oracle/gen_golden.py draws them for unet_small_ncsnpp / unet_small_ddpmpp
FORWARD_CASES = {"unet_small_ncsnpp_elu": ("ncsnpp", "elu"), "unet_small_ncsnpp_relu": ("ncsnpp", "relu"),
                 "unet_small_ncsnpp_lrelu": ("ncsnpp", "lrelu"), "unet_small_ddpmpp_elu": ("ddpmpp", "elu")}
FORWARD_BATCH = 3
# tests/golden/train_small_elu.npz: the continuous VE loss on the small NCSN++ network with ELU and dropout 0.1, the layout of
# train_small_ddpm.npz.  The reference's nn.Dropout draws from torch's generator; the recorder puts this package's mask -- a
# pure function of (seed word, block salt, element index) -- in its place (hash_dropout below), with the seed words the fused
# step uses after torch.manual_seed(0) (step_seed) and GRAD_SEED for the gradient case.
TRAIN_NAME = "ve_cont_elu"
TRAIN_CASE = ("ncsnpp", {}, "vesde", True, False, False)      # the layout of tests/_util.TRAIN_CASES entries
TRAIN_DROPOUT = 0.1
TRAIN_PROBE_LIMIT = 5000
GRAD_SEED = 5


def forward_config(name):
    kind, act = FORWARD_CASES[name]
    cfg = _util.small_config(kind)
    cfg.model.nonlinearity = act
    return cfg


def forward_inputs(name):
    cfg = forward_config(name)
    g = torch.Generator().manual_seed(123)
    R, batch = cfg.data.image_size, FORWARD_BATCH
    x = torch.rand(batch, 3, R, R, generator=g) if not cfg.data.centered else torch.rand(batch, 3, R, R, generator=g) * 2 - 1
    if FORWARD_CASES[name][0] == "ncsnpp":
        cond = torch.exp(torch.rand(batch, generator=g) * (np.log(50.0) - np.log(0.01)) + np.log(0.01)).float()
        x = x + cond[:, None, None, None] * torch.randn(batch, 3, R, R, generator=g)
    else:
        cond = (torch.rand(batch, generator=g) * 999).float()
    return x, cond


def train_config(act="elu", dropout=TRAIN_DROPOUT):
    cfg = _util.train_case_config(TRAIN_CASE)
    cfg.model.nonlinearity = act
    cfg.model.dropout = dropout
    return cfg


def step_seed(count):
    """the dropout seed word of the fused step's call `count` after torch.manual_seed(0), one rank (losses.FusedTrainStep)"""
    from score_sde_pytorch_amd import losses
    assert int(torch.initial_seed()) == 0
    return losses.FusedTrainStep._dropout_seed(types.SimpleNamespace(steps_done=count)) & 0x7FFFFFFF


def hash_dropout(model, p, holder):
    """Replace Dropout_0 of every residual block of a REFERENCE model (all_modules order = the lowering's block count) by this
    package's mask: element e = ((n H + y) W + x) C + c of the block's NHWC tensor is kept when hash32(e * 0x9E3779B1 + (seed ^
    salt)) >= p 2^32, salt = 0x9E3779B1 * block number (include/ssde.h, engine.UNetEngine._res).  holder.seed: the seed word."""
    thresh = min(int(round(p * 2.0 ** 32)), 2 ** 32 - 1)

    class HashDropout(torch.nn.Module):
        def __init__(self, salt):
            super().__init__()
            self.salt = salt & 0xFFFFFFFF

        def forward(self, h):
            if not self.training:
                return h
            n, c, hh, ww = h.shape
            keep = T.hash_keep(np.arange(n * hh * ww * c, dtype=np.uint64), (holder.seed ^ self.salt) & 0xFFFFFFFF, thresh, 1.0 / (1.0 - p))
            return h * torch.from_numpy(keep).to(h.dtype).reshape(n, hh, ww, c).permute(0, 3, 1, 2)
    blocks = [m for m in model.all_modules if hasattr(m, "Dropout_0")]
    for i, m in enumerate(blocks):
        m.Dropout_0 = HashDropout(0x9E3779B1 * (i + 1))
    return len(blocks)


# ---- fp64 references -------------------------------------------------------------------------------------------------
def act64(act, u):
    return {"swish": F.silu, "elu": F.elu, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, 0.2)}[act](u)


def _act_id(act):
    from score_sde_pytorch_amd import _lib as L
    return L.ACT_BY_NAME[act]


def _ref64(xc, groups, gamma, beta, act, mask, dy, eps=1e-6):
    """fp64: u = GroupNorm(x), y = mask * act(u) and its gradients, NHWC"""
    x = xc.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    ga, be = gamma.double().requires_grad_(), beta.double().requires_grad_()
    u = F.group_norm(x, groups, ga, be, eps)
    y = act64(act, u)
    if mask is not None:
        y = y * mask.double().permute(0, 3, 1, 2)
    y.backward(dy.double().permute(0, 3, 1, 2))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()      # noqa: E731
    return nhwc(u.detach()), nhwc(y.detach()), nhwc(x.grad), ga.grad, be.grad


def _keep_mask(n_elem, shape, drop_p, salt, seed_word):
    thresh = min(int(round(drop_p * 2.0 ** 32)), 2 ** 32 - 1)
    return torch.from_numpy(T.hash_keep(np.arange(n_elem, dtype=np.uint64), seed_word ^ salt, thresh, 1.0 / (1.0 - drop_p))).reshape(shape)


def kernel_case(act, c0, c1, groups, side):
    """the inputs of one kernel case: _gn_width_checks._case with seed 100 c0 + c1 + side + 1000003 k, k the smallest of 0..5 whose
    fp64 pre-activation keeps KINK_MARGIN from 0 (relu, lrelu); ELU is C1 and takes k = 0"""
    for k in range(KINK_TRIES):
        xc, gamma, beta, dy = K._case(c0, c1, side, seed=100 * c0 + c1 + side + 1000003 * k)
        if act == "elu":
            return k, (xc, gamma, beta, dy)
        u = F.group_norm(xc.double().permute(0, 3, 1, 2), groups, gamma.double(), beta.double(), 1e-6)
        if float(u.abs().min()) >= KINK_MARGIN:
            return k, (xc, gamma, beta, dy)
    raise AssertionError("no seed in 0..%d keeps the fp64 pre-activation %g away from the kink (%s, %d + %d, %dx%d)"
                         % (KINK_TRIES - 1, KINK_MARGIN, act, c0, c1, side, side))


# ---- 1. the apply launch and its adjoint against fp64 ------------------------------------------------------------------
def check_kernels(dev, act, c0, c1, groups, side):
    """ssde_gn_apply / ssde_gn_apply_bwd with src.act, with and without dropout: y, dx into both halves (p0's accumulated onto a
    base, p1's written), dgamma and dbeta against fp64; a second call gives the same bits"""
    from score_sde_pytorch_amd import hipops as ops
    d = lambda t: t.to(dev)  # noqa: E731
    A = _act_id(act)
    k, (xc, gamma, beta, dy) = kernel_case(act, c0, c1, groups, side)
    n, Ct, hw = xc.shape[0], c0 + c1, side * side
    xa = d(xc[..., :c0].contiguous())
    xb = d(xc[..., c0:].contiguous()) if c1 else None
    drop_p, salt, seed_word = 0.25, 0x1234567, 77
    seed_t = torch.tensor([seed_word], dtype=torch.int32).to(dev)
    keep = _keep_mask(n * hw * Ct, (n, side, side, Ct), drop_p, salt, seed_word)
    mean, rstd = ops.groupnorm_stats(xa, groups, 1e-6, xb)
    gn = (mean, rstd, d(gamma), d(beta), groups)
    for mask in (None, keep):
        drop = (drop_p, seed_t, salt) if mask is not None else None
        u64, y64, dx64, dg64, db64 = _ref64(xc, groups, gamma, beta, act, mask, dy)
        assert act == "elu" or float(u64.abs().min()) >= KINK_MARGIN
        y = ops.groupnorm_apply(xa, gn, xb, silu=True, drop=drop, act=A)
        assert tuple(y.shape) == (n, side, side, Ct)
        e_y = rel_err(y, y64)
        base = torch.randn(n, side, side, c0, generator=torch.Generator().manual_seed(1))
        slices = 2 if hw >= 64 else 1
        dx0, dx1, dga, dbe = ops.groupnorm_apply_bwd(d(dy), xa, gn, xb, silu=True, drop=drop, slices=slices, g0=d(base.clone()), act=A)
        e_dx0 = rel_err(dx0.cpu() - base, dx64[..., :c0])
        e_dx1 = rel_err(dx1, dx64[..., c0:]) if c1 else 0.0
        e_dg, e_db = rel_err(dga, dg64), rel_err(dbe, db64)
        print("gn_apply %s %d+%d in %d, %dx%d, k=%d, dropout %d: y %.3g dx0 %.3g dx1 %.3g dgamma %.3g dbeta %.3g"
              % (act, c0, c1, groups, side, side, k, mask is not None, e_y, e_dx0, e_dx1, e_dg, e_db))
        if mask is not None:            # the mask itself is exact
            assert torch.equal(y.cpu() == 0, (keep == 0) | (y64 == 0).to(torch.bool))
        assert e_y < TOL_ELEM, ("apply", act, e_y)
        assert e_dx0 < TOL_CONTRACT and e_dx1 < TOL_CONTRACT, (act, e_dx0, e_dx1)
        assert e_dg < TOL_CONTRACT and e_db < TOL_CONTRACT, (act, e_dg, e_db)
        again = ops.groupnorm_apply_bwd(d(dy), xa, gn, xb, silu=True, drop=drop, slices=slices, g0=d(base.clone()), act=A)
        assert all(torch.equal(a, b) for a, b in zip((dx0, dga, dbe), (again[0], again[2], again[3])))
        assert dx1 is None or torch.equal(dx1, again[1])
        assert torch.equal(y, ops.groupnorm_apply(xa, gn, xb, silu=True, drop=drop, act=A))


# ---- 2. the activation alone (SSDE_PRO_SILU through the apply launch) ---------------------------------------------------
def act_only_case(act, shape):
    n, hw, c = shape
    for k in range(KINK_TRIES):
        g = torch.Generator().manual_seed(7 * c + hw + 1000003 * k)
        x = torch.randn(n, hw, c, generator=g) * 2.0
        dy = torch.randn(n, hw, c, generator=g)
        if act in ("swish", "elu") or float(x.abs().min()) >= KINK_MARGIN:
            return x, dy
    raise AssertionError("no seed in 0..%d keeps x %g away from the kink (%s, %s)" % (KINK_TRIES - 1, KINK_MARGIN, act, shape))


def check_act_only(dev, act, shape):
    """dst = drop(act(x)) and dx = dy * mask * act'(x), no statistics and no affine, against fp64 (element-wise)"""
    from score_sde_pytorch_amd import hipops as ops
    d = lambda t: t.to(dev)  # noqa: E731
    A = _act_id(act)
    x, dy = act_only_case(act, shape)
    n, hw, c = shape
    drop_p, salt, seed_word = 0.25, 0x7654321, 91
    seed_t = torch.tensor([seed_word], dtype=torch.int32).to(dev)
    keep = _keep_mask(n * hw * c, shape, drop_p, salt, seed_word)
    for mask in (None, keep):
        drop = (drop_p, seed_t, salt) if mask is not None else None
        x64 = x.double().requires_grad_()
        y64 = act64(act, x64) * (mask.double() if mask is not None else 1.0)
        y64.backward(dy.double())
        y = ops.groupnorm_apply(d(x), None, act=A, drop=drop)
        assert tuple(y.shape) == shape
        base = torch.randn(shape, generator=torch.Generator().manual_seed(2))
        dx_acc, _, dga, dbe = ops.groupnorm_apply_bwd(d(dy), d(x), None, act=A, drop=drop, g0=d(base.clone()))
        dx, _, _, _ = ops.groupnorm_apply_bwd(d(dy), d(x), None, act=A, drop=drop)
        assert dga is None and dbe is None
        e_y, e_dx, e_acc = rel_err(y, y64.detach()), rel_err(dx, x64.grad), rel_err(dx_acc.cpu() - base, x64.grad)
        print("act only %s %s dropout %d: y %.3g dx %.3g dx (accumulated) %.3g" % (act, shape, mask is not None, e_y, e_dx, e_acc))
        assert e_y < TOL_ELEM and e_dx < TOL_ELEM and e_acc < TOL_ELEM, (act, shape, e_y, e_dx, e_acc)
        assert torch.equal(dx, ops.groupnorm_apply_bwd(d(dy), d(x), None, act=A, drop=drop)[0])


def check_act_only_silu_is_the_fused_prologue(dev, shape):
    """SiLU through the apply launch, then an identity 1x1 GEMM, against the GEMM that applies SSDE_PRO_SILU itself"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    n, hw, c = shape
    x, _ = act_only_case("swish", shape)
    x4 = x.reshape(n, hw, 1, c).to(dev)
    eye = torch.eye(c)
    y = ops.groupnorm_apply(x4, None, act=L.ACT_SILU)
    a = ops.conv2d(aux=y, aux_weight=eye)
    b = ops.conv2d(aux=x4, aux_weight=eye, aux_pro=L.PRO_SILU)
    assert rel_err(a, b) < TOL_CONTRACT, rel_err(a, b)
    assert rel_err(a, F.silu(x4.double().cpu())) < TOL_CONTRACT


# ---- 3. refusals ------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    """every entry point but the apply launches refuses src.act != 0 by its own name, before any launch (the outputs keep their
    sentinel); ssde_gn_apply refuses a value outside SSDE_ACT_*"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    lib = L.load()
    n, side, c = 2, 4, 32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, side, side, c, generator=g).to(dev)
    dp = torch.randn(n, side, side, c, generator=g).to(dev)
    mean, rstd = ops.groupnorm_stats(x, 8)
    gamma, beta = torch.ones(c).to(dev), torch.zeros(c).to(dev)
    gn = (mean, rstd, gamma, beta, 8)
    sentinel = lambda *shape: torch.full(shape, 12345.0).to(dev)       # noqa: E731
    p = ops._p
    st = ops._stream()

    def refused(rc, entry, out):
        msg = lib.ssde_last_error().decode()
        assert rc != 0, entry
        assert entry in msg and "activation %d" % L.ACT_ELU in msg, (entry, msg)
        if dev != "cpu":
            torch.cuda.synchronize()
        assert bool((out == 12345.0).all()), entry

    # ssde_conv2d: the 3x3 source and the 1x1 source
    for which in ("main", "aux"):
        a = L.ConvArgs()
        out = sentinel(n, side, side, 64)
        w3 = ops.pack_conv_weight(torch.randn(64, c, 3, 3, generator=g).to(dev))
        w1 = ops.pack_matrix(torch.randn(64, c, generator=g).to(dev))
        if which == "main":
            ops._fill_src(a.main, x, None, L.PRO_GN_SILU, gn, act=L.ACT_ELU)
            a.w_main, a.ksize, a.stride, a.pad, a.h_in, a.w_in = p(w3), 3, 1, 1, side, side
        else:
            ops._fill_src(a.aux, x, None, L.PRO_SILU, None, act=L.ACT_ELU)
            a.w_aux, a.ksize, a.stride, a.pad = p(w1), 0, 1, 0
        a.n, a.h_out, a.w_out, a.c_out, a.out_scale, a.dst = n, side, side, 64, 1.0, p(out)
        refused(lib.ssde_conv2d(C.byref(a), st), "conv", out)
        assert which in lib.ssde_last_error().decode()
    # ssde_upfirdn2d
    a = L.UpfirdnArgs()
    out = sentinel(n, side, side, c)
    ops._fill_src(a.src, x, None, L.PRO_GN_SILU, gn, act=L.ACT_ELU)
    a.n, a.h_in, a.w_in, a.c, a.h_out, a.w_out = n, side, side, c, side, side
    a.up, a.down, a.pad0, a.pad1, a.kh, a.kw = 1, 1, 0, 0, 1, 1
    a.k[0] = 1.0
    a.dst = p(out)
    refused(lib.ssde_upfirdn2d(C.byref(a), st), "upfirdn2d", out)
    # ssde_conv_wgrad
    a = L.WgradArgs()
    out = sentinel(64, c, 3, 3)
    ops._fill_src(a.src, x, None, L.PRO_GN_SILU, gn, act=L.ACT_ELU)
    gy = torch.randn(n, side, side, 64, generator=g).to(dev)
    a.g, a.g_ld, a.g_off, a.n, a.h_in, a.w_in, a.h_out, a.w_out, a.c_out = p(gy), 64, 0, n, side, side, side, side, 64
    a.ksize, a.stride, a.pad, a.cin_store, a.scale, a.dw = 3, 1, 1, c, 1.0, p(out)
    refused(lib.ssde_conv_wgrad(C.byref(a), st), "wgrad", out)
    # ssde_prologue_bwd
    a = L.PrologueBwdArgs()
    out = sentinel(n, side, side, c)
    ops._fill_src(a.src, x, None, L.PRO_SILU, None, act=L.ACT_ELU)
    a.dp, a.dp_ld, a.dp_off, a.n, a.hw, a.scale, a.g0 = p(dp), c, 0, n, side * side, 1.0, p(out)
    refused(lib.ssde_prologue_bwd(C.byref(a), st), "prologue_bwd", out)
    # ssde_gn_bwd_reduce
    a = L.GnBwdReduceArgs()
    out = sentinel(n, side, side, c)
    dga, dbe = sentinel(c), sentinel(c)
    sums, scratch = sentinel(n, 8, 2), sentinel(n * c * 2)
    ops._fill_src(a.src, x, None, L.PRO_GN_SILU, gn, act=L.ACT_ELU)
    a.dp, a.n, a.hw, a.sums, a.dgamma, a.dbeta, a.scratch, a.slices, a.g0, a.scale = p(dp), n, side * side, p(sums), p(dga), p(dbe), p(scratch), 1, p(out), 1.0
    refused(lib.ssde_gn_bwd_reduce(C.byref(a), st), "gn_bwd_reduce", torch.cat([out.reshape(-1), dga, dbe, sums.reshape(-1), scratch]))
    # ssde_gn_apply / ssde_gn_apply_bwd: a value that is none of SSDE_ACT_*
    for bad in (4, -1):
        a = L.GnApplyArgs()
        out = sentinel(n, side, side, c)
        ops._fill_src(a.src, x, None, L.PRO_GN_SILU, gn, act=bad)
        a.n, a.hw, a.dst = n, side * side, p(out)
        assert lib.ssde_gn_apply(C.byref(a), st) != 0
        msg = lib.ssde_last_error().decode()
        assert "gn_apply" in msg and "activation %d" % bad in msg, msg
        assert bool((out == 12345.0).all())
    with_bad = pytest_raises(L.SsdeError, lambda: ops.groupnorm_apply_bwd(dp, x, gn, act=7))
    assert "gn_apply_bwd" in with_bad and "activation 7" in with_bad, with_bad
    # and SiLU (act = 0) still passes everywhere: one fused launch as a witness
    assert bool(torch.isfinite(ops.conv2d(aux=x, aux_weight=torch.eye(c), aux_pro=L.PRO_SILU)).all())


def pytest_raises(exc, fn):
    try:
        fn()
    except exc as e:
        return str(e)
    raise AssertionError("%s was not raised" % exc.__name__)


# ---- 4. whole forward ---------------------------------------------------------------------------------------------------
_SRCS = None


def op_sources(op):
    """every ssde_src of a program op"""
    from score_sde_pytorch_amd import _lib as L
    global _SRCS
    if _SRCS is None:
        _SRCS = {L.OP_CONV: lambda u: (u.conv.main, u.conv.aux), L.OP_UPFIRDN: lambda u: (u.fir.src,), L.OP_WGRAD: lambda u: (u.wgrad.src,),
                 L.OP_GN_BWD_REDUCE: lambda u: (u.gn_bwd.src,), L.OP_PROLOGUE_BWD: lambda u: (u.pro_bwd.src,),
                 L.OP_GN_APPLY: lambda u: (u.gn_apply.src,), L.OP_GN_APPLY_BWD: lambda u: (u.gn_apply_bwd.src,)}
    return _SRCS.get(int(op.kind), lambda u: ())(op.u)


def program_acts(prog):
    """(op kinds, the act word of every source of every op: [(op kind, act)])"""
    kinds, acts = [], []
    for i in range(prog.n):
        op = prog.ops[i]
        kinds.append(int(op.kind))
        acts.extend((int(op.kind), int(s.act)) for s in op_sources(op))
    return kinds, acts


def assert_act_words(prog, act, backward=False):
    """OP_GN_APPLY launches carry the model's activation; no op but OP_GN_APPLY / OP_GN_APPLY_BWD carries a non-zero word, and no
    consumer applies an activation itself"""
    from score_sde_pytorch_amd import _lib as L
    kinds, acts = program_acts(prog)
    A = L.ACT_BY_NAME[act]
    assert kinds.count(L.OP_GN_APPLY) >= 3
    assert all(a == 0 for k, a in acts if k not in (L.OP_GN_APPLY, L.OP_GN_APPLY_BWD)), acts
    assert any(a == A for k, a in acts if k == L.OP_GN_APPLY)
    assert all(a in (0, A) for _, a in acts)
    for i in range(prog.n):
        op = prog.ops[i]
        for s in op_sources(op):
            if int(op.kind) not in (L.OP_GN_APPLY, L.OP_GN_APPLY_BWD):
                assert s.pro_mode not in (L.PRO_GN_SILU, L.PRO_SILU), (int(op.kind), s.pro_mode)
            elif s.pro_mode in (L.PRO_GN_SILU, L.PRO_SILU):
                assert s.act == A
    if backward:
        assert kinds.count(L.OP_GN_APPLY_BWD) >= 3
    return kinds


def model_of(cfg, dev):
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    sd = {k: v.clone() for k, v in _util.load_seeded(model, seed=1).items()}
    return model.to(dev), sd


def check_forward(dev, name, tol):
    """one forward against the REFERENCE's (tests/golden/<name>.npz)"""
    from score_sde_pytorch_amd import engine as E
    gold = np.load(os.path.join(_util.GOLDEN, name + ".npz"))
    cfg = forward_config(name)
    model, _ = model_of(cfg, dev)
    x, cond, y_ref = (torch.from_numpy(gold[k]) for k in ("x", "cond", "y"))
    xi, ci = forward_inputs(name)
    assert torch.equal(x, xi) and torch.equal(cond, ci)
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
    assert_act_words(eng.program, FORWARD_CASES[name][1])
    y = eng.forward(x.to(dev), cond.to(dev))
    err = rel_err(y, y_ref)
    print("%s (SSDE_WINOGRAD=%s) forward vs reference: rel err %.3g" % (name, os.environ.get("SSDE_WINOGRAD", "1"), err))
    assert err < tol, (name, err)
    assert torch.equal(y, eng.forward(x.to(dev), cond.to(dev)))


# ---- 5. one program for every activation ------------------------------------------------------------------------------
def check_same_program_for_every_activation():
    """dry lowering of _util.small_config(): forward and training programs of elu, relu and lrelu have the same op kinds and
    differ from each other in the act words only; the swish program has no apply launch"""
    from score_sde_pytorch_amd import engine as E, backward as B, _lib as L
    fwd, trn = {}, {}
    for act in ACTS + ("swish",):
        cfg = _util.small_config()
        cfg.model.nonlinearity = act
        model, _ = model_of(cfg, "cpu")
        R = cfg.data.image_size
        fwd[act] = program_acts(E.UNetEngine(model, 2, R, R, "cpu").program)
        trn[act] = program_acts(B.TrainEngine(model, 2, R, R, "cpu", input_grad=True).program)
    for progs in (fwd, trn):
        assert progs["elu"][0] == progs["relu"][0] == progs["lrelu"][0]
        assert L.OP_GN_APPLY not in progs["swish"][0] and all(a == 0 for _, a in progs["swish"][1])
        for act in ACTS:
            A = L.ACT_BY_NAME[act]
            assert [(k, A if a else 0) for k, a in progs["elu"][1]] == progs[act][1]
    assert trn["elu"][0].count(L.OP_GN_APPLY_BWD) == trn["elu"][0].count(L.OP_GN_APPLY) == fwd["elu"][0].count(L.OP_GN_APPLY)


# ---- 6. gradients and training, ELU ------------------------------------------------------------------------------------
def _train_state(dev):
    from score_sde_pytorch_amd.models import ema as ema_mod
    from score_sde_pytorch_amd import losses, sde_lib
    _, _, _, continuous, reduce_mean, lw = TRAIN_CASE
    cfg = train_config()
    model, init = model_of(cfg, dev)
    sde = _util.train_case_sde(sde_lib, TRAIN_CASE, cfg)
    opt = losses.get_optimizer(cfg, model.parameters())
    ema = ema_mod.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    optimize_fn = losses.optimization_manager(cfg)
    kw = dict(optimize_fn=optimize_fn, reduce_mean=reduce_mean, continuous=continuous, likelihood_weighting=lw)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    return cfg, init, state, losses.get_step_fn(sde, train=True, **kw), losses.get_step_fn(sde, train=False, **kw)


def check_loss_and_gradients(dev):
    """the continuous VE loss of the first batch with dropout seed GRAD_SEED: the loss, the norm of EVERY parameter gradient and
    the probe tensors in full against the reference's loss.backward() (tests/golden/train_small_elu.npz); twice, same bits"""
    name = TRAIN_NAME
    gold = np.load(os.path.join(_util.GOLDEN, "train_small_elu.npz"))
    cfg, _, state, train_step, _ = _train_state(dev)
    batch, u, labels, z = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)[0]
    fs = train_step.fused_for(state, batch.to(dev))
    assert fs is not None
    assert_act_words(fs.eng.program, "elu", backward=True)
    t = u * (1 - 1e-5) + 1e-5                                     # losses.py:84
    loss = float(fs.loss_and_grads(batch.to(dev), t=t.to(dev), z=z.to(dev), seed=GRAD_SEED))
    ref_loss = float(gold[name + "/grad_loss"])
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    params = [(n, p) for n, p in state["model"].named_parameters() if p.requires_grad]
    gnorms = gold[name + "/gnorms"]
    assert len(params) == gnorms.shape[0]
    worst = 0.0
    for (n, p), ref in zip(params, gnorms):
        got = float(fs.flat.grad_view(p).double().norm())
        if ref < 1e-4:                   # analytically-zero gradients (the key bias of attention): compared absolutely
            assert got < 1e-4, (n, got)
            continue
        worst = max(worst, abs(got - ref) / ref)
        assert abs(got - ref) <= TOL_GRAD * ref, (n, got, ref)
    probes = {k.split("/", 2)[2]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(name + "/g/")}
    assert len(probes) >= 20
    worst_p = T.compare_param_grads(types.SimpleNamespace(named_parameters=lambda: [(n, p) for n, p in params if n in probes]),
                                    fs.flat, probes, tol=TOL_GRAD)
    print("elu training gradients: worst norm error %.3g over %d tensors, worst probe %.3g over %d" % (worst, len(params), worst_p, len(probes)))
    g1 = fs.flat.grad.clone()
    loss2 = float(fs.loss_and_grads(batch.to(dev), t=t.to(dev), z=z.to(dev), seed=GRAD_SEED))
    assert loss2 == loss and torch.equal(g1, fs.flat.grad)


def check_train_steps_against_reference_run(dev):
    """three steps of losses.get_step_fn on the ELU network with dropout 0.1 against the REFERENCE's run with the same masks
    (tests/golden/train_small_elu.npz), then the eval step"""
    name = TRAIN_NAME
    gold = np.load(os.path.join(_util.GOLDEN, "train_small_elu.npz"))
    cfg, init, state, train_step, eval_step = _train_state(dev)
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
    fs = train_step.fused_for(state, inputs[0][0].to(dev))
    assert fs.steps_done == _util.TRAIN_STEPS, "the steps must have run as the fused step"
    batch, u, labels, z = inputs[_util.TRAIN_STEPS]
    with _util.inject_rng(u, labels, z):
        eval_loss = float(eval_step(state, batch.to(dev)))
    ref_eval = float(gold[name + "/eval_loss"])
    assert abs(eval_loss - ref_eval) <= 1e-5 * abs(ref_eval), (eval_loss, ref_eval)
    return losses_, state["model"]


# ---- 7. plans -----------------------------------------------------------------------------------------------------------
def check_unet_plan_round_trip(dev):
    """a U-Net plan of the ELU network through plan_export and LoadedPlan: the engine's bits"""
    from score_sde_pytorch_amd import engine as E, plan_export as P, _lib as L
    name = "unet_small_ncsnpp_elu"
    model, _ = model_of(forward_config(name), dev)
    x, cond = forward_inputs(name)
    eng = E.UNetEngine(model, x.shape[0], x.shape[2], x.shape[3], torch.device(dev))
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


def check_train_plan_round_trip(dev, n_steps=2):
    """a training plan of the ELU network with dropout: whole steps through ssde_train_step against the Python-driven fused
    step (the pattern of _train_checks.check_train_plan)"""
    from score_sde_pytorch_amd import plan_export
    cfg, _, state, train_step, _ = _train_state(dev)
    from score_sde_pytorch_amd import losses
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


def check_pc_plan(dev, steps=4, B=2):
    """a 4-step PC sampler plan (reverse diffusion + Langevin) of the ELU network, exported without its random-number launches and
    fed the noise pc_engine is fed: the same state"""
    from score_sde_pytorch_amd import pc_engine, plan_export, sampling, sde_lib
    name = "unet_small_ncsnpp_elu"
    cfg = forward_config(name)
    model, _ = model_of(cfg, dev)
    model.eval()
    R = cfg.data.image_size
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=steps)
    plan_ = pc_engine.plan_fused(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, model, True,
                                 types.SimpleNamespace(is_cuda=True))
    eng = pc_engine.FusedPCSampler(model, sde, plan_, (B, 3, R, R), snr=0.16, n_steps=1, probability_flow=False, eps=1e-5,
                                   device=torch.device(dev))
    assert_act_words(eng.step_program(with_rng=False), "elu")
    x_T, noises = _util.pc_case_inputs(B, steps, 50.0, R, seed=11)
    x_T, noises = x_T.to(dev).contiguous(), noises.to(dev).contiguous()
    x, x_mean = eng.run(x_T, noises=noises)
    assert bool(torch.isfinite(x).all())
    plan = plan_export.LoadedPlan(plan_export.export_pc_plan(eng, with_rng=False))
    try:
        plan.pc_reset(x_T, 0)
        for i in range(steps):
            plan.pc_set_noise(0, noises[i, 0])
            plan.pc_set_noise(1, noises[i, 1])
            plan.pc_run(1)
        px, pm = plan.pc_state(x_T)
        if dev != "cpu":
            torch.cuda.synchronize()
    finally:
        plan.close()
    assert torch.equal(px.cpu(), x.cpu()) and torch.equal(pm.cpu(), x_mean.cpu())


# ---- 8. the constructor -------------------------------------------------------------------------------------------------
def check_constructor():
    from score_sde_pytorch_amd import _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    for name, want in (("elu", L.ACT_ELU), ("ReLU", L.ACT_RELU), ("lrelu", L.ACT_LRELU), ("swish", L.ACT_SILU), ("Swish", L.ACT_SILU)):
        cfg = _util.small_config()
        cfg.model.nonlinearity = name
        assert mutils.get_model("ncsnpp")(cfg).act_kind == want
    cfg = _util.small_config()
    cfg.model.nonlinearity = "gelu"
    msg = pytest_raises(NotImplementedError, lambda: mutils.get_model("ncsnpp")(cfg))
    assert msg == "activation function does not exist!"
    cfg.model.nonlinearity = "elu"
    model = mutils.get_model("ncsnpp")(cfg)
    msg = pytest_raises(RuntimeError, lambda: model(torch.zeros(1, 3, 16, 16), torch.ones(1)))
    assert "no CPU fallback" in msg
