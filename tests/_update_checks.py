"""Checks of the kernels that run between U-Net evaluations -- the sampler, ODE, loss-head and optimizer launches of
csrc/elementwise.hip and of the loss / optimizer part of csrc/backward.hip -- against fp64, shared by the emulator suite
(tests/test_update_cpu.py) and the GPU suite (tests/test_update_gpu.py).  `dev` is "cpu" (the caller holds emu.emulated())
or "cuda".  Kernels are driven through hipops where a wrapper exists, through the ctypes mirrors of _lib.py otherwise.

Every reference is computed on the CPU in fp64 from the fp32 inputs the kernel receives.  u = 2^-24.  Bounds are first order
in u, times HIGHER_ORDER = 1 + 2^-10 for the terms that leaves out, and none is tuned.  A ratio close to 1 is what a bound made
of a single rounding gives (half an ulp of the stored value is u times it); no ratio can pass 1 for a correct kernel:

(a) Elementwise kernels written with ssde_fmul_rn / ssde_fadd_rn / ssde_fdiv_rn (predictor, sample_update, project's elementwise form,
    perturb, pf_drift, to_nhwc, to_nchw, fused_bias_act): torch.equal with the fp32 torch expression in the reference's operation
    order, and |result - fp64 expression| <= k u sum|terms| per element, k = the roundings of the kernel as written (counted
    beside each check).  axpy is not written with _rn operations (hipcc may fuse its `dst + alpha x`): the fp64 bound only, and
    only without a gate -- the gated form multiplies by ssde_silu_grad, whose __expf / rcp approximations have no derived bound.
(b) fp32 block reductions of non-negative terms (sumsq, sumsq_flat, dsm_loss' per-sample loss, the two batch means of langevin):
        relative error <= (serial terms per thread + tree depth + 2) u             (red_rel below)
    serial = ceil(m / 256) for a sum of length m by one 256-thread block; tree depth = 8 (six wave shuffles, two levels over the
    four waves); the + 2 covers the rounding of a term and the one operation after the sum (a division by n or per, a sqrt).
    sumsq_flat: serial = 4 ceil(ceil(numel / 4) / (256 blocks)) + 3 with blocks = min(1024, ceil(numel / 1024)) -- every trip of
    the stride blocks * 256 adds four squares, thread 0 of block 0 up to three tail elements --, and its tree is two blocks
    deep: 8 + ceil(blocks / 256) + 8 (the partials' tree, the serial part and the tree of the final kernel).
    The dsm_loss batch mean and dscore follow the same way (check_dsm_loss).
(c) fp64 sums (hutch_div, rk_error_norm): against math.fsum over the same terms, |error| <= m 2^-53 sum|t| for a sum of
    length m.  hutch_div's terms are the fp32 products, restated in the kernel's fp32 order and widened.  rk_error_norm's
    terms are fp64 expressions which hipcc may fuse differently from the CPU, so their own roundings are added (check_rk_error).
    rk_combine: (2 terms + 1) 2^-53 (|y| + sum|c_j K_j|).
(d) langevin, project's colour form, Adam: per-element bounds from the operation count, derived beside each check.  Adam is
    compared UPDATE against update (p_new - p_old, m, v, ema_new - ema_old against the fp64 step from the same fp32 state), so
    the bound is relative to the update and not to max|p|.  No flat tolerance is used anywhere.

Shapes: per-sample sizes PERS x batches BATCHES, every pair; per 1..257 sit around the wave and block size, 969 = 3 * 17 * 19 and
1000 are no multiple of anything; n = 257 and 300 make the strided loops over the batch (langevin's means, mean_kernel) take a
second trip.  One "large" case per kernel (GPU only) crosses the kernel's block cap, so the grid-stride loop takes a second,
ragged pass: LARGE = 4096 * 256 + 3 * 256 + 5 elements (pixels for to_nhwc and project's colour form), ADAM_LARGE for Adam's cap
of 8192 blocks, FLAT_LARGE (% 4 == 3) for the cap of 1024 blocks of sumsq_flat and randn, 262144 + 261 / 131072 + 261 for the
single / pair form of rk_error_norm.

randn: rocRAND's Philox on the GPU, the emulator's stand-in on the CPU -- no value is compared, only reproducibility, the
seed word, finiteness of every size, and moments / correlations inside 5 sigma of their estimators (computed from N).  Seeds
are fixed: on the emulator every statistic of the chosen seeds sits inside its bound (largest |z| / 5 below).

Largest error / bound seen (every check prints its own):
                                       emulator (exact fp32)   MI355X (both matrix modes)
  sumsq                                0.25                    0.25
  langevin      x_mean / x             1.00 / 0.98             1.00 / 0.98      (0.997: |step g| << |x|, the bound is the last rounding)
  predictor     x_mean / x             0.58 / 0.53             0.64 / 0.53
  sample_update x_mean / x_out         0.66 / 0.51             0.66 / 0.53
  project       x / x_mean             0.33 / 0.36             0.38 / 0.36
  project, colour form  x / x_mean     0.35 / 0.33             0.51 / 0.41
  perturb / pf_drift                   0.65 / 0.41             0.65 / 0.49
  to_nhwc / to_nchw                    0.57 / 0.61             0.57 / 0.78
  fused_bias_act  forward / gradient   0.52 / 0.54             0.57 / 0.57
  hutch_div                            0.00 (exact)            0.00 (exact)
  rk_combine / rk_error_norm           0.00 / 0.07             0.20 / 0.07
  dsm_loss  losses / loss / dscore     0.17 / 0.04 / 0.92      0.17 / 0.04 / 0.92
  sumsq_flat                           0.06                    0.06
  adam  p / m / v / ema                0.98 / 0.97 / 0.85 / 0.93   0.98 / 0.97 / 0.62 / 0.98
  axpy                                 0.82                    0.96
  randn  largest |z| / 5               0.34                    0.50
The MI355X column holds the large cases too; where it differs from the emulator's, hipcc fused a product into a sum (Adam,
axpy, the reductions, rk_combine) or the case is a large one.  torch.equal holds for every kernel of (a) on both.

What the cases found, and what was fixed:
  * test_predictor_update[True] (numel = 1, no step word) on the MI355X: x_mean one ulp off the torch expression, 2.4e-7 at
    -3.67.  hipcc's __fmul_rn / __fadd_rn are a plain `*` / `+`, which its default -ffp-contract=fast fused after inlining
    (v_mul + 2 v_fmac in predictor_kernel's ISA), so none of the "_rn" kernels -- predictor, langevin, sample_update, project,
    project_prepare, perturb, pf_drift, hutch_div, dsm_loss' residual, to_nhwc -- kept the reference's operation order
    wherever a product was inexact.  The older bit-for-bit tests multiply by 0 / 1 masks or by 2, where fusing changes nothing.
    Fixed by ssde_fmul_rn / ssde_fadd_rn / ssde_fsub_rn / ssde_fdiv_rn (ssde_common.h), compiled under contract(off).
    The emulator is built without contraction and never saw it.
  * ssde_sumsq_flat and ssde_randn took a pointer that is not 16-byte aligned and read / wrote it as float4: now refused.
No case found a kernel's arithmetic or indexing wrong beyond that.
"""
import ctypes as C
import itertools
import math

import torch

from score_sde_pytorch_amd import _lib as L

U = 2.0 ** -24
U64 = 2.0 ** -53
HIGHER_ORDER = 1 + 2.0 ** -10          # the bounds are first order in u: the neglected terms are below k u of a bound of k roundings, k u < 2^-10 here
PERS = (1, 3, 63, 64, 65, 255, 256, 257, 969, 1000)
BATCHES = (1, 3, 257, 300)
SHAPES = tuple(itertools.product(BATCHES, PERS))
LARGE = 4096 * 256 + 3 * 256 + 5
ADAM_LARGE = 8192 * 256 + 3 * 256 + 5
FLAT_LARGE = 1024 * 1024 + 1027
assert LARGE % 3 == 0 and FLAT_LARGE % 4 == 3
NUMELS = (1, 3, 255, 257, 1000)                                              # kernels over a flat range
STEPS = (None, 0, 1, 4)                                                      # no step word, first, second and last row of a 5-row table
FEW_SHAPES = ((3, 1), (3, 65), (3, 257), (3, 1000))
LANGEVIN_MODES = ((False, None), (True, None), (True, 0), (True, 3))         # (alpha_tab, step word)
PROJECT_SHAPES = ((1, 1, 1), (3, 3, 25), (3, 3, 64), (2, 4, 257))
COLOUR_HW = (1, 25, 64, 257)
N32_MODES = (None, 0, 100)                                                   # no fp32 copy, all of it, its first elements
DSM_SHAPES = ((300, 257), (3, 1000), (4, 192), (1, 1))
DSM_MODES = ((1.0, True), (0.125, True), (1.0, False))                       # (grad_scale, want_grad)
FLAT_NUMELS = (1, 2, 3, 4, 5, 7, 1003)
NCHW_MODES = ((1.0, False), (0.7, False), (1.0, True), (0.7, True))          # (alpha, accumulate)
ADAM_NUMELS = (1, 5, 1003)
ADAM_CASES = {"clipped": dict(clip=0.01, g_scale=3.0), "unclipped": dict(clip=1.0, g_scale=1e-4),
              "clip_off": dict(clip=-1.0, g_scale=3.0), "no_norm": dict(clip=1.0, g_scale=3.0, use_gnorm=False)}
WORST = {}


# ---- plumbing -----------------------------------------------------------------------------------------------------------
def _ops():
    from score_sde_pytorch_amd import hipops
    return hipops


def _stream(dev):
    return None if dev == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(entry, args, dev):
    L.check(getattr(L.load(), entry)(C.byref(args), _stream(dev)), entry)


def refused(entry, args, dev, *words):
    lib = L.load()
    rc = getattr(lib, entry)(C.byref(args), _stream(dev))
    msg = lib.ssde_last_error() or b""
    assert rc != 0 and all(w.encode() in msg for w in words), (entry, rc, msg, words)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def put(t, dev):
    """a device copy the kernel may write (on the emulator .to() would hand back the input itself)"""
    return t.clone().to(dev)


def p(t):
    return None if t is None else t.data_ptr()


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def i32(v, dev):
    return torch.tensor([v], dtype=torch.int32).to(dev)


def red_rel(m, serial=None, depth=8):
    """bound (b) of the module docstring"""
    return ((serial if serial is not None else -(-m // 256)) + depth + 2) * U


def within(name, got, ref, bound):
    """|got - ref| <= bound everywhere (fp64); records and returns the worst error / bound"""
    got, ref, bound = got.detach().cpu().double().reshape(-1), ref.double().reshape(-1), bound.double().reshape(-1)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()), name
    err = (got - ref).abs()
    bound = bound * HIGHER_ORDER
    exact = bound == 0
    assert bool((err[exact] == 0).all()), (name, "an exact element differs")
    ratio = float((err[~exact] / bound[~exact]).max()) if bool((~exact).any()) else 0.0
    WORST[name.split()[0]] = max(WORST.get(name.split()[0], 0.0), ratio)
    print("%s: worst |err| / bound %.3f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)
    return ratio


def same(name, got, ref):
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and torch.equal(got, ref), (name, float((got.double() - ref.double()).abs().max()))


# ---- per-sample sum of squares --------------------------------------------------------------------------------------------
def run_sumsq(a, b, dev):
    n, per = a.shape
    oa, ob = torch.full((n,), float("nan")).to(dev), torch.full((n,), float("nan")).to(dev)
    args = L.SumsqArgs()
    args.a, args.b, args.out_a, args.out_b, args.n, args.per = p(a), p(b), p(oa), p(ob) if b is not None else None, n, per
    launch("ssde_sumsq", args, dev)
    sync(dev)
    return oa, ob


def check_sumsq(dev, n, per, seed=1):
    """out[n] = sum(a[n, :]^2), with and without the second tensor; returns the device tensors and the checked sums"""
    g = gen(seed + 7 * n + per)
    a, b = torch.randn(n, per, generator=g) * 3, torch.randn(n, per, generator=g)
    da, db = put(a, dev), put(b, dev)
    oa, ob = run_sumsq(da, db, dev)
    ra, rb = a.double().square().sum(1), b.double().square().sum(1)
    within("sumsq a n=%d per=%d" % (n, per), oa, ra, red_rel(per) * ra)
    within("sumsq b n=%d per=%d" % (n, per), ob, rb, red_rel(per) * rb)
    oa1, ob1 = run_sumsq(da, None, dev)
    assert torch.equal(oa1, oa) and bool(torch.isnan(ob1).all())          # out_b is not written without b
    return (a, b), (da, db), (oa, ob)


# ---- Langevin corrector update --------------------------------------------------------------------------------------------
def check_langevin(dev, n, per, alpha_tab, step, snr=0.16):
    """x_mean = x + step g ; x = x_mean + sqrt(2 step) z with step = (snr mean||z|| / mean||g||)^2 2 alpha, gss / zss from ssde_sumsq
    on the same tensors (checked against fp64 by check_sumsq on the way).

    Bound, e_m = red_rel(n) for each of the two batch means (n sqrtf's summed by one block, divided by n):
      r = snr zn / gn        : 2 e_m + 2u        step = r r 2 alpha : rel_s = 2 (2 e_m + 2u) + 2u        nz = sqrtf(2 step) : rel_s / 2 + u
      x_mean = x + step g    : (rel_s + u) |step g| + u |x_mean|
      x = x_mean + nz z      : the above + (rel_s / 2 + 2u) |nz z| + u |x|"""
    (g_, z_), (dg, dz), (gss, zss) = check_sumsq(dev, n, per, seed=3)
    x = torch.randn(n, per, generator=gen(5 + n + per)) * 20
    dx, dxm = put(x, dev), torch.full((n, per), float("nan")).to(dev)
    tab = torch.tensor([0.7, 1.3, 0.25, 2.0, 0.9])
    dtab, dstep = (tab.to(dev) if alpha_tab else None), (i32(step, dev) if step is not None else None)
    args = L.LangevinArgs()
    args.x, args.x_mean, args.grad, args.noise, args.grad_sumsq, args.noise_sumsq = p(dx), p(dxm), p(dg), p(dz), p(gss), p(zss)
    args.alpha_tab, args.step_ptr, args.n, args.per, args.snr = p(dtab), p(dstep), n, per, snr
    launch("ssde_langevin_update", args, dev)
    sync(dev)
    alpha = float(tab[step or 0]) if alpha_tab else 1.0
    snr64 = float(torch.tensor(snr, dtype=torch.float32))
    gn, zn = gss.cpu().double().sqrt().mean(), zss.cpu().double().sqrt().mean()
    st = (snr64 * zn / gn) ** 2 * 2 * alpha
    nz = torch.sqrt(st * 2)
    xm64 = x.double() + st * g_.double()
    x64 = xm64 + nz * z_.double()
    e_m = red_rel(n)
    rel_s = 2 * (2 * e_m + 2 * U) + 2 * U
    b_xm = (rel_s + U) * (st * g_.double()).abs() + U * xm64.abs()
    b_x = b_xm + (rel_s / 2 + 2 * U) * (nz * z_.double()).abs() + U * x64.abs()
    tag = "n=%d per=%d alpha_tab=%d step=%s" % (n, per, alpha_tab, step)
    within("langevin x_mean " + tag, dxm, xm64, b_xm)
    within("langevin x " + tag, dx, x64, b_x)


# ---- predictor update -------------------------------------------------------------------------------------------------------
PRED_COEF = torch.tensor([[1.0, 0.37, 0.61], [0.9875, 1.9, 1.4], [1.0, 0.011, 0.105], [0.5, 7.0, 2.6], [0.93, 0.0041, 0.064]])


def run_predictor(dev, dx, dxm, ds, dz, dcoef, dstep):
    args = L.PredictorArgs()
    args.x, args.x_mean, args.score, args.noise, args.coef, args.step_ptr, args.numel = p(dx), p(dxm), p(ds), p(dz), p(dcoef), p(dstep), dx.numel()
    launch("ssde_predictor_update", args, dev)


def predictor_ref(x, s, z, row):
    """(x_mean, x) in the kernel's order, in the dtype of the inputs; the sums of |terms| for the fp64 bound (3 and 5 roundings)"""
    a, b, c = (row[k].to(x.dtype) for k in range(3))
    xa = x if float(a) == 1.0 else a * x
    xm = xa + b * s
    xo = xm + c * z if z is not None else xm
    t_xm = (a * x).abs() + (b * s).abs()
    return xm, xo, t_xm, t_xm + ((c * z).abs() if z is not None else 0)


def check_predictor(dev, numel, step, with_z, seed=11):
    g = gen(seed + numel)
    x, s, z = torch.randn(numel, generator=g) * 10, torch.randn(numel, generator=g) * 3, torch.randn(numel, generator=g)
    dx, dxm = put(x, dev), torch.full((numel,), float("nan")).to(dev)
    run_predictor(dev, dx, dxm, s.to(dev), z.to(dev) if with_z else None, PRED_COEF.to(dev), i32(step, dev) if step is not None else None)
    sync(dev)
    row = PRED_COEF[step or 0]
    zz = z if with_z else None
    xm32, xo32, _, _ = predictor_ref(x, s, zz, row)
    same("predictor x_mean", dxm, xm32)
    same("predictor x", dx, xo32)
    xm64, xo64, t_xm, t_x = predictor_ref(x.double(), s.double(), None if zz is None else zz.double(), row)
    tag = "numel=%d step=%s z=%d" % (numel, step, with_z)
    within("predictor x_mean " + tag, dxm, xm64, 3 * U * t_xm)
    within("predictor x " + tag, dx, xo64, 5 * U * t_x)


# ---- per-sample update (hipops.sample_update) ----------------------------------------------------------------------------------
def check_sample_update(dev, n, per, use_a, use_y, use_z, seed=17):
    """x_mean = a[n] x + b[n] y ; x_out = x_mean + c[n] z: a product, a product, a sum (3 roundings), a product and a sum more (5)"""
    g = gen(seed + n + per)
    x, y, z = torch.randn(n, per, generator=g) * 10, torch.randn(n, per, generator=g) * 3, torch.randn(n, per, generator=g)
    a, b, c = (torch.rand(n, generator=g) + 0.25 + k for k in range(3))         # distinct per sample and per vector
    d = lambda t, use: t.to(dev) if use else None                             # noqa: E731
    xo, xm = _ops().sample_update(x.to(dev), y=d(y, use_y), b=d(b, use_y), z=d(z, use_z), c=d(c, use_z), a=d(a, use_a))
    sync(dev)

    def ref(x, y, z, a, b, c):
        xm = a[:, None] * x if use_a else x
        t = xm.abs()
        if use_y:
            xm = xm + b[:, None] * y
            t = t + (b[:, None] * y).abs()
        xo = xm + c[:, None] * z if use_z else xm
        return xm, xo, t, (t + (c[:, None] * z).abs()) if use_z else t
    xm32, xo32, _, _ = ref(x, y, z, a, b, c)
    same("sample_update x_mean", xm, xm32)
    same("sample_update x_out", xo, xo32)
    xm64, xo64, t_xm, t_x = ref(*(v.double() for v in (x, y, z, a, b, c)))
    tag = "n=%d per=%d a=%d y=%d z=%d" % (n, per, use_a, use_y, use_z)
    within("sample_update x_mean " + tag, xm, xm64, 3 * U * t_xm)
    within("sample_update x_out " + tag, xo, xo64, 5 * U * t_x)


# ---- controllable-generation projection -------------------------------------------------------------------------------------
PROJ_COEF = torch.tensor([[1.0, 0.8], [0.91, 2.5], [0.45, 11.0], [1.0, 0.02], [0.07, 37.0]])


def project_inputs(n, c, hw, seed):
    g = gen(seed)
    x, data, z = torch.randn(n, c, hw, generator=g) * 10, torch.rand(n, c, hw, generator=g), torch.randn(n, c, hw, generator=g)
    mask = torch.tensor([0.0, 1.0, 0.25, 0.6])[torch.randint(0, 4, (n, c, hw), generator=g)]
    return x, data, z, mask


def run_project(dev, x, data, z, mask, step, M=None, invM=None):
    n, c, hw = x.shape
    dx, dxm = put(x, dev), torch.full(x.shape, float("nan")).to(dev)
    keep = [data.to(dev), mask.to(dev), z.to(dev), PROJ_COEF.to(dev), i32(step, dev) if step is not None else None]
    args = L.ProjectArgs()
    args.x, args.x_mean, args.data, args.mask, args.noise, args.coef, args.step_ptr = (p(t) for t in [dx, dxm] + keep)
    args.n, args.c, args.hw, args.use_matrix = n, c, hw, int(M is not None)
    if M is not None:
        args.M, args.invM = (C.c_float * 9)(*M), (C.c_float * 9)(*invM)
    launch("ssde_project_update", args, dev)
    sync(dev)
    return dx, dxm


def check_project(dev, n, c, hw, step, seed=23):
    """elementwise form.  x: 1 - mask, m data, z s, their sum, x inv, known mask, their sum = 7 roundings; x_mean: 3 more"""
    x, data, z, mask = project_inputs(n, c, hw, seed + hw + n)
    dx, dxm = run_project(dev, x, data, z, mask, step)
    row = PROJ_COEF[step or 0]

    def ref(x, data, z, mk):
        m, s = row[0].to(x.dtype), row[1].to(x.dtype)
        inv = 1.0 - mk
        mean = data if float(m) == 1.0 else m * data
        known = mean + z * s
        xn = x * inv + known * mk
        xm = xn * inv + mean * mk
        t_x = (x * inv).abs() + (mean * mk).abs() + (z * s * mk).abs()
        return xn, xm, t_x, t_x * inv.abs() + (mean * mk).abs()
    xn32, xm32, _, _ = ref(x, data, z, mask)
    same("project x", dx, xn32)
    same("project x_mean", dxm, xm32)
    known = mask == 1
    assert bool(known.any()) or x.numel() < 8
    m32 = PROJ_COEF[step or 0, 0]
    assert torch.equal(dxm.cpu()[known], (data if float(m32) == 1.0 else m32 * data)[known])      # known pixels come back as m data
    xn64, xm64, t_x, t_xm = ref(*(v.double() for v in (x, data, z, mask)))
    tag = "n=%d c=%d hw=%d step=%s" % (n, c, hw, step)
    within("project x " + tag, dx, xn64, 7 * U * t_x)
    within("project x_mean " + tag, dxm, xm64, 10 * U * t_xm)


def check_project_colour(dev, n, hw, step, own_mask, seed=29):
    """colour form, the colorizer's M / invM.  One mat3_apply has forward error <= 4u |v|^T |A| (gamma_3, as in
    _plan_control_checks.check_prepare_colour); with inv = fl(1 - mask), e_mean = u |m data| (0 for m == 1):
      y = M x              e_y   = 4u |x|^T |M|
      known = mean + z s   e_kn  = e_mean + u |z s| + u |known|
      yn = y inv + known mask          e_yn = e_y |inv| + 2u |y inv| + e_kn mask + u |known mask| + u |yn|
      xn = invM yn         e_xn  = 4u |yn|^T |invM| + e_yn^T |invM|
      y2 = M xn            e_y2  = 4u |xn|^T |M| + e_xn^T |M|
      ym = y2 inv + mean mask          e_ym = e_y2 |inv| + 2u |y2 inv| + e_mean mask + u |mean mask| + u |ym|
      x_mean = invM ym     e_xm  = 4u |ym|^T |invM| + e_ym^T |invM|"""
    import _plan_control_checks as P
    M, invM = P.matrices()
    x, data, z, mask = project_inputs(n, 3, hw, seed + hw + n)
    if own_mask:
        mask = torch.cat([torch.ones(n, 1, hw), torch.zeros(n, 2, hw)], dim=1)
    dx, dxm = run_project(dev, x, data, z, mask, step, M, invM)
    M64, I64 = (torch.tensor(v, dtype=torch.float32).double().view(3, 3) for v in (M, invM))
    ap = lambda v, A: torch.einsum('bih,ij->bjh', v, A)                        # noqa: E731
    m, s = (float(v) for v in PROJ_COEF[step or 0])
    x_, d_, z_, mk = (v.double() for v in (x, data, z, mask))
    inv = 1.0 - mk
    mean = m * d_
    e_mean = U * mean.abs() if m != 1.0 else torch.zeros_like(mean)
    y = ap(x_, M64)
    e_y = 4 * U * ap(x_.abs(), M64.abs())
    known = mean + z_ * s
    e_kn = e_mean + U * (z_ * s).abs() + U * known.abs()
    yn = y * inv + known * mk
    e_yn = e_y * inv.abs() + 2 * U * (y * inv).abs() + e_kn * mk + U * (known * mk).abs() + U * yn.abs()
    xn = ap(yn, I64)
    e_xn = 4 * U * ap(yn.abs(), I64.abs()) + ap(e_yn, I64.abs())
    y2 = ap(xn, M64)
    e_y2 = 4 * U * ap(xn.abs(), M64.abs()) + ap(e_xn, M64.abs())
    ym = y2 * inv + mean * mk
    e_ym = e_y2 * inv.abs() + 2 * U * (y2 * inv).abs() + e_mean * mk + U * (mean * mk).abs() + U * ym.abs()
    xm = ap(ym, I64)
    e_xm = 4 * U * ap(ym.abs(), I64.abs()) + ap(e_ym, I64.abs())
    tag = "n=%d hw=%d step=%s own_mask=%d" % (n, hw, step, own_mask)
    within("project_colour x " + tag, dx, xn, e_xn)
    within("project_colour x_mean " + tag, dxm, xm, e_xm)


# ---- perturb ----------------------------------------------------------------------------------------------------------------
def check_perturb(dev, n, per, use_a, seed=31):
    """dst = a[n] x + s[n] z: two products and a sum (3 roundings)"""
    g = gen(seed + n + per)
    x, z = torch.randn(n, per, generator=g), torch.randn(n, per, generator=g)
    a, s = torch.rand(n, generator=g) + 0.1, torch.rand(n, generator=g) * 40 + 0.01
    out = _ops().perturb(x.to(dev), z.to(dev), s.to(dev), a_coef=a.to(dev) if use_a else None)
    sync(dev)
    ref = lambda x, z, a, s: ((a[:, None] * x) if use_a else x) + s[:, None] * z      # noqa: E731
    same("perturb", out, ref(x, z, a, s))
    x_, z_, a_, s_ = (v.double() for v in (x, z, a, s))
    terms = ((a_[:, None] * x_) if use_a else x_).abs() + (s_[:, None] * z_).abs()
    within("perturb n=%d per=%d a=%d" % (n, per, use_a), out, ref(x_, z_, a_, s_), 3 * U * terms)


# ---- probability-flow drift and Hutchinson divergence ------------------------------------------------------------------------
SENTINEL = -12345.5


def dyn_record(dev, a, g2, dst_ptr):
    rec = L.OdeDyn()
    rec.label, rec.std, rec.a, rec.g2, rec.dst = 0.25, 0.5, a, g2, dst_ptr
    return torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8).clone().to(dev)


def check_pf_drift(dev, numel, use_dyn, seed=37):
    """dst = (double)(a x - (g2 score) 0.5): a x, g2 score, the halving, the difference = 4 roundings; the slots before and after
    dst keep their sentinel"""
    g = gen(seed + numel)
    x, s = torch.randn(numel, generator=g) * 5, torch.randn(numel, generator=g) * 30
    a, g2 = torch.tensor(-0.5 * 7.3, dtype=torch.float32), torch.tensor(3.7, dtype=torch.float32) ** 2
    pad = 5
    buf = torch.full((numel + 2 * pad,), SENTINEL, dtype=torch.float64).to(dev)
    dst_ptr = buf.data_ptr() + 8 * pad
    dx, ds = x.to(dev), s.to(dev)
    args = L.PfDriftArgs()
    args.x, args.score, args.numel = p(dx), p(ds), numel
    if use_dyn:
        rec = dyn_record(dev, float(a), float(g2), dst_ptr)
        args.dst, args.a, args.g2, args.dyn = None, 99.0, -99.0, p(rec)          # the immediates must not be read
    else:
        args.dst, args.a, args.g2 = dst_ptr, float(a), float(g2)
    launch("ssde_pf_drift", args, dev)
    sync(dev)
    buf = buf.cpu()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all())
    out = buf[pad:-pad]
    same("pf_drift", out, (a * x - g2 * s * 0.5).double())
    a_, g_ = float(a), float(g2)
    within("pf_drift numel=%d dyn=%d" % (numel, use_dyn), out, a_ * x.double() - g_ * s.double() * 0.5,
           4 * U * ((a_ * x.double()).abs() + (g_ * s.double() * 0.5).abs()))


def check_hutch_div(dev, n, per, use_dyn, dst_off, seed=41):
    """dst[dst_off + b] = sum_i ((a eps_i - (g2 gx_i) 0.5) eps_i): fp32 terms in the kernel's order, summed in fp64"""
    g = gen(seed + n + per)
    gx, eps = torch.randn(n, per, generator=g) * 30, torch.randn(n, per, generator=g)
    a, g2 = torch.tensor(-0.5 * 7.3, dtype=torch.float32), torch.tensor(3.7, dtype=torch.float32) ** 2
    pad = 3
    buf = torch.full((dst_off + n + 2 * pad,), SENTINEL, dtype=torch.float64).to(dev)
    dst_ptr = buf.data_ptr() + 8 * pad
    dgx, deps = gx.to(dev), eps.to(dev)
    args = L.HutchDivArgs()
    args.gx, args.eps, args.dst_off, args.n, args.per = p(dgx), p(deps), dst_off, n, per
    if use_dyn:
        rec = dyn_record(dev, float(a), float(g2), dst_ptr)
        args.dst, args.a, args.g2, args.dyn = None, 99.0, -99.0, p(rec)
    else:
        args.dst, args.a, args.g2 = dst_ptr, float(a), float(g2)
    launch("ssde_hutch_div", args, dev)
    sync(dev)
    buf = buf.cpu()
    assert bool((buf[:pad + dst_off] == SENTINEL).all()) and bool((buf[pad + dst_off + n:] == SENTINEL).all())
    t = ((a * eps - g2 * gx * 0.5) * eps).double()                              # fp32, then widened
    ref = torch.tensor([math.fsum(r) for r in t.tolist()], dtype=torch.float64)
    within("hutch_div n=%d per=%d dyn=%d off=%d" % (n, per, use_dyn, dst_off), buf[pad + dst_off: pad + dst_off + n], ref,
           per * U64 * t.abs().sum(1))


# ---- Runge-Kutta stage arithmetic ----------------------------------------------------------------------------------------------
RK_COEF = {0: [], 1: [0.2], 7: [0.3, 0.0, -1.7, 0.025, 0.0, 4.1, -0.6],
           12: [0.05, 0.0, 0.0, 0.3, -0.2, 0.0, 1.1, -0.9, 0.0, 0.4, 0.0, 0.7]}


def check_rk_combine(dev, n, terms, n32, rows=13, seed=43):
    """dst = y + sum_j coef[j] K[j] over the rows with a non-zero coefficient (every other row is NaN: reading one fails), and
    its fp32 copy on the first n32 elements (n32 = 0: all of them; None: no copy).  2 terms + 1 fp64 roundings."""
    g = gen(seed + n + terms)
    coef = RK_COEF[terms][:min(terms, 12)]
    y = torch.randn(n, generator=g, dtype=torch.float64)
    K = torch.randn(rows, n, generator=g, dtype=torch.float64) * 3
    for j in range(rows):
        if j >= len(coef) or coef[j] == 0.0:
            K[j] = float("nan")
    dy, dK = y.to(dev), K.to(dev)
    dst = torch.full((n,), float("nan"), dtype=torch.float64).to(dev)
    d32 = torch.full((n,), SENTINEL).to(dev) if n32 is not None else None
    args = L.RkCombineRowsArgs()
    args.y, args.k, args.n, args.terms, args.dst, args.dst32, args.n32 = p(dy), p(dK), n, terms, p(dst), p(d32), n32 or 0
    for j, cj in enumerate(coef):
        args.coef[j] = cj
    launch("ssde_rk_combine_rows", args, dev)
    sync(dev)
    mag = y.abs()
    dy_ = torch.zeros_like(y)
    for j, cj in enumerate(coef):
        if cj != 0.0:
            dy_ = dy_ + K[j] * cj
            mag = mag + (K[j] * cj).abs()
    ref = y + dy_
    live = sum(1 for cj in coef if cj != 0.0)
    within("rk_combine n=%d terms=%d n32=%s" % (n, terms, n32), dst, ref, (2 * live + 1) * U64 * mag)
    if d32 is not None:
        m = n32 or n
        d32 = d32.cpu()
        assert torch.equal(d32[:m], dst.cpu()[:m].float()) and bool((d32[m:] == SENTINEL).all())


def rk_error_args(dev, y, y_new, K, coef, coef2, h_abs, atol, rtol, partial_len=1024):
    keep = [y.to(dev), y_new.to(dev), K.to(dev), torch.full((1024,), float("nan"), dtype=torch.float64).to(dev),
            torch.full((1,), float("nan"), dtype=torch.float64).to(dev)]
    args = L.RkErrorRowsArgs()
    args.y, args.y_new, args.k, args.partial, args.out = (p(t) for t in keep)
    args.n, args.rows, args.pair, args.h_abs, args.atol, args.rtol, args.partial_len = y.numel(), len(coef), int(coef2 is not None), h_abs, atol, rtol, partial_len
    for j, cj in enumerate(coef):
        args.coef[j] = cj
        args.coef2[j] = coef2[j] if coef2 is not None else 0.0
    return args, keep


def check_rk_error(dev, n, pair, h_abs=0.37, zero=False, seed=47):
    """single form: scipy's rms_norm(sum_j E_j h K_j / scale), scale = atol + max(|y|, |y_new|) rtol.  Pair form: scipy's
    DOP853._estimate_error_norm, err5 = K^T E5 / scale, err3 = K^T E3 / scale, |h| s5 / sqrt((s5 + 0.01 s3) n) and 0 when both are 0.

    Bound on a sum s = sum_i q_i^2, q_i = e_i / scale_i: the summation n 2^-53 s (c), plus the terms' own roundings, which the
    CPU and hipcc (fused multiply-adds) need not share: e_i is a dot product of `rows` terms, |d e_i| <= rows 2^-53 sum_j |c_j K_ji| (twice: the reference's own too);
    scale_i has 2 roundings, the quotient and the square one each: |d (q_i^2)| <= 2 |q_i| |d e_i| / scale_i + 5 2^-53 q_i^2.
    The result takes a square root (single: half the relative error of s, plus the division and the root: + 2 2^-53) or
    s5 / sqrt(s5 + 0.01 s3) (pair: rel(s5) + max(rel(s5), rel(s3)) / 2 + 6 2^-53)."""
    g = gen(seed + n + pair)
    rows = 13 if pair else 7
    y, y_new = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    K = torch.randn(rows, n, generator=g, dtype=torch.float64) * (0.0 if zero else 1e-3)
    coef = [0.12, 0.0, -0.45, 0.3, 0.0, -0.2, 0.23, 0.0, 0.0, 0.31, -0.37, 0.06, -0.2][:rows]
    coef2 = [-0.2, 0.0, 0.0, 0.0, 0.0, 0.7, -0.4, 0.15, -0.25, 0.0, 0.0, 0.0, 0.0] if pair else None
    atol, rtol = 1e-5, 1e-5
    args, keep = rk_error_args(dev, y, y_new, K, coef, coef2, h_abs if pair else 0.0, atol, rtol)
    launch("ssde_rk_error_norm_rows", args, dev)
    sync(dev)
    out = keep[4].cpu()
    scale = atol + torch.maximum(y.abs(), y_new.abs()) * rtol

    def total(c):
        cv = torch.tensor(c, dtype=torch.float64)
        q = (K * cv[:, None]).sum(0) / scale
        de = 2 * rows * U64 * (K * cv[:, None]).abs().sum(0)                    # the kernel's dot product and this one
        s = math.fsum((q * q).tolist())
        b = n * U64 * s + float((2 * q.abs() * de / scale + 5 * U64 * q * q).sum())
        return s, (b / s if s > 0 else 0.0)
    s5, r5 = total(coef)
    tag = "n=%d pair=%d h=%g zero=%d" % (n, pair, h_abs, zero)
    if not pair:
        ref, rel = math.sqrt(s5 / n), r5 / 2 + 2 * U64
    else:
        s3, r3 = total(coef2)
        ref = 0.0 if (s5 == 0 and s3 == 0) else h_abs * s5 / math.sqrt((s5 + 0.01 * s3) * n)
        rel = r5 + max(r5, r3) / 2 + 6 * U64
    if zero or (pair and h_abs == 0):
        assert ref == 0.0
    within("rk_error_norm " + tag, out, torch.tensor([ref], dtype=torch.float64), torch.tensor([rel * abs(ref)], dtype=torch.float64))


def check_rk_error_refusals(dev):
    y = torch.zeros(300, dtype=torch.float64)
    K = torch.zeros(13, 300, dtype=torch.float64)
    one = [1.0] * 7
    args, keep = rk_error_args(dev, y, y, K, [], None, 0.0, 1e-5, 1e-5)
    refused("ssde_rk_error_norm_rows", args, dev, "rk_error_norm", "rows = 0")
    args, keep = rk_error_args(dev, y, y, K, one, None, 0.0, 1e-5, 1e-5, partial_len=1)          # 300 elements: two blocks
    refused("ssde_rk_error_norm_rows", args, dev, "rk_error_norm", "partial buffer needs 2")
    args, keep = rk_error_args(dev, y, y, K, one, one, 0.5, 1e-5, 1e-5, partial_len=3)           # pair form: two sums of two blocks
    refused("ssde_rk_error_norm_rows", args, dev, "rk_error_norm", "partial buffer needs 4")
    for h in (float("inf"), float("nan"), -1.0):
        args, keep = rk_error_args(dev, y, y, K, one, one, h, 1e-5, 1e-5)
        refused("ssde_rk_error_norm_rows", args, dev, "rk_error_norm", "finite |h|")
    args, keep = rk_error_args(dev, y, y, K, one, None, float("nan"), 1e-5, 1e-5)                # the single form does not read h_abs
    launch("ssde_rk_error_norm_rows", args, dev)
    sync(dev)
    assert float(keep[4].cpu()) == 0.0


# ---- DSM loss head -----------------------------------------------------------------------------------------------------------
def check_dsm_loss(dev, n, per, reduce_mean, lw, grad_scale=1.0, want_grad=True, seed=53):
    """losses[b] = w_b red sum_i r_i^2 (red = 1/2, or 1/per for reduce_mean), r = score + z / s (likelihood weighting, w = g2) or
    score s + z (w = 1); loss = mean_b losses; dscore = grad_scale d loss / d score, against fp64 autograd of that expression.

    Bounds: r takes two roundings, d r = u |first term| + u |r|.  t = sum r^2 is reduction (b) over terms that carry 2 |r| d r
    each; red and w add a rounding each: |d losses| <= w red ((red_rel(per) + 2u) t + sum 2 |r| d r).  The batch mean is
    reduction (b) again over n (its + 2 covers the division): red_rel(n) mean(losses) + mean(|d losses|).  dscore = r gfac with
    gfac = w red' [s] / n grad_scale, five roundings (2 / per, three products, a division) and the product itself:
    |d dscore| <= |gfac| d r + 6u |dscore|."""
    g = gen(seed + n + per)
    sc, z = torch.randn(n, per, generator=g), torch.randn(n, per, generator=g)
    s, g2 = torch.rand(n, generator=g) * 3 + 0.05, torch.rand(n, generator=g) * 9 + 0.5
    loss, losses, ds = _ops().dsm_loss(sc.to(dev), z.to(dev), s.to(dev), g2=g2.to(dev) if lw else None, reduce_mean=reduce_mean,
                                       likelihood_weighting=lw, want_grad=want_grad, grad_scale=grad_scale)
    sync(dev)
    assert (ds is not None) == want_grad
    sc64 = sc.double().requires_grad_()
    z64, s64, w = z.double(), s.double()[:, None], (g2.double() if lw else torch.ones(n, dtype=torch.float64))
    r = sc64 + z64 / s64 if lw else sc64 * s64 + z64
    first = (z64 / s64 if lw else sc64 * s64).detach().abs()
    t = (r * r).sum(1)
    red = 1.0 / per if reduce_mean else 0.5
    ls64 = w * red * t
    ls64.mean().backward()
    r = r.detach()
    dr = U * first + U * r.abs()
    b_ls = w * red * ((red_rel(per) + 2 * U) * t.detach() + (2 * r.abs() * dr).sum(1))
    tag = "n=%d per=%d mean=%d lw=%d gs=%g" % (n, per, reduce_mean, lw, grad_scale)
    within("dsm_loss losses " + tag, losses, ls64.detach(), b_ls)
    within("dsm_loss loss " + tag, loss, ls64.detach().mean().reshape(1), (red_rel(n) * ls64.detach().mean() + b_ls.mean()).reshape(1))
    if want_grad:
        gs32 = float(torch.tensor(grad_scale, dtype=torch.float32))
        ds64 = sc64.grad * gs32
        gfac = (w * (2 * red) * (1.0 if lw else s.double()) / n * gs32)[:, None]
        within("dsm_loss dscore " + tag, ds, ds64, gfac.abs() * dr + 6 * U * ds64.abs())


# ---- flat sum of squares --------------------------------------------------------------------------------------------------------
def flat_rel(numel):
    blocks = min(1024, max(1, -(-numel // 1024)))
    trips = -(-(-(-numel // 4)) // (256 * blocks))
    return red_rel(numel, serial=4 * trips + 3, depth=8 + -(-blocks // 256) + 8)


def check_sumsq_flat(dev, numel, seed=59):
    x = torch.randn(numel, generator=gen(seed + numel % 1000)) * 3
    out = _ops().sumsq_flat(x.to(dev))
    sync(dev)
    ref = x.double().square().sum().reshape(1)
    within("sumsq_flat numel=%d" % numel, out, ref, flat_rel(numel) * ref)


# ---- clip + Adam + EMA ----------------------------------------------------------------------------------------------------------
def adam_step64(p_, g_, m_, v_, ema_, hyper, gnorm_sq):
    """one step of adam_kernel in fp64 from its fp32 inputs; returns the new (p, m, v, ema) and their error bounds.  The kernel's
    lines, and the first-order error each adds (a hat marks the kernel's value, rel_c the relative error of coef):
      coef = min(1, clip / (sqrtf(gnorm_sq) + 1e-6))       (clip >= 0 and gnorm_sq given; else 1)    rel_c = 3u (root, sum, quotient)
      gi = g coef [+ wd p]                                  e_g = (rel_c + u) |g coef| [+ 2u |wd p| + u |gi|]
      mi = m + (gi - m) (1 - b1)                            e_m = (1 - b1) (e_g + u |gi - m|) + 2u |(gi - m)(1 - b1)| + u |mi|
      vi = v b2 + (1 - b2) gi gi                            e_v = u |v b2| + 3u (1 - b2) gi^2 + 2 (1 - b2) |gi| e_g + u |vi|
      denom = sqrtf(vi) / bc2s + eps                        e_d = (e_v / (2 vi) + 2u) sqrt(vi) / bc2s + u denom
      p -= (lr / bc1) (mi / denom)                          e_up = (lr / bc1) e_m / denom + |upd| (e_d / denom + 3u) ; e_p = e_up + u |p_new|
      ema = e - omd (e - p)                                 e_e = omd (e_p + u |e - p|) + u |omd (e - p)| + u |ema_new|
    1 - b1 and 1 - b2 are exact in fp32 for b1, b2 in [0.5, 1]."""
    h = [float(v) for v in hyper]
    lr, b1, b2, eps, wd, clip, bc1, bc2s, omd = h[:9]
    assert 0.5 <= b1 <= 1 and 0.5 <= b2 <= 1
    coef, rel_c = 1.0, 0.0
    if gnorm_sq is not None and clip >= 0:
        c = clip / (math.sqrt(float(gnorm_sq)) + float(torch.tensor(1e-6, dtype=torch.float32)))
        coef, rel_c = (c, 3 * U) if c < 1.0 else (1.0, 0.0)
    gi = g_ * coef
    e_g = (rel_c + U) * gi.abs() if coef != 1.0 else torch.zeros_like(gi)
    if wd != 0.0:
        gi = gi + wd * p_
        e_g = e_g + 2 * U * (wd * p_).abs() + U * gi.abs()
    mi = m_ + (gi - m_) * (1 - b1)
    e_m = (1 - b1) * (e_g + U * (gi - m_).abs()) + 2 * U * ((gi - m_) * (1 - b1)).abs() + U * mi.abs()
    vi = v_ * b2 + (1 - b2) * gi * gi
    e_v = U * (v_ * b2).abs() + 3 * U * (1 - b2) * gi * gi + 2 * (1 - b2) * gi.abs() * e_g + U * vi
    denom = vi.sqrt() / bc2s + eps
    e_d = (e_v / (2 * vi) + 2 * U) * vi.sqrt() / bc2s + U * denom
    upd = (lr / bc1) * (mi / denom)
    pn = p_ - upd
    e_up = (lr / bc1) * e_m / denom + upd.abs() * (e_d / denom + 3 * U)
    e_p = e_up + U * pn.abs()
    out = [pn, mi, vi, None]
    bounds = [e_p, e_m, e_v, None]
    if ema_ is not None:
        out[3] = ema_ - omd * (ema_ - pn)
        bounds[3] = omd * (e_p + U * (ema_ - pn).abs()) + U * (omd * (ema_ - pn)).abs() + U * out[3].abs()
    return out, bounds


def check_adam(dev, numel, clip, g_scale, wd, use_ema, use_gnorm=True, steps=3, seed=61):
    """three steps of ssde_adam_clip_ema; every step is compared with adam_step64 from the fp32 state the kernel started from:
    p_new - p_old, m, v and ema_new - ema_old, each within its own bound (a few u of the update, plus the half ulp of the
    stored value)."""
    ops = _ops()
    g = gen(seed + numel % 1000)
    P = torch.randn(numel, generator=g) * 0.05
    state = [put(P, dev), torch.zeros(numel).to(dev), torch.zeros(numel).to(dev), put(P, dev) if use_ema else None]
    tag = "numel=%d clip=%g g=%g wd=%g ema=%d gnorm=%d" % (numel, clip, g_scale, wd, use_ema, use_gnorm)
    for step in range(1, steps + 1):
        G = torch.randn(numel, generator=g) * g_scale
        dG = G.to(dev)
        decay = min(0.999, (1 + step) / (10 + step))
        hyper = torch.tensor([2e-4, 0.9, 0.999, 1e-8, wd, clip, 1 - 0.9 ** step, (1 - 0.999 ** step) ** 0.5, 1 - decay, 0, 0, 0])
        gn = ops.sumsq_flat(dG) if use_gnorm else None
        before = [None if t is None else t.cpu().double() for t in state]
        ops.adam_clip_ema(state[0], dG, state[1], state[2], state[3], hyper.to(dev), gn)
        sync(dev)
        gn_host = float(gn.cpu()) if gn is not None else None
        if gn_host is not None and clip >= 0:                                # the case is what it says: clipping active or not
            assert (gn_host ** 0.5 > 1.5 * clip) or (gn_host ** 0.5 < clip / 1.5), (gn_host, clip)
        ref, bounds = adam_step64(before[0], G.double(), before[1], before[2], before[3], hyper, gn_host)
        after = [None if t is None else t.cpu().double() for t in state]
        within("adam_p step %d %s" % (step, tag), after[0] - before[0], ref[0] - before[0], bounds[0])
        within("adam_m step %d %s" % (step, tag), after[1], ref[1], bounds[1])
        within("adam_v step %d %s" % (step, tag), after[2], ref[2], bounds[2])
        if use_ema:
            within("adam_ema step %d %s" % (step, tag), after[3] - before[3], ref[3] - before[3], bounds[3])


# ---- layout boundary and fused bias + activation ------------------------------------------------------------------------------
def check_to_nhwc(dev, n, c, h, w, c_pad, mode, a=2.0, b=-1.0, seed=67):
    """dst[n, y, x, ch] = f src[n, ch, y, x] + b, f = a, a / v[n] or -a / v[n]; padded channels 0.  3 roundings."""
    g = gen(seed + h * w + c_pad)
    x, v = torch.rand(n, c, h, w, generator=g), torch.rand(n, generator=g) + 0.5
    dx, dv = x.to(dev), v.to(dev)
    dst = torch.full((n, h, w, c_pad), float("nan")).to(dev)
    args = L.ToNhwcArgs()
    args.src, args.dst, args.n, args.c, args.h, args.w, args.c_pad, args.a, args.b, args.mode = p(dx), p(dst), n, c, h, w, c_pad, a, b, mode
    args.v = p(dv) if mode else None
    launch("ssde_to_nhwc", args, dev)
    sync(dev)
    a32 = torch.tensor(a, dtype=torch.float32)

    def ref(x, v):
        f = {0: a32.to(x.dtype).expand(n), 1: a32.to(x.dtype) / v, 2: -a32.to(x.dtype) / v}[mode]
        t = f[:, None, None, None] * x
        return (t + b).permute(0, 2, 3, 1), (t.abs() + abs(b)).permute(0, 2, 3, 1)
    out = dst.cpu()
    same("to_nhwc", out[..., :c].contiguous(), ref(x, v)[0].contiguous())
    assert c_pad == c or float(out[..., c:].abs().max()) == 0.0
    r64, t64 = ref(x.double(), v.double())
    within("to_nhwc n=%d %dx%d c_pad=%d mode=%d" % (n, h, w, c_pad, mode), out[..., :c], r64, 3 * U * t64)


def check_to_nchw(dev, n, c, h, w, c_src, mode, alpha, accumulate, seed=71):
    """dst[n, ch, y, x] (+)= alpha q, q = src[n, y, x, ch], src / v[n] or -src / v[n]: a quotient, a product, a sum = 3 roundings"""
    g = gen(seed + h * w + c_src)
    x, v = torch.randn(n, h, w, c_src, generator=g), torch.rand(n, generator=g) + 0.5
    old = torch.randn(n, c, h, w, generator=g) if accumulate else torch.full((n, c, h, w), float("nan"))
    dx, dv, dst = x.to(dev), v.to(dev), put(old, dev)
    args = L.ToNchwArgs()
    args.src, args.dst, args.n, args.c, args.h, args.w, args.c_src, args.mode = p(dx), p(dst), n, c, h, w, c_src, mode
    args.v, args.alpha, args.accumulate = p(dv) if mode else None, alpha, int(accumulate)
    launch("ssde_to_nchw", args, dev)
    sync(dev)
    al = torch.tensor(alpha, dtype=torch.float32)

    def ref(x, v, old):
        q = x[..., :c].permute(0, 3, 1, 2)
        if mode:
            q = (q if mode == 1 else -q) / v[:, None, None, None]
        if alpha != 1.0:
            q = al.to(x.dtype) * q
        return (old + q, old.abs() + q.abs()) if accumulate else (q, q.abs())
    same("to_nchw", dst, ref(x, v, old)[0].contiguous())
    r64, t64 = ref(x.double(), v.double(), old.double())
    within("to_nchw n=%d %dx%d c=%d/%d mode=%d alpha=%g acc=%d" % (n, h, w, c, c_src, mode, alpha, accumulate), dst, r64, 3 * U * t64)


def run_bias_act(dev, x, bias, channels, inner, act, alpha, scale, grad=0, ref=None, numel=None):
    dst = torch.full(x.shape, float("nan")).to(dev)
    keep = [x.to(dev), bias.to(dev) if bias is not None else None, ref.to(dev) if ref is not None else None]
    a = L.BiasActArgs()
    a.src, a.bias, a.dst, a.numel, a.channels, a.inner = p(keep[0]), p(keep[1]), p(dst), x.numel() if numel is None else numel, channels, inner
    a.act, a.alpha, a.scale, a.grad, a.ref = act, alpha, scale, grad, p(keep[2])
    launch("ssde_fused_bias_act", a, dev)
    sync(dev)
    return dst.cpu()


def check_bias_act(dev, shape, act, use_bias, alpha=0.2, scale=2 ** 0.5, seed=73):
    """forward: ((src + bias) slope) scale, slope = alpha where the sum is <= 0 (act 3); gradient mode: the slope is chosen by the
    sign of `ref`, the forward output of the same kernel with exact zeros put in.  A sum and two products = 3 roundings."""
    n, ch, hh, ww = shape
    g = gen(seed + n * ch * hh * ww + act)
    x, bias = torch.randn(shape, generator=g), (torch.randn(ch, generator=g) if use_bias else None)
    al, sc = torch.tensor(alpha, dtype=torch.float32), torch.tensor(scale, dtype=torch.float32)

    def fwd(x, bias, sign_of=None):
        u = x + bias.view(1, -1, 1, 1) if use_bias else x
        if act == 3:
            u = torch.where((u if sign_of is None else sign_of) > 0, u, u * al.to(x.dtype))
        return u * sc.to(x.dtype), ((x.abs() + bias.abs().view(1, -1, 1, 1)) if use_bias else x.abs()) * float(sc)
    out = run_bias_act(dev, x, bias, ch, hh * ww, act, alpha, scale)
    same("fused_bias_act", out, fwd(x, bias)[0])
    b64 = bias.double() if use_bias else None
    r64, t64 = fwd(x.double(), b64)
    tag = "%s act=%d bias=%d" % (shape, act, use_bias)
    within("fused_bias_act fwd " + tag, out, r64, 3 * U * t64)
    ref = out.clone()
    ref.view(-1)[::7] = 0.0                                                   # exact zeros take the alpha slope
    assert bool((ref > 0).any()) and bool((ref < 0).any())
    gout = torch.randn(shape, generator=g)
    got = run_bias_act(dev, gout, bias, ch, hh * ww, act, alpha, scale, grad=1, ref=ref)
    same("fused_bias_act grad", got, fwd(gout, bias, sign_of=ref)[0])
    r64, t64 = fwd(gout.double(), b64, sign_of=ref.double())
    within("fused_bias_act grad " + tag, got, r64, 3 * U * t64)


def check_bias_act_empty(dev):
    x = torch.randn(1, 2, 2, 2)
    out = run_bias_act(dev, x, None, 1, 1, 3, 0.2, 1.0, numel=0)
    assert bool(torch.isnan(out).all())                                        # nothing was written


# ---- axpy ---------------------------------------------------------------------------------------------------------------------
def check_axpy(dev, numel, acc, alpha=-0.37, seed=79):
    """dst (+)= alpha x: a product and a sum (2 roundings, 1 where hipcc fuses them)"""
    g = gen(seed + numel)
    x, old = torch.randn(numel, generator=g) * 4, torch.randn(numel, generator=g)
    dx, dst = x.to(dev), put(old if acc else torch.full((numel,), float("nan")), dev)
    a = L.AxpyArgs()
    a.x, a.gate, a.dst, a.numel, a.alpha, a.acc = p(dx), None, p(dst), numel, alpha, int(acc)
    launch("ssde_axpy", a, dev)
    sync(dev)
    al = float(torch.tensor(alpha, dtype=torch.float32))
    v = al * x.double()
    ref, mag = (old.double() + v, old.double().abs() + v.abs()) if acc else (v, v.abs())
    within("axpy numel=%d acc=%d" % (numel, acc), dst, ref, 2 * U * mag)


# ---- fill_from_table / step_inc -----------------------------------------------------------------------------------------------
def run_fill(dev, dst, tab, step):
    a = L.FillArgs()
    a.dst, a.tab, a.step_ptr, a.n = p(dst), p(tab), p(step), dst.numel()
    launch("ssde_fill_from_table", a, dev)


def run_step_inc(dev, step, delta):
    a = L.StepIncArgs()
    a.step_ptr, a.delta = p(step), delta
    launch("ssde_step_inc", a, dev)


def check_fill_and_step(dev):
    tab = torch.tensor([0.5, 1.5, -2.25, 3.0, 7.75]).to(dev)
    step = i32(1, dev)
    for n in (1, 257):
        buf = torch.full((n + 4,), SENTINEL).to(dev)
        run_fill(dev, buf[2:2 + n], tab, step)
        sync(dev)
        assert bool((buf.cpu()[2:2 + n] == 1.5).all()) and bool((buf.cpu()[:2] == SENTINEL).all()) and bool((buf.cpu()[2 + n:] == SENTINEL).all())
        run_fill(dev, buf[2:2 + n], tab, None)                                 # no step word: entry 0
        sync(dev)
        assert bool((buf.cpu()[2:2 + n] == 0.5).all())
    run_step_inc(dev, step, 3)
    sync(dev)
    assert int(step.cpu()) == 4
    run_step_inc(dev, step, -2)
    sync(dev)
    assert int(step.cpu()) == 2


def check_step_sequence(dev, numel=257, seed=83):
    """step_inc -> fill_from_table -> predictor_update in stream order: the fill and the predictor read the incremented row"""
    g = gen(seed)
    x, s, z = torch.randn(numel, generator=g) * 10, torch.randn(numel, generator=g) * 3, torch.randn(numel, generator=g)
    tab = torch.arange(5, dtype=torch.float32).mul(1.25).add(0.5)
    dx, dxm, dfill = put(x, dev), torch.full((numel,), float("nan")).to(dev), torch.full((3,), float("nan")).to(dev)
    keep = [s.to(dev), z.to(dev), PRED_COEF.to(dev), tab.to(dev), i32(1, dev)]
    run_step_inc(dev, keep[4], 2)
    run_fill(dev, dfill, keep[3], keep[4])
    run_predictor(dev, dx, dxm, keep[0], keep[1], keep[2], keep[4])
    sync(dev)
    assert int(keep[4].cpu()) == 3 and bool((dfill.cpu() == tab[3]).all())
    xm32, xo32, _, _ = predictor_ref(x, s, z, PRED_COEF[3])
    same("sequence x_mean", dxm, xm32)
    same("sequence x", dx, xo32)


# ---- randn --------------------------------------------------------------------------------------------------------------------
def run_randn(dev, numel, seed, step=None, stream_id=0, seed_word=None):
    dst = torch.full((numel,), float("nan")).to(dev)
    keep = [None if step is None else i32(step, dev), None if seed_word is None else torch.tensor([seed_word], dtype=torch.int64).to(dev)]
    a = L.RandnArgs()
    a.dst, a.numel, a.seed, a.step_ptr, a.stream_id, a.seed_ptr = p(dst), numel, seed, p(keep[0]), stream_id, p(keep[1])
    launch("ssde_randn", a, dev)
    sync(dev)
    return dst.cpu()


def _z(name, value, sigma):
    """|value| against 5 sigma of its estimator"""
    ratio = abs(value) / (5 * sigma)
    WORST["randn"] = max(WORST.get("randn", 0.0), ratio)
    print("randn %s: %.3g, 5 sigma = %.3g (ratio %.3f)" % (name, value, 5 * sigma, ratio))
    assert ratio <= 1.0, (name, value, 5 * sigma)


def moments(name, a):
    a = a.double()
    N = a.numel()
    assert bool(torch.isfinite(a).all())
    _z(name + " mean", float(a.mean()), 1 / N ** 0.5)
    _z(name + " variance", float((a * a).mean()) - 1.0, (2 / N) ** 0.5)
    _z(name + " fourth moment", float((a ** 4).mean()) - 3.0, (96 / N) ** 0.5)


def corr(name, a, b):
    _z(name + " correlation", float((a.double() * b.double()).mean()), 1 / a.numel() ** 0.5)


def check_randn_reproducible(dev, numel=1027):
    a = run_randn(dev, numel, 1234, step=3, stream_id=2)
    assert torch.equal(a, run_randn(dev, numel, 1234, step=3, stream_id=2))
    for other in (run_randn(dev, numel, 1235, step=3, stream_id=2), run_randn(dev, numel, 1234, step=4, stream_id=2),
                  run_randn(dev, numel, 1234, step=3, stream_id=3), run_randn(dev, numel, 1234, step=None, stream_id=2)):
        assert not torch.equal(a, other)
    assert torch.equal(run_randn(dev, numel, 1234, stream_id=2), run_randn(dev, numel, 1234, step=0, stream_id=2))   # no step word: step 0
    assert torch.equal(run_randn(dev, numel, 1000, step=3, stream_id=2, seed_word=234), a)         # seed + *seed_ptr
    assert torch.equal(run_randn(dev, numel, 0, step=3, stream_id=2, seed_word=1234), a)


def check_randn_sizes(dev):
    for numel in (1, 2, 3, 5, 7, 1027):
        assert bool(torch.isfinite(run_randn(dev, numel, 77 + numel)).all()), numel
    tails = torch.cat([run_randn(dev, 1027, 5000 + s)[1024:] for s in range(200)]).double()
    assert tails.numel() == 600 and bool(torch.isfinite(tails).all())
    _z("tail mean", float(tails.mean()), 1 / 600 ** 0.5)
    _z("tail variance", float((tails * tails).mean()) - 1.0, (2 / 600) ** 0.5)


def check_randn_moments(dev, numel=100003):
    a = run_randn(dev, numel, 4321, step=5, stream_id=0)
    moments("numel=%d" % numel, a)
    corr("steps 5 / 6", a, run_randn(dev, numel, 4321, step=6, stream_id=0))
    streams = [a] + [run_randn(dev, numel, 4321, step=5, stream_id=k) for k in (1, 2, 3)]
    for i, j in itertools.combinations(range(4), 2):
        corr("streams %d / %d" % (i, j), streams[i], streams[j])
    corr("neighbours", a[:-1], a[1:])


def check_randn_large(dev, numel=2 * 1024 * 1024 + 3):
    """1024 blocks of 256 lanes write 4 elements each per pass: the first 2^20 elements are the first pass, the next 2^20 the second"""
    assert numel > 1024 * 1024 and numel % 4 == 3
    a = run_randn(dev, numel, 97, step=1, stream_id=1)
    moments("large", a)
    half = 1024 * 1024
    corr("first / second pass", a[:half], a[half:2 * half])


# ---- alignment refusals (host-side: nothing is launched) -------------------------------------------------------------------------
def check_alignment_refusals(dev):
    buf = torch.zeros(64).to(dev)
    part, out = torch.zeros(1024).to(dev), torch.zeros(1).to(dev)
    assert buf.data_ptr() % 16 == 0
    for off in (4, 8, 12):
        a = L.SumsqFlatArgs()
        a.x, a.numel, a.partial, a.out = buf.data_ptr() + off, 16, p(part), p(out)
        refused("ssde_sumsq_flat", a, dev, "sumsq_flat", "16-byte aligned")
        r = L.RandnArgs()
        r.dst, r.numel, r.seed = buf.data_ptr() + off, 16, 1
        refused("ssde_randn", r, dev, "randn", "16-byte aligned")
    sync(dev)
    assert float(buf.cpu().abs().max()) == 0.0
