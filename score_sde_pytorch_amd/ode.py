"""On-device adaptive explicit Runge-Kutta: scipy's RK45, RK23 and DOP853.

The reference drives its probability-flow ODE sampler and likelihood with `scipy.integrate.solve_ivp(method=...)`
(sampling.py:473, likelihood.py:99; 'RK45' by default): every function evaluation converts the fp64 numpy state to an
fp32 device tensor and back (models/utils.py:181-188).  This is the same algorithm -- scipy's `RungeKutta` classes: the
method's table (TABLEAUS), FSAL, RMS error norm over the whole state (DOP853: its combined 5th / 3rd-order estimate),
step factor 0.9 * err^(-1/(order+1)) clamped to [0.2, 10], scipy's `select_initial_step` -- with the state kept as an
fp64 tensor on the GPU, so only one scalar (the error norm) crosses the PCIe bus per step.  `fun(t, y)` receives and
returns fp64 device tensors.
"""
import ctypes as C
import math
import os
import struct

import numpy as np
import torch

from . import _lib as L
from . import engine as E
from . import hipops
from . import sde_lib

# scipy 1.15's tables (scipy/integrate/_ivp/rk.py: RK23, RK45; dop853_coefficients.py: the first 12 stages of its extended
# table, which is all a step uses), value for value: tests/test_ode_methods_cpu.py compares them with `==`.  Row s of A
# holds its s entries; `order` is scipy's error_estimator_order; E has n_stages + 1 entries (the last slope row is
# f(t + h, y_new)); DOP853 has the two error rows of its 8(5,3) estimator.
_DOP853_C = [0.0, 0.05260015195876773, 0.0789002279381516, 0.1183503419072274, 0.2816496580927726, 0.3333333333333333, 0.25, 0.3076923076923077, 0.6512820512820513, 0.6, 0.8571428571428571, 1.0]
_DOP853_A = [[],
             [0.05260015195876773],
             [0.0197250569845379, 0.0591751709536137],
             [0.02958758547680685, 0.0, 0.08876275643042054],
             [0.2413651341592667, 0.0, -0.8845494793282861, 0.924834003261792],
             [0.037037037037037035, 0.0, 0.0, 0.17082860872947386, 0.12546768756682242],
             [0.037109375, 0.0, 0.0, 0.17025221101954405, 0.06021653898045596, -0.017578125],
             [0.03709200011850479, 0.0, 0.0, 0.17038392571223998, 0.10726203044637328, -0.015319437748624402, 0.008273789163814023],
             [0.6241109587160757, 0.0, 0.0, -3.3608926294469414, -0.868219346841726, 27.59209969944671, 20.154067550477894, -43.48988418106996],
             [0.47766253643826434, 0.0, 0.0, -2.4881146199716677, -0.590290826836843, 21.230051448181193, 15.279233632882423, -33.28821096898486, -0.020331201708508627],
             [-0.9371424300859873, 0.0, 0.0, 5.186372428844064, 1.0914373489967295, -8.149787010746927, -18.52006565999696, 22.739487099350505, 2.4936055526796523, -3.0467644718982196],
             [2.273310147516538, 0.0, 0.0, -10.53449546673725, -2.0008720582248625, -17.9589318631188, 27.94888452941996, -2.8589982771350235, -8.87285693353063, 12.360567175794303, 0.6433927460157636]]
_DOP853_B = [0.054293734116568765, 0.0, 0.0, 0.0, 0.0, 4.450312892752409, 1.8915178993145003, -5.801203960010585, 0.3111643669578199, -0.1521609496625161, 0.20136540080403034, 0.04471061572777259]
_DOP853_E3 = [-0.18980075407240762, 0.0, 0.0, 0.0, 0.0, 4.450312892752409, 1.8915178993145003, -5.801203960010585, -0.4226823213237919, -0.1521609496625161, 0.20136540080403034, 0.02265179219836082, 0.0]
_DOP853_E5 = [0.01312004499419488, 0.0, 0.0, 0.0, 0.0, -1.2251564463762044, -0.4957589496572502, 1.6643771824549864, -0.35032884874997366, 0.3341791187130175, 0.08192320648511571, -0.022355307863886294, 0.0]
TABLEAUS = {
    "RK23": dict(n_stages=3, order=2, C=[0.0, 1 / 2, 3 / 4], A=[[], [1 / 2], [0.0, 3 / 4]], B=[2 / 9, 1 / 3, 4 / 9],
                 E=[5 / 72, -1 / 12, -1 / 9, 1 / 8]),
    "RK45": dict(n_stages=6, order=4, C=[0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0],
                 A=[[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
                    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]],
                 B=[35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
                 E=[-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]),
    "DOP853": dict(n_stages=12, order=7, C=_DOP853_C, A=_DOP853_A, B=_DOP853_B, E3=_DOP853_E3, E5=_DOP853_E5),
}
SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10.0


def _rms(x):
    return float(torch.sqrt(torch.mean(x * x)))


def _initial_step(fun, t0, y0, f0, direction, rtol, atol, order=4):
    """scipy.integrate._ivp.common.select_initial_step (runs once per solve); order: the method's error-estimator order."""
    scale = atol + torch.abs(y0) * rtol
    d0, d1 = _rms(y0 / scale), _rms(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    y1 = y0 + h0 * direction * f0
    f1 = fun(t0 + h0 * direction, y1)
    d2 = _rms((f1 - f0) / scale) / h0
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1 / (order + 1))
    return min(100 * h0, h1)


class _TorchStages:
    """Stage arithmetic with torch ops.  Reached only with host tensors (the CPU unit tests of the step-size controller
    against scipy on analytic right-hand sides): the model's right-hand side cannot run there."""

    def __init__(self, n, like, rows=7):
        self.K = torch.empty(rows, n, dtype=torch.float64, device=like.device)
        self.x32 = None

    def _dot(self, coefs):
        acc = None
        for j, c in enumerate(coefs):
            if c != 0.0:
                acc = self.K[j] * c if acc is None else acc + self.K[j] * c
        return acc

    def combine(self, y, coefs, dst):
        acc = self._dot(coefs)
        dst.copy_(y if acc is None else y + acc)

    def error_norm(self, y, y_new, coefs, atol, rtol):
        scale = atol + torch.maximum(torch.abs(y), torch.abs(y_new)) * rtol
        return _rms(self._dot(coefs) / scale)

    def error_norm_pair(self, y, y_new, coefs5, coefs3, h_abs, atol, rtol):
        """scipy's DOP853._estimate_error_norm: the 5th- and 3rd-order estimates combined; the coefficients are not scaled by h"""
        scale = atol + torch.maximum(torch.abs(y), torch.abs(y_new)) * rtol
        s5 = float(torch.sum((self._dot(coefs5) / scale) ** 2))
        s3 = float(torch.sum((self._dot(coefs3) / scale) ** 2))
        if s5 == 0 and s3 == 0:
            return 0.0
        return h_abs * s5 / math.sqrt((s5 + 0.01 * s3) * y.numel())


class _HipStages:
    """Stage arithmetic on the device (libssde_hip: ssde_rk_combine_rows, ssde_rk_error_norm_rows): one launch forms a stage
    argument together with its fp32 copy -- written straight into the U-Net's input buffer when the right-hand side is
    the fused drift (FusedDrift) -- and the error norm comes back as ONE scalar per step.  rows: slope rows of K, the
    method's n_stages + 1 (7: RK45).  The kernels read only rows with a non-zero coefficient, so K starts uninitialised."""

    def __init__(self, n, like, x32=None, n32=0, rows=7):
        self.lib, self.n, self.n32 = L.load(), n, int(n32)
        self.K = torch.empty(rows, n, dtype=torch.float64, device=like.device)
        self.partial = torch.empty(1024, dtype=torch.float64, device=like.device)
        self.out = torch.empty(1, dtype=torch.float64, device=like.device)
        self.x32 = x32

    def _stream(self):
        return hipops._stream()

    def combine(self, y, coefs, dst):
        a = L.RkCombineRowsArgs()
        terms = max([j + 1 for j, c in enumerate(coefs) if c != 0.0], default=0)
        a.y, a.k, a.n, a.terms, a.dst = y.data_ptr(), self.K.data_ptr(), self.n, terms, dst.data_ptr()
        a.dst32 = self.x32.data_ptr() if self.x32 is not None else None
        a.n32 = self.n32
        for j in range(terms):
            a.coef[j] = coefs[j]
        L.check(self.lib.ssde_rk_combine_rows(C.byref(a), self._stream()), "ssde_rk_combine_rows")

    def _norm(self, y, y_new, coefs, coefs2, h_abs, atol, rtol):
        a = L.RkErrorRowsArgs()
        a.y, a.y_new, a.k, a.n, a.atol, a.rtol = y.data_ptr(), y_new.data_ptr(), self.K.data_ptr(), self.n, atol, rtol
        a.partial, a.partial_len, a.out = self.partial.data_ptr(), self.partial.numel(), self.out.data_ptr()
        a.rows, a.pair, a.h_abs = len(coefs), int(coefs2 is not None), h_abs
        for j, c in enumerate(coefs):
            a.coef[j] = c
        for j, c in enumerate(coefs2 or ()):
            a.coef2[j] = c
        L.check(self.lib.ssde_rk_error_norm_rows(C.byref(a), self._stream()), "ssde_rk_error_norm_rows")
        return float(self.out.item())          # the one host read of the step

    def error_norm(self, y, y_new, coefs, atol, rtol):
        return self._norm(y, y_new, coefs, None, 0.0, atol, rtol)

    def error_norm_pair(self, y, y_new, coefs5, coefs3, h_abs, atol, rtol):
        return self._norm(y, y_new, coefs5, coefs3, h_abs, atol, rtol)


def solve_rk(fun, t_span, y0, rtol=1e-5, atol=1e-5, method="RK45", stages=None):
    """Integrate dy/dt = fun(t, y) from t_span[0] to t_span[1] with scipy's explicit method `method` (a key of TABLEAUS);
    returns (y_final, nfev).

    `fun(t, y)` returns the fp64 slope, or -- for right-hand sides that write their result in place (FusedDrift) --
    `fun(t, y, out=K_row)` fills `out`.  `stages`: the arithmetic backend (device kernels for CUDA tensors), with at least
    n_stages + 1 rows of K."""
    if method not in TABLEAUS:
        raise ValueError("solve_rk: method must be one of %s, got %r" % (sorted(TABLEAUS), method))
    tab = TABLEAUS[method]
    n_stages, tab_a, tab_b, tab_c = tab["n_stages"], tab["A"], tab["B"], tab["C"]
    exponent = -1 / (tab["order"] + 1)
    t, t_bound = float(t_span[0]), float(t_span[1])
    direction = 1.0 if t_bound >= t else -1.0
    y = y0.to(torch.float64).clone()
    n = y.numel()
    if stages is None:
        stages = (_HipStages if y.is_cuda else _TorchStages)(n, y, rows=n_stages + 1)
    K = stages.K
    if K.shape[0] < n_stages + 1:
        raise ValueError("solve_rk: %s needs %d slope rows, the stages hold %d" % (method, n_stages + 1, K.shape[0]))
    in_place = getattr(fun, "writes_out", False)

    def evaluate(tt, yy, row):
        if in_place:
            fun(tt, yy, out=K[row])
        else:
            K[row].copy_(fun(tt, yy))
    y_stage, y_new = torch.empty_like(y), torch.empty_like(y)
    stages.combine(y, [], y_stage)                       # stage argument of the first evaluation (and its fp32 copy)
    evaluate(t, y_stage, 0)
    nfev = 1
    h_abs = _initial_step((lambda tt, yy: _once(fun, stages, tt, yy, in_place)), t, y, K[0].clone(), direction, rtol, atol,
                          order=tab["order"])
    nfev += 1
    while direction * (t - t_bound) < 0:
        min_step = 10 * abs(math.nextafter(t, direction * math.inf) - t)
        h_abs = max(h_abs, min_step)
        rejected = False
        while True:
            if h_abs < min_step:
                raise RuntimeError("solve_rk: step size underflow (scipy: 'Required step size is less than spacing')")
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = abs(h)
            for s_ in range(1, n_stages):
                stages.combine(y, [a * h for a in tab_a[s_]], y_stage)
                evaluate(t + tab_c[s_] * h, y_stage, s_)
            stages.combine(y, [b * h for b in tab_b], y_new)
            evaluate(t + h, y_new, n_stages)
            nfev += n_stages
            if "E" in tab:
                error_norm = stages.error_norm(y, y_new, [e * h for e in tab["E"]], atol, rtol)
            else:
                error_norm = stages.error_norm_pair(y, y_new, tab["E5"], tab["E3"], h_abs, atol, rtol)
            if error_norm < 1:
                factor = MAX_FACTOR if error_norm == 0 else min(MAX_FACTOR, SAFETY * error_norm ** exponent)
                if rejected:
                    factor = min(1.0, factor)
                h_abs *= factor
                break
            h_abs *= max(MIN_FACTOR, SAFETY * error_norm ** exponent)
            rejected = True
        t = t_new
        y, y_new = y_new, y                              # accept: swap buffers
        K[0].copy_(K[n_stages])                          # FSAL: the last slope is the next step's first
    return y, nfev


def solve_rk45(fun, t_span, y0, rtol=1e-5, atol=1e-5, stages=None):
    """solve_rk with scipy's RK45 (Dormand-Prince 5(4))."""
    return solve_rk(fun, t_span, y0, rtol=rtol, atol=atol, method="RK45", stages=stages)


def _once(fun, stages, t, yy, in_place):
    """One extra evaluation outside the stage table (scipy's select_initial_step probes f(t0 + h0, y0 + h0 f0))."""
    if not in_place:
        return fun(t, yy)
    out = torch.empty_like(yy)
    tmp = torch.empty_like(yy)
    stages.combine(yy, [], tmp)                          # refreshes the fp32 copy the fused right-hand side reads
    fun(t, tmp, out=out)
    return out


def rhs_cache_get(model, key, make, limit=None):
    """The fused right-hand sides of a model (lowered program + arena + packed weights + hipGraph each), newest last.
    Bounded PER KIND (key[0]: "drift" of the ODE sampler, "likelihood"): building samplers / likelihood closures with fresh SDE
    objects or varying batch shapes evicts the oldest entry of that kind (its graph and arena are released with it) instead of
    growing until the device runs out of memory -- and a loop that alternates sampling and likelihood evaluation over a few
    shapes does not make the two kinds evict each other (every eviction is a re-lowering and a re-capture on the next call).
    limit: entries kept per kind (default 4; SSDE_ODE_RHS_CACHE=<n> overrides)."""
    if limit is None:
        limit = max(1, int(os.environ.get("SSDE_ODE_RHS_CACHE", "4")))
    cache = model.__dict__.setdefault("_ode_rhs", {})
    rhs = cache.pop(key, None)
    fresh = rhs is None
    if fresh:
        rhs = make()
    cache[key] = rhs                                   # (re-)inserted as the most recently used
    kind = key[0] if isinstance(key, tuple) and key else None
    same = [k for k in cache if (k[0] if isinstance(k, tuple) and k else None) == kind]     # oldest first
    for k in same[:max(0, len(same) - limit)]:
        cache.pop(k)
    return rhs, fresh


class _FusedRhs:
    """Common part of the fused right-hand sides: the per-evaluation scalars live in a 24-byte DEVICE record
    (include/ssde.h: ssde_ode_dyn -- label, std, drift coefficient, g^2, the slope row to fill), uploaded before every
    evaluation, and every launch of an evaluation is an op of ONE program that reads them from there.  On the GPU that
    program is captured into a hipGraph once and replayed per evaluation (SSDE_ODE_GRAPH=0: launched op by op): an
    adaptive solve is ~500 evaluations of ~230 (sampler) to ~1100 (likelihood) launches each."""
    writes_out = True
    _RING = 32

    def _init_dyn(self, device):
        self.device = torch.device(device)
        self.dyn = torch.zeros(24, dtype=torch.uint8, device=self.device)
        on_gpu = self.device.type == "cuda"
        # a driver that enqueues more than _RING evaluations without reading anything back (a fixed-step integrator) must
        # not overwrite a record whose upload has not executed yet
        self._ring = E.PinnedRing(self._RING if on_gpu else 1, 24, torch.uint8, pinned=on_gpu)
        self.use_graph = on_gpu and os.environ.get("SSDE_ODE_GRAPH", "1") != "0"
        self.graph_stream = torch.cuda.Stream(device=self.device) if self.use_graph else None
        self.nfev = 0
        self.last_path = None

    def _scalars(self, t):
        """(label, std, a, g2) with the SDE's own fp32 torch expressions (f(x, t) is linear in x: a = f(1, t))."""
        sde = self.sde
        tv = torch.full((1,), float(t), dtype=torch.float32)
        one = torch.ones(1, 1, 1, 1)
        drift1, diffusion = sde.sde(one, tv)
        std = sde.marginal_prob(torch.zeros(1, 1, 1, 1), tv)[1]
        label = tv * 999 if self.vp_like else std                         # models/utils.py:147-166 (continuous labels)
        eng = self.unet
        second = float(std)
        if eng.sig is not eng.cond:
            # discrete-label (positional embedding) VE model with scale_by_sigma: the output is divided by
            # sigmas[labels.long()] (ncsnpp.py:245,377-379) -- the same table lookup UNetEngine.load_inputs does; the
            # value rides in the record's `std` slot (a VE network has no std head)
            second = float(eng.model.sigmas[int(label.reshape(-1)[0])])
        return float(label), second, float(drift1.reshape(-1)[0]), float((diffusion ** 2).reshape(-1)[0])

    def _upload(self, t, out):
        record = np.frombuffer(struct.pack("<ffffQ", *self._scalars(t), out.data_ptr()), dtype=np.uint8)

        def write(h):
            h.numpy()[:] = record
        self._ring.upload(self.dyn, write)

    def _head_ops(self):
        eng, n = self.unet, self.shape[0]
        p = self.dyn.data_ptr()
        ops = [L.make(L.OP_FILL, dst=eng.cond.tensor, tab=p, step_ptr=None, n=n)]
        if eng.sig is not eng.cond:
            ops.append(L.make(L.OP_FILL, dst=eng.sig.tensor, tab=p + 4, step_ptr=None, n=n))
        if self.vp_like:
            ops.append(L.make(L.OP_FILL, dst=eng.std.tensor, tab=p + 4, step_ptr=None, n=n))
        return ops

    def __call__(self, t, y, out):
        self.unet.weights.refresh()
        self._upload(t, out)
        if self.use_graph:
            cur = torch.cuda.current_stream()
            self.program.replay_from_current(cur if cur.cuda_stream != 0 else self.graph_stream)    # (capture needs a non-default stream)
            self.last_path = "graph"
        else:
            self.program.run()
            self.last_path = "eager"
        self.nfev += 1

    @staticmethod
    def applies(model, sde, x):
        from .models.ncsnpp import HipUNet
        if not isinstance(model, HipUNet) or not x.is_cuda or type(sde) not in (sde_lib.VESDE, sde_lib.VPSDE, sde_lib.subVPSDE):
            return False
        return not (type(sde) is not sde_lib.VESDE and model.config.model.scale_by_sigma)


class FusedDrift(_FusedRhs):
    """Right-hand side of the probability-flow ODE for an NCSNpp model and a stock SDE, without torch arithmetic:
    drift = f(x, t) - g(t)^2 score(x, t) / 2 (sde_lib.py:93-97 with probability_flow=True; score_fn models/utils.py:129-178).
    The integrator's combine kernel writes the fp32 state straight into the U-Net program's input buffer, the program
    runs (score head included: -h / std for VP / sub-VP), ssde_pf_drift forms the fp64 slope."""

    def __init__(self, model, sde, shape, device):
        self.sde, self.shape = sde, tuple(shape)
        self.vp_like = isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE))
        self.unet = E.UNetEngine(model, shape[0], shape[2], shape[3], device, vp_score=self.vp_like)
        self.n = int(torch.tensor(self.shape).prod())
        self.x32, self.n32 = self.unet.x_in.tensor[: self.n], self.n
        self._init_dyn(device)
        drift = L.make(L.OP_PF_DRIFT, x=self.x32, score=self.unet.out.tensor, dst=None, numel=self.n, a=0.0, g2=0.0, dyn=self.dyn)
        self.program = E.Program.of([self._head_ops(), self.unet.program, drift], self)


class FusedLikelihoodRhs(_FusedRhs):
    """Right-hand side of the likelihood ODE (likelihood.py:59-67): d/dt [x, delta log p] = [drift, eps^T (d drift / d x) eps]
    with the Hutchinson-Skilling probe eps fixed for the whole solve (likelihood.py:76-81).  One program per evaluation:
    labels -> U-Net forward (activations resident) -> drift -> input-gradient program with the probe as the cotangent
    (backward.TrainEngine without weight-gradient kernels) -> per-sample divergence (ssde_hutch_div).  The reference gets
    the same vector-Jacobian product from torch.autograd.grad (likelihood.py:29-35)."""

    def __init__(self, model, sde, shape, probe, device):
        from . import backward as B
        self.sde, self.shape = sde, tuple(shape)
        self.vp_like = isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE))
        eng = self.unet = B.TrainEngine(model, shape[0], shape[2], shape[3], device, vp_score=self.vp_like, input_grad=True,
                                        dropout=False, param_grads=False)
        self.n = int(torch.tensor(self.shape).prod())
        self.per = self.n // self.shape[0]
        self.x32, self.n32 = eng.x_in.tensor[: self.n], self.n
        self.eps = probe.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        eng.gout.tensor[: self.n].copy_(self.eps)        # the cotangent never changes: d(sum(score * eps)) / d score = eps
        self._init_dyn(device)
        drift = L.make(L.OP_PF_DRIFT, x=self.x32, score=eng.out.tensor, dst=None, numel=self.n, a=0.0, g2=0.0, dyn=self.dyn)
        div = L.make(L.OP_HUTCH_DIV, gx=eng.gx.tensor, eps=self.eps, dst=None, dst_off=self.n, n=self.shape[0], per=self.per,
                     a=0.0, g2=0.0, dyn=self.dyn)
        self.program = E.Program.of([self._head_ops(), eng.program[:eng.n_fwd], drift, eng.program[eng.n_fwd:], div], self)

    def set_probe(self, probe):
        """a new Hutchinson probe for the next solve (the reference draws one per likelihood_fn call, likelihood.py:76-81)"""
        self.eps.copy_(probe.detach().to(self.eps.device, torch.float32).reshape(-1))
        self.unet.gout.tensor[: self.n].copy_(self.eps)


def scalars_fn(rhs):
    """t -> (label, second, a, g2): the four floats a fused right-hand side uploads for an evaluation at t, as a callable.
    A C-ABI solve of the plan exported from `rhs` (plan_export.LoadedPlan.ode_solve) driven with it sees the very floats
    the Python solve uploads."""
    return rhs._scalars


def solve_host(fun, t_span, y0, rtol=1e-5, atol=1e-5, method="RK45"):
    """The reference's integrator, scipy.integrate.solve_ivp on the host, around the same tensor right-hand side as
    solve_rk: `fun(t, y)` takes / returns an fp64 tensor on y0's device; every evaluation crosses to numpy and back
    (what models/utils.py:181-188 does in the reference).  Used for the implicit methods and with SSDE_HOST_ODE=1."""
    from scipy import integrate
    dev = y0.device

    def rhs(t, y_np):
        y = torch.from_numpy(np.ascontiguousarray(y_np)).to(dev)
        return fun(float(t), y).detach().to("cpu", torch.float64).numpy()
    sol = integrate.solve_ivp(rhs, (float(t_span[0]), float(t_span[1])), y0.detach().to("cpu", torch.float64).numpy().reshape(-1),
                              rtol=rtol, atol=atol, method=method)
    return torch.from_numpy(sol.y[:, -1].copy()).to(dev), int(sol.nfev)


last_driver = None      # which integrator the latest integrate_ode call ran: "device" (solve_rk) or "host" (solve_host)


def integrate_ode(fun, t_span, y0, rtol, atol, method):
    """The device driver (solve_rk) for scipy's explicit methods -- RK23, RK45, DOP853 -- when the state lives on the GPU
    and nothing asks for the host path, else scipy on the host (implicit methods need Jacobians; SSDE_HOST_ODE=1).
    A right-hand side with `writes_out` (FusedDrift) gets the fp32 copy of every stage argument written into its input."""
    global last_driver
    if method in TABLEAUS and y0.is_cuda and os.environ.get("SSDE_HOST_ODE", "0") != "1":
        last_driver = "device"
        rows = TABLEAUS[method]["n_stages"] + 1
        side = getattr(fun, "graph_stream", None)
        if side is None:
            stages = _HipStages(y0.numel(), y0, x32=getattr(fun, "x32", None), n32=getattr(fun, "n32", 0), rows=rows)
            return solve_rk(fun, t_span, y0, rtol=rtol, atol=atol, method=method, stages=stages)
        # graph-captured right-hand side: the whole solve (stage kernels, graph replays, the one scalar read per step)
        # runs on the side stream the graph was captured on
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            stages = _HipStages(y0.numel(), y0, x32=getattr(fun, "x32", None), n32=getattr(fun, "n32", 0), rows=rows)
            res = solve_rk(fun, t_span, y0, rtol=rtol, atol=atol, method=method, stages=stages)
        torch.cuda.current_stream().wait_stream(side)
        return res
    last_driver = "host"
    if getattr(fun, "writes_out", False):
        inner = fun

        def fun(t, y):                                   # host scipy loop around the fused right-hand side
            inner.x32.copy_(y[: inner.n32].to(torch.float32))    # (the likelihood state carries B more values behind the image)
            out = torch.empty_like(y)
            inner(t, y, out=out)
            return out
    return solve_host(fun, t_span, y0, rtol=rtol, atol=atol, method=method)
