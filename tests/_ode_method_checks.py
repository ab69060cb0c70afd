"""Shared checks of the explicit Runge-Kutta methods beside RK45 -- scipy's RK23 and DOP853 -- in ode.solve_rk, the stage
kernels (ssde_rk_combine_rows / ssde_rk_error_norm_rows) and the library driver (ssde_ode_solve_method), for the emulator
tests (test_ode_methods_cpu.py) and the device tests (test_ode_methods_gpu.py).

Network, SDE and inputs are those of _plan_ode_checks.py (_util.ODE_CASE; sub-VP, batch 2, 16 px); the right-hand sides and
the default (7-row) plans are its cached ones, so the methods share them as the samplers do.  The reference's own runs are
in tests/golden/ode_methods_small.npz (tools/gen_golden_ode_methods.py).

Bounds.  Drivers against each other: _plan_ode_checks.DRIVER_TOL (1e-6), evaluation counts within one step of the method
(n_stages).  Against the reference: samples 1e-3 relative (SAMPLE_TOL; an fp32 evaluation differs by ~1e-5 and the
stored sensitivities, 9.2e-7 and 3.7e-6 per 1e-6 of input change, put that two orders below the bound), counts within two
steps.  Likelihood: 100 x the stored move per 1e-6 of input change (x10 for a 1e-5 evaluation difference, x10 margin: the
ratio _train_checks.check_likelihood arrives at), counts within 3 %.

The emulator runs one evaluation of the sampler program in ~2 s and one of the likelihood program in ~5 s, hence the short
spans there (evaluation counts of scipy.integrate.solve_ivp around the CPU oracle's right-hand side, recorded when the spans
were chosen; the emulator test requires at least two step attempts and at most 40 evaluations of ode.solve_rk):
  ("sample", "RK23"):       t 1.0  -> 0.98  at rtol = atol = 1e-3: 20 evaluations (6 step attempts)
  ("sample", "DOP853"):     t 1.0  -> 0.991 at rtol = atol = 1e-3: 38 evaluations (3 step attempts, 2 accepted)
  ("likelihood", "RK23"):   t 1e-5 -> 0.05  at rtol = atol = 1e-3: 20 evaluations (6 step attempts)
  ("likelihood", "DOP853"): t 1e-5 -> 0.02  at rtol = atol = 1e-3: 38 evaluations (3 step attempts)
"""
import functools
import math
import os

import numpy as np
import torch

import _util
import _plan_ode_checks as P

METHODS = ("RK23", "DOP853")
N_STAGES = {"RK23": 3, "RK45": 6, "DOP853": 12}
SHORT = {("sample", "RK23"): (1.0, 0.98, 1e-3), ("sample", "DOP853"): (1.0, 0.991, 1e-3),
         ("likelihood", "RK23"): (1e-5, 0.05, 1e-3), ("likelihood", "DOP853"): (1e-5, 0.02, 1e-3)}
ONE_STEP = (1.0, 0.999, 1e-3)              # a sampler span of a step or two with any method: for the row-count tests
SAMPLE_TAGS = {"RK23": "ode_rk23", "DOP853": "ode_dop853"}
LIK_TAGS = {"RK23": "lik_rk23", "DOP853": "lik_dop853"}


def gold():
    return np.load(os.path.join(_util.GOLDEN, "ode_methods_small.npz"))


# ---- scipy's tables and analytic systems ----------------------------------------------------------------------------
def scipy_tableau(method):
    """scipy's arrays for `method`: dict of C, A (n_stages x n_stages), B and E (or E3, E5)"""
    from scipy.integrate._ivp import rk, dop853_coefficients as D
    if method == "DOP853":
        return dict(C=D.C[:12], A=D.A[:12, :12], B=D.B, E3=D.E3, E5=D.E5, n_stages=12, order=rk.DOP853.error_estimator_order)
    cls = getattr(rk, method)
    return dict(C=cls.C, A=cls.A, B=cls.B, E=cls.E, n_stages=cls.n_stages, order=cls.error_estimator_order)


def dense_a(rows, cols):
    """ode.TABLEAUS stores row s of A with its s entries; scipy pads them to `cols` columns (RK45: 5, the others n_stages)"""
    a = np.zeros((len(rows), cols))
    for s, r in enumerate(rows):
        a[s, :len(r)] = r
    return a


def small_system():
    """the 3 x 3 system of test_host_cpu.test_on_device_rk45_reproduces_scipy: (numpy rhs, torch rhs, y0, spans)"""
    A = np.array([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.3], [0.0, -0.3, -1.0]])
    At = torch.from_numpy(A)
    b = np.array([1.0, 0.0, 0.5])
    bt = torch.from_numpy(b)
    y0 = np.array([1.0, -0.5, 2.0])
    return (lambda t, y: A @ y + math.sin(3 * t) * b), (lambda t, y: At @ y + math.sin(3 * t) * bt), y0, [(0.0, 5.0), (1.0, 1e-3)]


def wide_system():
    """the n = 301 system of test_emulated_kernels.test_rk45_stage_kernels_reproduce_scipy: (numpy rhs, torch rhs, y0)"""
    g = torch.Generator().manual_seed(3)
    n = 301                                            # not a multiple of the block size
    A = (torch.randn(n, n, generator=g, dtype=torch.float64) / n ** 0.5 - 0.5 * torch.eye(n, dtype=torch.float64))
    y0 = torch.randn(n, generator=g, dtype=torch.float64)
    An = A.numpy()
    return (lambda t, v: An @ v + np.sin(3.0 * t)), (lambda t, y: A @ y + torch.sin(torch.tensor(3.0 * t, dtype=torch.float64))), y0


def pair_norm_numpy(K, e5, e3, y, y_new, h_abs, atol, rtol):
    """scipy's DOP853._estimate_error_norm on numpy arrays (K: [rows, n])"""
    scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
    s5 = float(np.sum((np.dot(K.T, e5) / scale) ** 2))
    s3 = float(np.sum((np.dot(K.T, e3) / scale) ** 2))
    if s5 == 0 and s3 == 0:
        return 0.0
    return h_abs * s5 / math.sqrt((s5 + 0.01 * s3) * len(scale))


# ---- the two drivers around the fused right-hand sides --------------------------------------------------------------
def plan_for(kind, dev, method):
    """RK23 runs on the default 7-row plan of _plan_ode_checks; DOP853 gets a plan exported for it"""
    if method != "DOP853":
        return P.plan_of(kind, dev)
    return _dop_plan(kind, dev, P._mode())


@functools.lru_cache(maxsize=None)
def _dop_plan(kind, dev, mode):
    from score_sde_pytorch_amd import plan_export
    return plan_export.LoadedPlan(plan_export.export_ode_plan(P.rhs_of(kind, dev)[0], method="DOP853"))


def python_solve(kind, dev, method, t0, t1, tol):
    """ode.solve_rk around the fused right-hand side: (state fp64 [n] or [n + B], evaluations); computed once"""
    return _python_solve(kind, dev, method, t0, t1, tol, P._mode())


@functools.lru_cache(maxsize=None)
def _python_solve(kind, dev, method, t0, t1, tol, mode):
    from score_sde_pytorch_amd import ode
    rhs = P.rhs_of(kind, dev)[0]
    x0, probe = P.start_of(kind, dev)
    y0 = x0.reshape(-1).to(torch.float64)
    if probe is not None:
        rhs.set_probe(probe)
        y0 = torch.cat([y0, torch.zeros(x0.shape[0], dtype=torch.float64, device=y0.device)])
    if dev != "cpu":
        y, nfev = ode.integrate_ode(rhs, (t0, t1), y0, tol, tol, method)
        torch.cuda.synchronize()
        assert ode.last_driver == "device"
        return y, nfev
    stages = ode._HipStages(y0.numel(), y0, x32=rhs.x32, n32=rhs.n32, rows=N_STAGES[method] + 1)   # (integrate_ode sends host tensors to scipy)
    return ode.solve_rk(rhs, (t0, t1), y0, rtol=tol, atol=tol, method=method, stages=stages)


def c_solve(kind, dev, method, t0, t1, tol, use_graph=False, plan=None, entry=None):
    """the same solve through LoadedPlan.ode_solve(method=...): (x fp32, delta_logp fp64 or None, evaluations).
    entry: a callable(plan, t0, t1, tol, scalars, stream) -> evaluations that replaces the ode_solve call"""
    from score_sde_pytorch_amd import ode
    rhs = P.rhs_of(kind, dev)[0]
    plan = plan or plan_for(kind, dev, method)
    x0, probe = P.start_of(kind, dev)
    stream = None
    if dev != "cpu":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        stream = side.cuda_stream
    plan.ode_reset(x0, probe, stream=stream)
    if entry is None:
        nfev = plan.ode_solve(t0, t1, tol, tol, ode.scalars_fn(rhs), use_graph=use_graph, stream=stream, method=method)
    else:
        nfev = entry(plan, t0, t1, tol, ode.scalars_fn(rhs), stream)
    x, dl = plan.ode_state(x0, stream=stream)
    if dev != "cpu":
        side.synchronize()
    return x, dl, nfev


def assert_drivers_agree(kind, method, x, dl, nfev, y_py, nfev_py):
    d_n, d_x, d_l = P.driver_differences(kind + " " + method, x, dl, nfev, y_py, nfev_py)
    assert torch.isfinite(x).all() and (dl is None or torch.isfinite(dl).all())
    assert d_n <= N_STAGES[method], (nfev, nfev_py)
    assert d_x < P.DRIVER_TOL, d_x
    assert d_l < P.DRIVER_TOL, d_l


# ---- against the reference's runs (device tests) --------------------------------------------------------------------
def sample_span(method):
    g = gold()
    return (1.0, _util.ODE_CASE["sample_eps"], float(g[SAMPLE_TAGS[method] + "_tol"]))      # sde.T -> eps


def assert_sample_matches_fixture(method, x_scaled, nfev):
    """x_scaled: after the inverse scaler, as get_ode_sampler returns it"""
    g, tag = gold(), SAMPLE_TAGS[method]
    ref_nfe = int(g[tag + "_nfe"])
    d = _util.rel_err(x_scaled, torch.from_numpy(g[tag + "_samples"]))
    print("ode sampler %s: nfev %d (reference %d), samples rel diff %.3g (bound %g)" % (method, nfev, ref_nfe, d, P.SAMPLE_TOL))
    assert abs(nfev - ref_nfe) <= 2 * N_STAGES[method], (nfev, ref_nfe)
    assert d < P.SAMPLE_TOL, d


def check_sampler(dev, method):
    from score_sde_pytorch_amd import sampling, ode
    cfg, model, sde, z, data, eps = P.case(dev)
    tol = sample_span(method)[2]
    smp = sampling.get_ode_sampler(sde, tuple(z.shape), _util.ode_inverse_scaler, denoise=False, rtol=tol, atol=tol, method=method,
                                   eps=_util.ODE_CASE["sample_eps"], device=dev)
    ode.last_driver = None
    x, nfe = smp(model, z=z)
    assert ode.last_driver == "device" and smp.last_path == "fused"
    assert_sample_matches_fixture(method, x, nfe)


def likelihood_bounds(method):
    """(bpd bound, latent bound), relative: 100 x the fixture's move per 1e-6 of input change"""
    g, tag = gold(), LIK_TAGS[method]
    return 100 * float(g[tag + "_sens_bpd"]), 100 * float(g[tag + "_sens_z"])


def check_likelihood(dev, method):
    from score_sde_pytorch_amd import likelihood, ode
    g, tag = gold(), LIK_TAGS[method]
    cfg, model, sde, z, data, epsilon = P.case(dev)
    tol = float(g[tag + "_tol"])
    real = torch.randint_like
    torch.randint_like = lambda t, low=0, high=2, **kw: ((epsilon + 1.) / 2.).to(t.device)
    try:
        lik = likelihood.get_likelihood_fn(sde, _util.ode_inverse_scaler, rtol=tol, atol=tol, method=method, eps=_util.ODE_CASE["lik_eps"])
        ode.last_driver = None
        bpd, lat, nfe = lik(model, data)
    finally:
        torch.randint_like = real
    assert ode.last_driver == "device" and lik.last_path == "fused"
    b_bpd, b_z = likelihood_bounds(method)
    ref_nfe = int(g[tag + "_nfe"])
    d_bpd, d_z = _util.rel_err(bpd, torch.from_numpy(g[tag + "_bpd"])), _util.rel_err(lat, torch.from_numpy(g[tag + "_z"]))
    print("likelihood %s: nfev %d (reference %d), bpd rel diff %.3g (bound %.3g), latent rel diff %.3g (bound %.3g)"
          % (method, nfe, ref_nfe, d_bpd, b_bpd, d_z, b_z))
    assert torch.isfinite(bpd).all() and torch.isfinite(lat).all()
    assert abs(nfe - ref_nfe) <= 0.03 * ref_nfe, (nfe, ref_nfe)
    assert d_bpd < b_bpd, (d_bpd, b_bpd)
    assert d_z < b_z, (d_z, b_z)
