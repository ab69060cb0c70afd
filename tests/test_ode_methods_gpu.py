"""scipy's RK23 and DOP853 on the MI355X (`-m gpu`): sampling.get_ode_sampler and likelihood.get_likelihood_fn with
`method=` against the REFERENCE's own runs (tests/golden/ode_methods_small.npz), and the library driver through
LoadedPlan.ode_solve(method=...) against the fixture and against ode.solve_rk on the same device.  The batch-2, 16-px case
of _util.ODE_CASE.  Bounds and the reasons for them: _ode_method_checks.py."""
import pytest
import torch

import _util
import _ode_method_checks as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", M.METHODS)
def test_ode_sampler_method_against_reference(method):
    """RK23 at rtol = atol = 1e-4 (368 evaluations in the reference), DOP853 at 1e-5 (1358): samples 1e-3 relative, count
    within two steps, on the device driver around the fused right-hand side"""
    M.check_sampler("cuda", method)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("method", M.METHODS)
def test_sampler_plan_method_full_span(method, use_graph):
    """the same spans through LoadedPlan.ode_solve(method=...), graph replay and op by op: against the fixture with the
    sampler's bounds, against ode.solve_rk on the device with the drivers' bounds"""
    span = M.sample_span(method)
    x, _, nfev = M.c_solve("sample", "cuda", method, *span, use_graph=use_graph)
    M.assert_sample_matches_fixture(method, _util.ode_inverse_scaler(x), nfev)
    y_py, nfev_py = M.python_solve("sample", "cuda", method, *span)
    M.assert_drivers_agree("sample", method, x, None, nfev, y_py, nfev_py)


@pytest.mark.parametrize("method", M.METHODS)
def test_likelihood_method_against_reference(method):
    """rtol = atol = 1e-3 (575 / 1562 evaluations in the reference): bpd and latent within 100 x the stored sensitivities,
    count within 3 %; then the same solve through a likelihood plan against the Python driver"""
    M.check_likelihood("cuda", method)
    span = (_util.ODE_CASE["lik_eps"], 1.0, 1e-3)
    x, dl, nfev = M.c_solve("likelihood", "cuda", method, *span, use_graph=True)
    y_py, nfev_py = M.python_solve("likelihood", "cuda", method, *span)
    M.assert_drivers_agree("likelihood", method, x, dl, nfev, y_py, nfev_py)
