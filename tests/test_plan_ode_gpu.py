"""ODE plans on the MI355X (`-m gpu`): the sampler plan over the full span against the reference's fixture and against
ode.solve_rk45 on the same device, the likelihood plan against the Python driver, and tests/c_host/ode_host.c linked with
libssde_hip.so as one child process.  Bounds and the reasons for them: _plan_ode_checks.py."""
import pytest
import torch

import _util
import _plan_ode_checks as P

pytestmark = pytest.mark.gpu


def _full_sample_span():
    case = _util.ODE_CASE
    return (1.0, case["sample_eps"], case["rtol"])     # sde.T -> eps, rtol = atol = 1e-5 (sampling.get_ode_sampler)


def _assert_matches_fixture(x, nfev):
    gold = P.gold()
    assert abs(nfev - int(gold["ode_nfe"])) <= P.SAMPLE_NFE, (nfev, int(gold["ode_nfe"]))
    assert _util.rel_err(_util.ode_inverse_scaler(x), torch.from_numpy(gold["ode_samples"])) < P.SAMPLE_TOL


@pytest.mark.parametrize("use_graph", [True, False])
def test_sampler_plan_full_span_on_device(use_graph):
    """T -> sample_eps at the fixture's rtol = atol = 1e-5 through LoadedPlan, graph replay and op by op: against the
    REFERENCE's get_ode_sampler output (bounds of check_ode_sampler) and against ode.solve_rk45 on the same device"""
    span = _full_sample_span()
    x, _, nfev = P.c_solve("sample", "cuda", *span, use_graph=use_graph)
    _assert_matches_fixture(x, nfev)
    y_py, nfev_py = P.python_solve("sample", "cuda", *span)
    P.assert_drivers_agree("sample", x, None, nfev, y_py, nfev_py)


def test_likelihood_plan_on_device():
    """lik_eps -> T at rtol = atol = 1e-3 (a few hundred evaluations; the count is printed) against the Python driver on the
    device; one evaluation is pinned to the reference by the emulator test of ssde_ode_eval, the 2000-evaluation solve at
    1e-5 stays with the Python test"""
    span = (_util.ODE_CASE["lik_eps"], 1.0, 1e-3)
    x, dl, nfev = P.c_solve("likelihood", "cuda", *span, use_graph=True)
    y_py, nfev_py = P.python_solve("likelihood", "cuda", *span)
    assert 50 <= nfev_py <= 2000, nfev_py
    P.assert_drivers_agree("likelihood", x, dl, nfev, y_py, nfev_py)


def test_ode_host_c_full_span_on_device(tmp_path):
    """tests/c_host/ode_host.c linked with libssde_hip.so: `sample` over the full span, graph replay, against the fixture"""
    exe = P.build_c_host(tmp_path)
    x, _, nfev, _ = P.run_c_host(exe, "sample", "cuda", tmp_path, *_full_sample_span(), use_graph=True, timeout=120)
    _assert_matches_fixture(x, nfev)
