"""scipy's RK23 and DOP853 beside RK45 (`-m "not gpu"`): the tables of ode.TABLEAUS, ode.solve_rk on the host against
scipy, the generalised stage kernels and the library driver ssde_ode_solve_method on the emulator, the slope rows a plan
blob carries, and the routing of ode.integrate_ode.  Systems, spans, bounds and the reasons for them: _ode_method_checks.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import _util
import _plan_ode_checks as P
import _ode_method_checks as M


@pytest.fixture()
def emulated():
    import emu
    if not emu.available():
        pytest.skip("emulator needs x86-64 + ROCm's clang++")
    with emu.emulated():
        yield emu


# ---- 1. tables --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["RK23", "RK45", "DOP853"])
def test_tableaus_are_scipys(method):
    """every entry equal, not close: the drivers reproduce scipy's accept / reject decisions only with its very coefficients"""
    from score_sde_pytorch_amd import ode
    tab, ref = ode.TABLEAUS[method], M.scipy_tableau(method)
    assert tab["n_stages"] == ref["n_stages"] == M.N_STAGES[method] and tab["order"] == ref["order"]
    assert np.array_equal(M.dense_a(tab["A"], ref["A"].shape[1]), ref["A"])
    assert all(len(r) == s for s, r in enumerate(tab["A"]))
    for name in ("C", "B") + (("E3", "E5") if method == "DOP853" else ("E",)):
        assert np.array_equal(np.array(tab[name]), ref[name]), name
    assert ("E" in tab) != ("E3" in tab)
    assert len(tab["E5" if method == "DOP853" else "E"]) == tab["n_stages"] + 1


# ---- 2. the host driver against scipy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-5, 1e-3])
@pytest.mark.parametrize("method", ["RK23", "RK45", "DOP853"])
def test_solve_rk_reproduces_scipy(method, tol):
    """ode.solve_rk is scipy's method (same initial step, error norm, step control): identical nfev, result to rounding"""
    from scipy import integrate
    from score_sde_pytorch_amd import ode
    f_np, f_t, y0, spans = M.small_system()
    for span in spans:
        sol = integrate.solve_ivp(f_np, span, y0, rtol=tol, atol=tol, method=method)
        y, nfev = ode.solve_rk(f_t, span, torch.from_numpy(y0), tol, tol, method=method)
        assert nfev == sol.nfev, (span, nfev, sol.nfev)
        assert float(np.abs(sol.y[:, -1] - y.numpy()).max()) < 1e-12
    if method == "RK45":
        y45, n45 = ode.solve_rk45(f_t, spans[0], torch.from_numpy(y0), tol, tol)
        y, nfev = ode.solve_rk(f_t, spans[0], torch.from_numpy(y0), tol, tol)
        assert n45 == nfev and torch.equal(y45, y)


def test_solve_rk_refuses_what_it_cannot_run():
    from score_sde_pytorch_amd import ode
    f_np, f_t, y0, spans = M.small_system()
    with pytest.raises(ValueError, match="Radau"):
        ode.solve_rk(f_t, spans[0], torch.from_numpy(y0), method="Radau")
    y = torch.from_numpy(y0)
    with pytest.raises(ValueError, match="13 slope rows.* 7"):
        ode.solve_rk(f_t, spans[0], y, method="DOP853", stages=ode._TorchStages(3, y))


# ---- 3. the stage kernels on the emulator -----------------------------------------------------------------------------
@pytest.mark.parametrize("method,want_nfev", [("RK23", 656), ("DOP853", 74)])
def test_stage_kernels_reproduce_scipy(method, want_nfev, emulated):
    """ssde_rk_combine_rows / ssde_rk_error_norm_rows driving scipy's step-size controller: identical evaluation count and
    solution on the analytic system of the RK45 kernel test"""
    from scipy import integrate
    from score_sde_pytorch_amd import ode
    f_np, f_t, y0 = M.wide_system()
    stages = ode._HipStages(y0.numel(), y0, rows=M.N_STAGES[method] + 1)
    stages.K.fill_(float("nan"))                       # no row is read before the step has filled it
    y, nfev = ode.solve_rk(f_t, (0.0, 2.0), y0, rtol=1e-6, atol=1e-8, method=method, stages=stages)
    sol = integrate.solve_ivp(f_np, (0.0, 2.0), y0.numpy(), rtol=1e-6, atol=1e-8, method=method)
    assert nfev == sol.nfev == want_nfev
    assert float((y - torch.from_numpy(sol.y[:, -1])).abs().max()) < 1e-11


def test_combine_rows_twelve_terms(emulated):
    """dst = y + sum of 12 non-zero terms, ascending, within 4 ulp of the same sum in torch (the kernel may contract a
    multiply-add; an ulp is taken at the largest intermediate of the element's sum), and the fp32 copy is its rounding"""
    from score_sde_pytorch_amd import ode
    g = torch.Generator().manual_seed(11)
    n = 777                                            # four blocks, the last one ragged
    y0 = torch.randn(n, generator=g, dtype=torch.float64)
    x32 = torch.zeros(n + 5, dtype=torch.float32)
    stages = ode._HipStages(n, y0, x32=x32, n32=n - 7, rows=13)
    stages.K.copy_(torch.randn(13, n, generator=g, dtype=torch.float64))
    coefs = [float(c) for c in torch.randn(12, generator=g, dtype=torch.float64)]
    out = torch.empty_like(y0)
    stages.combine(y0, coefs, out)
    acc, big = torch.zeros_like(y0), y0.abs()
    for j, c in enumerate(coefs):
        term = stages.K[j] * c
        acc = acc + term
        big = torch.maximum(big, torch.maximum(term.abs(), acc.abs()))
    ref = y0 + acc
    ulp = torch.from_numpy(np.spacing(torch.maximum(big, ref.abs()).numpy()))
    assert bool(((out - ref).abs() <= 4 * ulp).all()), float(((out - ref).abs() / ulp).max())
    assert torch.equal(x32[:n - 7], out.to(torch.float32)[:n - 7]) and not x32[n - 7:].any()      # n32 bounds the copy
    # a zero coefficient's row is not read: NaN there changes nothing
    stages.K[4].fill_(float("nan"))
    coefs[4] = 0.0
    out2 = torch.empty_like(y0)
    stages.combine(y0, coefs, out2)
    assert torch.isfinite(out2).all()
    # thirteen terms do not fit
    from score_sde_pytorch_amd import _lib as L
    a = L.RkCombineRowsArgs()
    a.y, a.k, a.n, a.terms, a.dst = y0.data_ptr(), stages.K.data_ptr(), n, 13, out.data_ptr()
    assert stages.lib.ssde_rk_combine_rows(C.byref(a), None) != 0 and b"terms = 13" in stages.lib.ssde_last_error()


def test_seven_row_entry_points_are_the_row_kernels(emulated):
    """ssde_rk_combine / ssde_rk_error_norm keep their structs and give the bits of the generalised entry points"""
    from score_sde_pytorch_amd import ode, _lib as L
    g = torch.Generator().manual_seed(12)
    n = 1500
    y0, y1 = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    stages = ode._HipStages(n, y0)
    stages.K.copy_(torch.randn(7, n, generator=g, dtype=torch.float64))
    tab = ode.TABLEAUS["RK45"]
    h = -0.0123
    new_out, old_out = torch.empty_like(y0), torch.empty_like(y0)
    stages.combine(y0, [b * h for b in tab["B"]], new_out)
    a = L.RkCombineArgs()
    a.y, a.k, a.n, a.terms, a.dst = y0.data_ptr(), stages.K.data_ptr(), n, 6, old_out.data_ptr()
    for j in range(6):
        a.coef[j] = tab["B"][j] * h
    L.check(stages.lib.ssde_rk_combine(C.byref(a), None))
    assert torch.equal(new_out, old_out)
    new_norm = stages.error_norm(y0, y1, [e * h for e in tab["E"]], 1e-5, 1e-4)
    e = L.RkErrorArgs()
    e.y, e.y_new, e.k, e.n, e.atol, e.rtol = y0.data_ptr(), y1.data_ptr(), stages.K.data_ptr(), n, 1e-5, 1e-4
    e.partial, e.partial_len, e.out = stages.partial.data_ptr(), stages.partial.numel(), stages.out.data_ptr()
    for j in range(7):
        e.coef[j] = tab["E"][j] * h
    L.check(stages.lib.ssde_rk_error_norm(C.byref(e), None))
    assert float(stages.out.item()) == new_norm
    scale = 1e-5 + torch.maximum(y0.abs(), y1.abs()) * 1e-4
    ref = float(torch.sqrt(torch.mean((sum(stages.K[j] * (tab["E"][j] * h) for j in range(7)) / scale) ** 2)))
    assert abs(new_norm - ref) <= 1e-14 * ref


@pytest.mark.parametrize("n", [301, 200000])
def test_pair_error_norm(n, emulated):
    """the DOP853 form of the norm against numpy's formula (1e-14 relative), exactly 0.0 when both sums are 0, and blind to
    a NaN row whose two coefficients are zero; n = 200000 takes more blocks than the 512 partials a sum may use"""
    from score_sde_pytorch_amd import ode
    g = torch.Generator().manual_seed(13)
    y0, y1 = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    stages = ode._HipStages(n, y0, rows=13)
    stages.K.copy_(torch.randn(13, n, generator=g, dtype=torch.float64))
    tab = ode.TABLEAUS["DOP853"]
    assert tab["E5"][12] == 0.0 and tab["E3"][12] == 0.0 and tab["E5"][1] == 0.0 and tab["E3"][1] == 0.0
    for j in (1, 2, 3, 4, 12):
        stages.K[j].fill_(float("nan"))                # rows neither E5 nor E3 weighs
    Kn = stages.K.numpy().copy()
    Kn[np.isnan(Kn)] = 0.0
    got = stages.error_norm_pair(y0, y1, tab["E5"], tab["E3"], 0.037, 1e-6, 1e-3)
    ref = M.pair_norm_numpy(Kn, np.array(tab["E5"]), np.array(tab["E3"]), y0.numpy(), y1.numpy(), 0.037, 1e-6, 1e-3)
    assert np.isfinite(got) and abs(got - ref) <= 1e-14 * ref, (got, ref)
    torch_ref = ode._TorchStages(n, y0, rows=13)
    torch_ref.K.copy_(torch.from_numpy(Kn))
    assert abs(torch_ref.error_norm_pair(y0, y1, tab["E5"], tab["E3"], 0.037, 1e-6, 1e-3) - ref) <= 1e-14 * ref
    stages.K.zero_()
    assert stages.error_norm_pair(y0, y1, tab["E5"], tab["E3"], 0.037, 1e-6, 1e-3) == 0.0


# ---- 4. the library driver against the Python driver ------------------------------------------------------------------
@pytest.mark.parametrize("method", M.METHODS)
@pytest.mark.parametrize("kind", ["sample", "likelihood"])
def test_c_driver_matches_python_driver(kind, method, emulated):
    """ssde_ode_solve_method against ode.solve_rk: same emulator, same scalars, the short spans of _ode_method_checks.py"""
    span = M.SHORT[(kind, method)]
    y_py, nfev_py = M.python_solve(kind, "cpu", method, *span)
    assert 2 + 2 * M.N_STAGES[method] <= nfev_py <= 40, nfev_py
    x, dl, nfev = M.c_solve(kind, "cpu", method, *span)
    M.assert_drivers_agree(kind, method, x, dl, nfev, y_py, nfev_py)


# ---- 5. slope rows ----------------------------------------------------------------------------------------------------
def _k_rows(blob, n_state):
    from score_sde_pytorch_amd import plan_export as X
    hdr = X.PlanHeader.from_buffer_copy(blob[:C.sizeof(X.PlanHeader)])
    off = C.sizeof(X.PlanHeader) + hdr.io[X.IO_ODE_K] * C.sizeof(X.PlanRegion)
    return X.PlanRegion.from_buffer_copy(blob[off: off + C.sizeof(X.PlanRegion)]).bytes // (8 * n_state)


def test_blob_rows_follow_the_method(emulated):
    """the default blob is the RK45 blob, byte for byte; a DOP853 blob carries 13 rows, an RK23 blob the 7 every plan has"""
    from score_sde_pytorch_amd import plan_export as X
    rhs, blob = P.rhs_of("sample", "cpu")
    assert X.export_ode_plan(rhs) == X.export_ode_plan(rhs, method="RK45") == blob
    assert _k_rows(blob, rhs.n) == 7
    assert _k_rows(X.export_ode_plan(rhs, method="DOP853"), rhs.n) == 13
    assert X.export_ode_plan(rhs, method="RK23") == blob
    with pytest.raises(ValueError, match="Radau"):
        X.export_ode_plan(rhs, method="Radau")


def test_default_blob_runs_rk23_and_refuses_dop853(emulated):
    from score_sde_pytorch_amd import ode, plan_export as X, _lib as L
    rhs, plan = P.rhs_of("sample", "cpu")[0], P.plan_of("sample", "cpu")
    cfg, model, sde, z, data, eps = P.case("cpu")
    x, _, nfev = M.c_solve("sample", "cpu", "RK23", *M.ONE_STEP, plan=plan)
    assert nfev >= 5 and (nfev - 2) % 3 == 0 and torch.isfinite(x).all() and not torch.equal(x, z)
    plan.ode_reset(z)
    with pytest.raises(L.SsdeError, match="DOP853 needs 13 slope rows, the plan holds 7"):
        plan.ode_solve(*M.ONE_STEP[:2], 1e-3, 1e-3, ode.scalars_fn(rhs), method="DOP853")
    assert torch.equal(plan.ode_state(z)[0], z)         # refused before anything ran
    with pytest.raises(ValueError, match="LSODA"):
        plan.ode_solve(*M.ONE_STEP[:2], 1e-3, 1e-3, ode.scalars_fn(rhs), method="LSODA")
    assert plan.lib.ssde_ode_solve_method(plan.handle, 3, 1.0, 0.9, 1e-3, 1e-3, X.ODE_SCALARS_FN(), None, 0, 0, None, None) != 0
    assert b"method 3" in plan.lib.ssde_last_error()


def test_dop853_blob_runs_dop853(emulated):
    x, _, nfev = M.c_solve("sample", "cpu", "DOP853", *M.ONE_STEP)
    cfg, model, sde, z, data, eps = P.case("cpu")
    assert nfev >= 14 and (nfev - 2) % 12 == 0 and torch.isfinite(x).all() and not torch.equal(x, z)
    # the larger plan still runs the two smaller methods
    x5, _, n5 = M.c_solve("sample", "cpu", "RK45", *M.ONE_STEP, plan=M.plan_for("sample", "cpu", "DOP853"))
    assert (n5 - 2) % 6 == 0 and torch.isfinite(x5).all()


def test_ode_solve_is_the_rk45_method(emulated):
    """ssde_ode_solve and ssde_ode_solve_method(SSDE_ODE_RK45): bitwise equal states, equal counts"""
    from score_sde_pytorch_amd import plan_export as X

    def old_entry(plan, t0, t1, tol, scalars, stream):
        nfev = C.c_int32(0)
        fn = X._ode_callback(scalars)
        rc = plan.lib.ssde_ode_solve(plan.handle, t0, t1, tol, tol, fn, None, 0, 0, C.byref(nfev), C.c_void_p(stream or 0))
        plan._ode_call("ssde_ode_solve", fn, rc)
        return int(nfev.value)
    assert X.ODE_METHODS["RK45"] == 0
    x_old, _, n_old = M.c_solve("sample", "cpu", "RK45", *P.SHORT_SAMPLE, entry=old_entry)
    x_new, _, n_new = M.c_solve("sample", "cpu", "RK45", *P.SHORT_SAMPLE)
    assert n_old == n_new and torch.equal(x_old, x_new)


# ---- 6. routing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["RK23", "Radau"])
def test_host_tensors_stay_with_scipy(method):
    from scipy import integrate
    from score_sde_pytorch_amd import ode
    f_np, f_t, y0, spans = M.small_system()
    ode.last_driver = None
    y, nfev = ode.integrate_ode(f_t, spans[0], torch.from_numpy(y0), 1e-5, 1e-5, method)
    sol = integrate.solve_ivp(f_np, spans[0], y0, rtol=1e-5, atol=1e-5, method=method)
    assert ode.last_driver == "host"
    assert nfev == sol.nfev and float(np.abs(sol.y[:, -1] - y.numpy()).max()) < 1e-12
