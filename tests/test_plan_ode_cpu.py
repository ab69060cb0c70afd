"""ODE plans on the emulator (`-m "not gpu"`): the blob of plan_export.export_ode_plan, the Dormand-Prince driver of
csrc/plan.hip through plan_export.LoadedPlan, and tests/c_host/ode_host.c compiled with gcc against the emulator library.
The loader, the relocation and the driver run for real; the kernels run on the emulator.  Spans, bounds and the reasons for
them: _plan_ode_checks.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _util
import _plan_ode_checks as P


@pytest.fixture()
def emulated():
    import emu
    if not emu.available():
        pytest.skip("emulator needs x86-64 + ROCm's clang++")
    with emu.emulated():
        yield emu


@pytest.mark.parametrize("kind", ["sample", "likelihood"])
def test_ode_blob_integrity(kind, emulated):
    """ops = the right-hand side's program, no absolute address left in it, kind and I/O slots as the header documents,
    solver regions of the documented sizes; a sampler plan refuses a probe"""
    from score_sde_pytorch_amd import plan_export as X, _lib as L
    rhs, blob = P.rhs_of(kind, "cpu")
    lik = kind == "likelihood"
    hdr = X.PlanHeader.from_buffer_copy(blob[:C.sizeof(X.PlanHeader)])
    assert hdr.abi_version == 13 and hdr.n_ops == rhs.program.n and hdr.n_relocs > hdr.n_ops
    assert hdr.kind == (X.PLAN_LIKELIHOOD if lik else X.PLAN_ODE) == (4 if lik else 3)
    assert (X.IO_ODE_DYN, X.IO_ODE_K, X.IO_ODE_STATE, X.IO_ODE_PROBE, X.IO_SLOTS) == (20, 21, 22, 23, 24)
    B, Cc, H, W = rhs.shape
    assert (hdr.batch, hdr.channels, hdr.height, hdr.width) == (B, Cc, H, W)
    off = C.sizeof(X.PlanHeader)
    regs = [X.PlanRegion.from_buffer_copy(blob[off + i * C.sizeof(X.PlanRegion): off + (i + 1) * C.sizeof(X.PlanRegion)])
            for i in range(hdr.n_regions)]
    off += hdr.n_regions * C.sizeof(X.PlanRegion)
    for i in range(hdr.n_ops):
        raw = blob[off + i * C.sizeof(L.Op): off + (i + 1) * C.sizeof(L.Op)]
        op = L.Op.from_buffer_copy(raw)
        assert int(op.kind) == int(rhs.program.ops[i].kind)
        for o in X._op_pointer_offsets(int(op.kind)):
            assert raw[o:o + 8] == b"\x00" * 8
    n = B * Cc * H * W
    n_state = n + (B if lik else 0)
    want = {X.IO_X: None, X.IO_COND: None, X.IO_OUT: None, X.IO_STD: None, X.IO_ODE_DYN: 24, X.IO_ODE_K: 7 * n_state * 8,
            X.IO_ODE_STATE: (3 * n_state + X.ODE_PARTIALS + 1) * 8}
    if lik:
        want.update({X.IO_ODE_PROBE: n * 4, X.IO_GOUT: None, X.IO_GX: None})
    for slot in range(X.IO_SLOTS):
        rid = hdr.io[slot]
        assert (rid >= 0) == (slot in want), slot
        if rid >= 0 and want[slot] is not None:
            assert regs[rid].bytes == want[slot] and regs[rid].kind == X.REGION_ZERO, slot
    plan = P.plan_of(kind, "cpu")
    assert plan.ode_state_len() == n_state
    if not lik:
        z, data, eps = _util.ode_case_inputs()
        with pytest.raises(L.SsdeError, match="probe"):
            plan.ode_reset(z, eps)


def test_ode_eval_matches_reference_rhs(emulated):
    """one evaluation through ssde_ode_eval at the data point against the REFERENCE's right-hand side (`rhs_drift`, `rhs_div`
    of the fixture at t_probe; the CPU oracle at a second time), bounds of _train_checks.check_fused_likelihood_rhs: 1e-4, the
    divergence on the scale of its number of terms.  The sampler plan's drift is the same function."""
    from score_sde_pytorch_amd import ode
    from oracle import ode_oracle, sampler_oracle
    gold, case = P.gold(), _util.ODE_CASE
    cfg, model, sde, z, data, eps = P.case("cpu")
    n, Bn = data.numel(), data.shape[0]
    scale = float(np.prod(data.shape[1:]))
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    osde = sampler_oracle.make_sde("subvpsde", **case["sde_kwargs"])
    rhs, plan = P.rhs_of("likelihood", "cpu")[0], P.plan_of("likelihood", "cpu")
    plan.ode_reset(data, eps)
    for t in (case["t_probe"], 0.61):
        out = plan.ode_eval(t, ode.scalars_fn(rhs), data)
        got_d, got_v = out[:n].reshape(data.shape).to(torch.float32), out[n:].to(torch.float32)
        if t == case["t_probe"]:
            ref_d, ref_v = torch.from_numpy(gold["rhs_drift"]), torch.from_numpy(gold["rhs_div"])
        else:
            ref_d, ref_v = ode_oracle.rhs_augmented(cfg, sd, osde, data, torch.ones(Bn) * t, eps)
        assert _util.rel_err(got_d, ref_d) < 1e-4, (t, _util.rel_err(got_d, ref_d))
        assert float((got_v - ref_v).abs().max()) / scale < 1e-4, (t, got_v, ref_v)
    srhs, splan = P.rhs_of("sample", "cpu")[0], P.plan_of("sample", "cpu")
    splan.ode_reset(data)
    out = splan.ode_eval(case["t_probe"], ode.scalars_fn(srhs), data)
    assert out.shape == (n,) and _util.rel_err(out.reshape(data.shape).to(torch.float32), torch.from_numpy(gold["rhs_drift"])) < 1e-4


@pytest.mark.parametrize("kind,span", [("sample", P.SHORT_SAMPLE), ("likelihood", P.SHORT_LIK)])
def test_c_driver_matches_python_driver(kind, span, emulated):
    """ssde_ode_solve against ode.solve_rk45: same emulator, same scalars, the short span of _plan_ode_checks.py"""
    y_py, nfev_py = P.python_solve(kind, "cpu", *span)
    assert 8 <= nfev_py <= 50, nfev_py
    x, dl, nfev = P.c_solve(kind, "cpu", *span)
    P.assert_drivers_agree(kind, x, dl, nfev, y_py, nfev_py)


@pytest.mark.parametrize("kind,span", [("sample", P.SHORT_SAMPLE), ("likelihood", P.SHORT_LIK)])
def test_ode_host_c_matches_python_driver(kind, span, emulated, tmp_path):
    """tests/c_host/ode_host.c (its own C scalars, which may differ from torch's in the last float bit) on the short span:
    the project's sampler bounds, _train_checks.check_ode_sampler -- state 1e-3 relative, NFE within two steps"""
    exe = P.build_c_host(tmp_path, emu_lib=emulated.build_emu.build())
    y_py, nfev_py = P.python_solve(kind, "cpu", *span)
    x, dl, nfev, _ = P.run_c_host(exe, kind, "cpu", tmp_path, *span, use_graph=False, timeout=900)
    n = x.numel()
    assert abs(nfev - nfev_py) <= P.SAMPLE_NFE, (nfev, nfev_py)
    assert _util.rel_err(x.reshape(-1), y_py[:n].to(torch.float32)) < P.SAMPLE_TOL
    if kind == "likelihood":
        assert _util.rel_err(dl, y_py[n:]) < P.SAMPLE_TOL, (dl, y_py[n:])


def test_ode_errors_are_reported_and_leave_the_plan_usable(emulated):
    from score_sde_pytorch_amd import ode, engine as E, plan_export as X, _lib as L
    cfg, model, sde, z, data, eps = P.case("cpu")
    rhs, plan = P.rhs_of("sample", "cpu")[0], P.plan_of("sample", "cpu")
    sc = ode.scalars_fn(rhs)
    t0, t1, tol = P.SHORT_SAMPLE
    plan.ode_reset(z)
    with pytest.raises(L.SsdeError, match="max_nfev = 7 reached"):
        plan.ode_solve(t0, t1, tol, tol, sc, max_nfev=7)
    # ... the two evaluations of the initial step ran, the state is untouched and the plan evaluates as before
    x, _ = plan.ode_state(z)
    assert torch.equal(x, z)
    ref = torch.empty(z.numel(), dtype=torch.float64)
    rhs.x32.copy_(z.reshape(-1))
    rhs(0.5, None, out=ref)
    assert torch.equal(plan.ode_eval(0.5, sc, z), ref)
    with pytest.raises(L.SsdeError, match="t0 == t1"):
        plan.ode_solve(0.5, 0.5, tol, tol, sc)
    with pytest.raises(L.SsdeError, match="non-default stream"):
        plan.ode_solve(t0, t1, tol, tol, sc, use_graph=True)
    with pytest.raises(ZeroDivisionError):                              # a failing callback aborts the solve
        plan.ode_solve(t0, t1, tol, tol, lambda t: 1 / 0)
    lib, h = plan.lib, plan.handle
    assert lib.ssde_ode_reset(h, None, None, None) != 0 and b"null x0" in lib.ssde_last_error()
    assert lib.ssde_ode_solve(h, t0, t1, tol, tol, X.ODE_SCALARS_FN(), None, 0, 0, None, None) != 0 and b"callback" in lib.ssde_last_error()
    assert lib.ssde_ode_eval(h, 0.5, X.ODE_SCALARS_FN(), None, None, None) != 0 and b"null" in lib.ssde_last_error()
    dl = torch.zeros(2, dtype=torch.float64)
    assert lib.ssde_ode_state(h, None, C.c_void_p(dl.data_ptr()), None) != 0 and b"sampler plan" in lib.ssde_last_error()
    assert lib.ssde_pc_run(h, 1, 0, None) != 0                          # an ODE plan is no sampler plan ...
    unet = X.LoadedPlan(X.export_unet_plan(E.UNetEngine(model, 2, 16, 16, torch.device("cpu"))))
    assert lib.ssde_ode_reset(unet.handle, C.c_void_p(z.data_ptr()), None, None) != 0 and b"not an ODE plan" in lib.ssde_last_error()
    assert lib.ssde_ode_solve(unet.handle, t0, t1, tol, tol, X._ode_callback(sc), None, 0, 0, None, None) != 0
    assert b"not an ODE plan" in lib.ssde_last_error()                  # ... and a U-Net plan is no ODE plan
    unet.close()
    with pytest.raises(TypeError):
        X.export_ode_plan(object())
