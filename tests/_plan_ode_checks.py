"""Shared checks of the ODE plans (plan_export.export_ode_plan; include/ssde.h: ssde_ode_reset / ssde_ode_eval /
ssde_ode_solve / ssde_ode_state) for the emulator tests (test_plan_ode_cpu.py) and the device tests (test_plan_ode_gpu.py).

Network, SDE and inputs: _util.ODE_CASE / ode_case_inputs() -- sub-VP, batch 2, 16 px, the network behind
tests/golden/ode_small.npz.  `dev` is "cpu" (kernels on the emulator; the caller holds emu.emulated()) or "cuda".

The C driver and ode.solve_rk45 run the same programs and the same stage kernels with the same scalars (ode.scalars_fn);
they differ only in the rounding of the three norms of the initial step (torch's reduction order against the kernel's),
about 1e-16 relative.  The fixture's own sensitivities are `ode_sens` (1.7e-6 per 1e-6 of input change) and `lik_sens_*`
(x13 / x1300), so such a difference cannot reach 1e-6: DRIVER_TOL.  An accept / reject decision cannot flip either, but one
step (6 evaluations) of slack is allowed: DRIVER_NFE.  Equality is what is observed.

The emulator runs one evaluation of the sampler program in ~2 s and one of the likelihood program in ~5 s, hence the short
spans there (evaluation counts of ode.solve_rk45, recorded when the spans were chosen):
  SHORT_SAMPLE: t 1.0 -> 0.97 at rtol = atol = 1e-3: 26 evaluations (4 steps)
  SHORT_LIK:    t 1e-5 -> 0.05 at rtol = atol = 1e-3: 14 evaluations (2 steps)
"""
import functools
import os
import subprocess

import numpy as np
import torch

import _util

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c_host", "ode_host.c")
INC = os.path.join(_util.ROOT, "include")

DRIVER_TOL, DRIVER_NFE = 1e-6, 6
SAMPLE_TOL, SAMPLE_NFE = 1e-3, 12          # _train_checks.check_ode_sampler: samples 1e-3 relative, NFE within two steps
SHORT_SAMPLE = (1.0, 0.97, 1e-3)            # (t0, t1, rtol = atol)
SHORT_LIK = (1e-5, 0.05, 1e-3)


def gold():
    return np.load(os.path.join(_util.GOLDEN, "ode_small.npz"))


@functools.lru_cache(maxsize=None)
def case(dev):
    import _train_checks as T
    cfg, model, sde = T._ode_case_model(dev)
    z, data, eps = _util.ode_case_inputs()
    return cfg, model, sde, z.to(dev), data.to(dev), eps.to(dev)


def _mode():
    """the matrix mode the GPU tests are parametrised over is read when a program is lowered: part of every cache key"""
    return os.environ.get("SSDE_MATRIX", "")


def rhs_of(kind, dev):
    """(right-hand side, its blob)"""
    return _rhs_of(kind, dev, _mode())


@functools.lru_cache(maxsize=None)
def _rhs_of(kind, dev, mode):
    from score_sde_pytorch_amd import ode, plan_export
    cfg, model, sde, z, data, eps = case(dev)
    if kind == "sample":
        rhs = ode.FusedDrift(model, sde, z.shape, torch.device(dev))
    else:
        rhs = ode.FusedLikelihoodRhs(model, sde, data.shape, eps, torch.device(dev))
    return rhs, plan_export.export_ode_plan(rhs)


def plan_of(kind, dev):
    return _plan_of(kind, dev, _mode())


@functools.lru_cache(maxsize=None)
def _plan_of(kind, dev, mode):
    from score_sde_pytorch_amd import plan_export
    return plan_export.LoadedPlan(rhs_of(kind, dev)[1])


def start_of(kind, dev):
    """(x0 fp32 [B,C,H,W], probe or None)"""
    cfg, model, sde, z, data, eps = case(dev)
    return (z, None) if kind == "sample" else (data, eps)


def python_solve(kind, dev, t0, t1, tol):
    """ode.solve_rk45 around the same right-hand side: (state fp64 [n] or [n + B], evaluations); computed once"""
    return _python_solve(kind, dev, t0, t1, tol, _mode())


@functools.lru_cache(maxsize=None)
def _python_solve(kind, dev, t0, t1, tol, mode):
    from score_sde_pytorch_amd import ode
    rhs = rhs_of(kind, dev)[0]
    x0, probe = start_of(kind, dev)
    y0 = x0.reshape(-1).to(torch.float64)
    if probe is not None:
        rhs.set_probe(probe)
        y0 = torch.cat([y0, torch.zeros(x0.shape[0], dtype=torch.float64, device=y0.device)])
    if dev != "cpu":
        y, nfev = ode.integrate_ode(rhs, (t0, t1), y0, tol, tol, "RK45")
        torch.cuda.synchronize()
        return y, nfev
    stages = ode._HipStages(y0.numel(), y0, x32=rhs.x32, n32=rhs.n32)       # (integrate_ode sends host tensors to scipy)
    return ode.solve_rk45(rhs, (t0, t1), y0, rtol=tol, atol=tol, stages=stages)


def c_solve(kind, dev, t0, t1, tol, use_graph=False, max_nfev=0):
    """the same solve through LoadedPlan: (x fp32, delta_logp fp64 or None, evaluations)"""
    from score_sde_pytorch_amd import ode
    rhs, plan = rhs_of(kind, dev)[0], plan_of(kind, dev)
    x0, probe = start_of(kind, dev)
    stream = None
    if dev != "cpu":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        stream = side.cuda_stream
    plan.ode_reset(x0, probe, stream=stream)
    nfev = plan.ode_solve(t0, t1, tol, tol, ode.scalars_fn(rhs), use_graph=use_graph, max_nfev=max_nfev, stream=stream)
    x, dl = plan.ode_state(x0, stream=stream)
    if dev != "cpu":
        side.synchronize()
    return x, dl, nfev


def driver_differences(kind, x, dl, nfev, y_py, nfev_py):
    """(NFE difference, relative state difference, relative delta-logp difference or 0.0), printed for the record"""
    n = x.numel()
    d_x = _util.rel_err(x.reshape(-1), y_py[:n].to(torch.float32))
    d_l = _util.rel_err(dl, y_py[n:]) if dl is not None else 0.0
    print("ode plan [%s]: C driver nfev %d, Python driver nfev %d, state rel diff %.3g, delta_logp rel diff %.3g"
          % (kind, nfev, nfev_py, d_x, d_l))
    return abs(nfev - nfev_py), d_x, d_l


def assert_drivers_agree(kind, x, dl, nfev, y_py, nfev_py):
    d_n, d_x, d_l = driver_differences(kind, x, dl, nfev, y_py, nfev_py)
    assert torch.isfinite(x).all() and (dl is None or torch.isfinite(dl).all())
    assert d_n <= DRIVER_NFE, (nfev, nfev_py)
    assert d_x < DRIVER_TOL, d_x
    assert d_l < DRIVER_TOL, d_l


def build_c_host(tmp_path, emu_lib=None):
    """ode_host.c compiled with gcc: against the emulator library (-DHOST_IS_DEVICE) or libssde_hip.so + the HIP runtime"""
    from score_sde_pytorch_amd import _lib as L
    exe = str(tmp_path / ("ode_host_emu" if emu_lib else "ode_host"))
    if emu_lib:
        cmd = ["gcc", "-O1", "-std=c11", "-DHOST_IS_DEVICE", "-I", INC, SRC, "-o", exe, emu_lib, "-lm", "-Wl,-rpath," + os.path.dirname(emu_lib)]
    else:
        cmd = ["gcc", "-O1", "-std=c11", "-I", INC, "-I", "/opt/rocm/include", SRC, "-o", exe, L.LIB_PATH, "-L/opt/rocm/lib", "-lamdhip64",
               "-lm", "-Wl,-rpath," + os.path.dirname(L.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_c_host(exe, kind, dev, tmp_path, t0, t1, tol, use_graph, timeout):
    """one child process: (x fp32 [B,C,H,W] on the CPU, delta_logp fp64 [B] or None, evaluations, seconds of the solve)"""
    import re
    blob = rhs_of(kind, dev)[1]
    kw = _util.ODE_CASE["sde_kwargs"]
    x0, probe = start_of(kind, dev)
    f = {k: str(tmp_path / (kind + "_" + k)) for k in ("plan.blob", "x0.f32", "x.f32", "probe.f32", "dlogp.f64")}
    open(f["plan.blob"], "wb").write(blob)
    x0.cpu().numpy().astype(np.float32).tofile(f["x0.f32"])
    cmd = [exe, "sample" if kind == "sample" else "likelihood", f["plan.blob"], "subvp", repr(kw["beta_min"]), repr(kw["beta_max"]),
           repr(t0), repr(t1), repr(tol), str(int(use_graph)), f["x0.f32"], f["x.f32"]]
    if probe is not None:
        probe.cpu().numpy().astype(np.float32).tofile(f["probe.f32"])
        cmd += [f["probe.f32"], f["dlogp.f64"]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    m = re.search(r"nfev (\d+), solve ([0-9.]+) s", r.stdout)
    assert m, r.stdout
    print(r.stdout.strip())
    x = torch.from_numpy(np.fromfile(f["x.f32"], dtype=np.float32)).reshape(x0.shape)
    dl = torch.from_numpy(np.fromfile(f["dlogp.f64"], dtype=np.float64)) if probe is not None else None
    return x, dl, int(m.group(1)), float(m.group(2))
