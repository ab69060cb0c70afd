#!/usr/bin/env python
"""Evaluations and wall seconds of the probability-flow ODE sampler and the likelihood per `method`, device driver
(ode.solve_rk) against the host path (SSDE_HOST_ODE=1: scipy.integrate.solve_ivp around the same fused right-hand side).

    python tools/ode_method_times.py [--repeat 3]          # needs the GPU; prints one line per (run, method, driver)

The case is the tests' (tests/_util.ODE_CASE: sub-VP DDPM++ down-sized, batch 2, 16 px, seeded weights), at the tolerances
of tests/golden/ode_methods_small.npz (RK23 sampler 1e-4, DOP853 sampler 1e-5, likelihoods 1e-3) and RK45 at 1e-5 / 1e-3.
One untimed call per (run, method, driver) first: it lowers the right-hand side and captures its graph.  The time is the
best of `--repeat` calls, synchronised.  A network this small spends its time in launches and host work, so the numbers say
what the host round trip of every evaluation costs here and nothing about kernels at CIFAR size.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _util                                            # noqa: E402

SAMPLER = (("RK23", 1e-4), ("RK45", 1e-5), ("DOP853", 1e-5))
LIKELIHOOD = (("RK23", 1e-3), ("RK45", 1e-3), ("DOP853", 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import _train_checks as T
    from score_sde_pytorch_amd import sampling, likelihood, ode
    dev = "cuda"
    cfg, model, sde = T._ode_case_model(dev)
    z, data, epsilon = (t.to(dev) for t in _util.ode_case_inputs())
    case, inv = _util.ODE_CASE, _util.ode_inverse_scaler
    real = torch.randint_like
    torch.randint_like = lambda t, low=0, high=2, **kw: ((epsilon + 1.) / 2.).to(t.device)

    def timed(call):
        call()
        best, out = None, None
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, out

    try:
        for run, table in (("sampler", SAMPLER), ("likelihood", LIKELIHOOD)):
            for method, tol in table:
                for driver in ("device", "host"):
                    os.environ["SSDE_HOST_ODE"] = "1" if driver == "host" else "0"
                    if run == "sampler":
                        fn = sampling.get_ode_sampler(sde, tuple(z.shape), inv, rtol=tol, atol=tol, method=method,
                                                      eps=case["sample_eps"], device=dev)
                        sec, (_, nfe) = timed(lambda: fn(model, z=z))
                    else:
                        fn = likelihood.get_likelihood_fn(sde, inv, rtol=tol, atol=tol, method=method, eps=case["lik_eps"])
                        sec, (_, _, nfe) = timed(lambda: fn(model, data))
                    assert ode.last_driver == driver and fn.last_path == "fused", (ode.last_driver, fn.last_path)
                    print("%-10s %-6s tol %g  %-6s  evaluations %5d  %8.3f s  %7.3f ms / evaluation"
                          % (run, method, tol, driver, nfe, sec, 1e3 * sec / nfe), flush=True)
    finally:
        torch.randint_like = real
        os.environ.pop("SSDE_HOST_ODE", None)


if __name__ == "__main__":
    main()
