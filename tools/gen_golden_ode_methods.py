#!/usr/bin/env python
"""Generate tests/golden/ode_methods_small.npz by running the REFERENCE's probability-flow ODE sampler and likelihood
with `method='RK23'` and `method='DOP853'` on CPU.

    python tools/gen_golden_ode_methods.py   # needs the reference checkout oracle/gen_golden.py names (~5 min of CPU)

Network, SDE and inputs are those of tests/golden/ode_small.npz (oracle/gen_golden_ode.py: _util.ODE_CASE and
ode_case_inputs(), latent injected through `z=`, Hutchinson probe through a patched torch.randint_like).  What runs is the
reference's own `sampling.get_ode_sampler` and `likelihood.get_likelihood_fn`; their `method` goes straight to
scipy.integrate.solve_ivp.  Stored per run <tag> in RUNS: the output, the evaluation count, and how far the output moves
when the input is scaled by (1 + 1e-6) -- the conditioning the GPU tests' tolerances are stated against:
  <tag>_samples, <tag>_nfe, <tag>_sens, <tag>_sens_nfe                         sampler runs (denoise=False)
  <tag>_bpd, <tag>_z, <tag>_nfe, <tag>_sens_bpd, <tag>_sens_z, <tag>_sens_nfe  likelihood runs
  <tag>_tol                                                                    rtol = atol of the run
The script asserts that oracle/ode_oracle.py with the same `method` reproduces every stored output, with the bounds of
oracle/gen_golden_ode.py.  Data only; weights are never stored (both sides seed them).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G                                  # noqa: E402

# tag -> (kind, method, rtol = atol)
RUNS = {"ode_rk23": ("sample", "RK23", 1e-4), "ode_dop853": ("sample", "DOP853", 1e-5),
        "lik_rk23": ("likelihood", "RK23", 1e-3), "lik_dop853": ("likelihood", "DOP853", 1e-3)}


def main():
    G.import_reference()
    import _util
    from oracle import ode_oracle
    import models.utils as ref_mutils            # noqa  (reference)
    import models.ncsnpp                         # noqa
    import sde_lib as ref_sde_lib                # noqa
    import sampling as ref_sampling              # noqa
    import likelihood as ref_likelihood          # noqa
    import ml_collections

    def ref_cfg_like(cfg):
        def conv(v):
            if hasattr(v, "items"):
                d = ml_collections.ConfigDict()
                for k, x in v.items():
                    d[k] = conv(x)
                return d
            return v
        return conv(cfg)

    torch.set_num_threads(min(16, os.cpu_count()))
    case = _util.ODE_CASE
    cfg = _util.small_config("ddpmpp")
    cfg.device = torch.device("cpu")
    torch.manual_seed(0)
    ref_model = ref_mutils.get_model("ncsnpp")(ref_cfg_like(cfg)).eval()
    sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(ref_model, seed=1), ref_model)
    ref_model.load_state_dict(sd, strict=False)
    full_sd = dict(sd)
    full_sd["sigmas"] = ref_model.sigmas
    kw = case["sde_kwargs"]
    sde = ref_sde_lib.subVPSDE(**kw)
    z, data, epsilon = _util.ode_case_inputs()
    shape = tuple(z.shape)
    inv = _util.ode_inverse_scaler
    out = {}

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    for tag, (kind, method, tol) in RUNS.items():
        out[tag + "_tol"] = np.float64(tol)
        if kind == "sample":
            smp = ref_sampling.get_ode_sampler(sde, shape, inv, denoise=False, rtol=tol, atol=tol, method=method,
                                               eps=case["sample_eps"], device="cpu")
            x, nfe = smp(ref_model, z=z.clone())
            xo, nfe_o = ode_oracle.ode_sample(cfg, full_sd, "subvpsde", kw, z.clone(), rtol=tol, atol=tol, method=method,
                                              eps=case["sample_eps"], denoise=False)
            e = rel(inv(xo), x)
            print("%-11s %-6s tol %g: nfe %d (oracle %d)  |x| max %.4g  oracle-vs-reference rel err %.3g"
                  % (tag, method, tol, nfe, nfe_o, float(x.abs().max()), e), flush=True)
            assert nfe == nfe_o and e < 1e-5, (tag, nfe, nfe_o, e)
            x2, nfe2 = smp(ref_model, z=z.clone() * (1 + 1e-6))
            out.update({tag + "_samples": x.numpy(), tag + "_nfe": np.int64(nfe), tag + "_sens": np.float64(rel(x2, x)),
                        tag + "_sens_nfe": np.int64(nfe2)})
            print("            conditioning: input x (1 + 1e-6) moves the samples by %.3g relative, nfe %d"
                  % (out[tag + "_sens"], nfe2), flush=True)
            continue
        real = torch.randint_like
        torch.randint_like = lambda t, low=0, high=2, **k: ((epsilon + 1.) / 2.).to(t.device)
        try:
            lf = ref_likelihood.get_likelihood_fn(sde, inv, hutchinson_type="Rademacher", rtol=tol, atol=tol, method=method,
                                                  eps=case["lik_eps"])
            bpd, zz, nfe = lf(ref_model, data.clone())
            bpd2, zz2, nfe2 = lf(ref_model, data.clone() * (1 + 1e-6))
        finally:
            torch.randint_like = real
        bo, zo, nfe_o = ode_oracle.likelihood(cfg, full_sd, "subvpsde", kw, data.clone(), epsilon, inv, rtol=tol, atol=tol,
                                              method=method, eps=case["lik_eps"])
        print("%-11s %-6s tol %g: nfe %d (oracle %d)  bpd %s  oracle-vs-reference: bpd %.3g  z %.3g"
              % (tag, method, tol, nfe, nfe_o, bpd.tolist(), rel(bo, bpd), rel(zo, zz)), flush=True)
        assert nfe == nfe_o and rel(bo, bpd) < 1e-5 and rel(zo, zz) < 1e-4, (tag, nfe, nfe_o)
        out.update({tag + "_bpd": bpd.numpy(), tag + "_z": zz.numpy(), tag + "_nfe": np.int64(nfe),
                    tag + "_sens_bpd": np.float64(rel(bpd2, bpd)), tag + "_sens_z": np.float64(rel(zz2, zz)),
                    tag + "_sens_nfe": np.int64(nfe2)})
        print("            conditioning: input x (1 + 1e-6) moves bpd by %.3g, the latent by %.3g relative, nfe %d"
              % (out[tag + "_sens_bpd"], out[tag + "_sens_z"], nfe2), flush=True)
    path = os.path.join(ROOT, "tests", "golden", "ode_methods_small.npz")
    np.savez_compressed(path, **out)
    print("written", path)


if __name__ == "__main__":
    main()
