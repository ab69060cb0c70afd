#!/usr/bin/env python
"""Generate the fixtures of the long-attention tests under tests/golden/ by running the REFERENCE implementation on CPU.

    python tools/gen_golden_attn_long.py     # needs the reference checkout oracle/gen_golden.py names; writes tests/golden/

Networks (tests/_attn_long_util.py): the small NCSN++ net at 32 px with attn_resolutions = (32, 16) -- AttnBlockpp over
L = 1024 tokens at C = 32 and L = 256 at C = 64 -- and the small DDPM net at 32 px with AttnBlock at 32 x 32 (L = 1024,
C = 128).  Weights are never stored (both sides seed them with tests/_util.load_seeded(model, seed=1)).  Written:
  unet_small_ncsnpp_attn32.npz    x, cond, y of one forward of the reference
  unet_small_ddpm_attn32.npz      the same for the DDPM net
  train_small_attn32.npz          three steps of the reference's get_step_fn on the NCSN++ net (losses, per-tensor parameter /
                                  update norms of the raw and the EMA weights, probe tensors) and its eval step: the layout
                                  of train_small.npz
The script also asserts that oracle.unet_oracle.ncsnpp_forward and tests/_ddpm_oracle.ddpm_forward reproduce the stored
forwards at 2e-5, so that the tests may take gradients from autograd through the oracle and store none.
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


def main():
    G.import_reference()
    import _util
    import _attn_long_util as A
    import _ddpm_oracle
    from oracle import unet_oracle
    import models.utils as ref_mutils            # noqa  (reference)
    import models.ncsnpp                         # noqa  registers 'ncsnpp' in the reference registry
    import models.ddpm                           # noqa  registers 'ddpm'
    import models.ema as ref_ema                 # noqa
    import sde_lib as ref_sde_lib                # noqa
    import losses as ref_losses                  # noqa
    import ml_collections

    out_dir = os.path.join(ROOT, "tests", "golden")
    torch.set_num_threads(min(16, os.cpu_count()))

    def ref_cfg_like(cfg):
        def conv(v):
            if hasattr(v, "items"):
                d = ml_collections.ConfigDict()
                for k, x in v.items():
                    d[k] = conv(x)
                return d
            return v
        return conv(cfg)

    # ---- 1. forwards
    cases = [("ncsnpp", A.small_config(), A.forward_inputs, unet_oracle.ncsnpp_forward, "unet_small_ncsnpp_attn32.npz"),
             ("ddpm", A.ddpm_config(), A.ddpm_inputs, _ddpm_oracle.ddpm_forward, "unet_small_ddpm_attn32.npz")]
    for family, cfg, make_inputs, oracle_fwd, fname in cases:
        cfg.device = torch.device("cpu")
        torch.manual_seed(0)
        model = ref_mutils.get_model(family)(ref_cfg_like(cfg)).eval()
        sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model, seed=1), model)
        missing = model.load_state_dict(sd, strict=False)
        assert set(missing.missing_keys) <= {"sigmas"} and not missing.unexpected_keys, missing
        full_sd = dict(sd); full_sd["sigmas"] = model.sigmas
        x, cond = make_inputs(cfg)
        with torch.no_grad():
            y = model(x, cond)
            y_orc = oracle_fwd(cfg, full_sd, x, cond)
        err = float((y - y_orc).abs().max() / y.abs().max())
        print("%-32s out absmax %.4g  oracle-vs-reference rel err %.3g" % (fname, float(y.abs().max()), err))
        assert err < 2e-5, err
        np.savez_compressed(os.path.join(out_dir, fname), x=x.numpy(), cond=cond.numpy(), y=y.numpy())

    # ---- 2. training: the reference's own steps on the NCSN++ net
    name, case = A.TRAIN_NAME, A.TRAIN_CASE
    cfg = A.train_config()
    cfg.device = torch.device("cpu")
    rcfg = ref_cfg_like(cfg)
    torch.manual_seed(0)
    model = ref_mutils.create_model(rcfg)
    sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model.module, seed=1), model.module)
    model.module.load_state_dict(sd, strict=False)
    sde = _util.train_case_sde(ref_sde_lib, case, rcfg)
    _, _, _, continuous, reduce_mean, lw = case
    params = [(n, p) for n, p in model.module.named_parameters() if p.requires_grad]
    names_ = [n for n, _ in params]
    init = {n: p.detach().clone() for n, p in params}
    probes = _util.train_probe_names([(n, tuple(init[n].shape)) for n in names_], limit=A.TRAIN_PROBE_LIMIT)
    inputs = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)
    optimizer = ref_losses.get_optimizer(rcfg, model.parameters())
    ema = ref_ema.ExponentialMovingAverage(model.parameters(), decay=rcfg.model.ema_rate)
    state = dict(optimizer=optimizer, model=model, ema=ema, step=0)
    optimize_fn = ref_losses.optimization_manager(rcfg)
    kw = dict(optimize_fn=optimize_fn, reduce_mean=reduce_mean, continuous=continuous, likelihood_weighting=lw)
    train_step = ref_losses.get_step_fn(sde, train=True, **kw)
    eval_step = ref_losses.get_step_fn(sde, train=False, **kw)
    out, losses_, norms, ema_norms = {}, [], [], []
    for step in range(_util.TRAIN_STEPS):
        batch, u, labels, z = inputs[step]
        with _util.inject_rng(u, labels, z):
            losses_.append(float(train_step(state, batch)))
        cur = dict(model.module.named_parameters())
        norms.append([[float(cur[n].detach().double().norm()), float((cur[n].detach() - init[n]).double().norm())] for n in names_])
        ema_norms.append([[float(s.double().norm()), float((s - init[n]).double().norm())] for s, n in zip(ema.shadow_params, names_)])
    for n in probes:
        out["%s/p/%s" % (name, n)] = cur[n].detach().numpy().copy()
        out["%s/e/%s" % (name, n)] = ema.shadow_params[names_.index(n)].numpy().copy()
    batch, u, labels, z = inputs[_util.TRAIN_STEPS]
    with _util.inject_rng(u, labels, z):
        eval_loss = eval_step(state, batch)
    out[name + "/loss"] = np.asarray(losses_, dtype=np.float64)
    out[name + "/eval_loss"] = np.asarray(float(eval_loss), dtype=np.float64)
    out[name + "/norms"] = np.asarray(norms, dtype=np.float64)
    out[name + "/ema_norms"] = np.asarray(ema_norms, dtype=np.float64)
    out[name + "/num_updates"] = np.asarray(ema.num_updates)
    path = os.path.join(out_dir, "train_small_attn32.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 20, os.path.getsize(path)
    print("training: losses %s eval %.6g, %d tensors, %d probes, %.2f MB"
          % (" ".join("%.6g" % v for v in losses_), float(eval_loss), len(names_), len(probes), os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
