#!/usr/bin/env python
"""Generate the fixtures of the GroupNorm-width tests under tests/golden/ by running the REFERENCE implementation on CPU.

    python tools/gen_golden_gn_width.py     # needs the reference checkout oracle/gen_golden.py names; writes tests/golden/

The network is the smallest one whose decoder has a GroupNorm of 6 channels per group: the FFHQ architecture at 32 px with
nf = 16, ch_mult = (1, 2, 4, 8), one block per level (tests/_gn_width_util.py); weights are never stored (both sides seed them
with tests/_util.load_seeded(model, seed=1)).  Written:
  unet_small_nf16.npz    x, cond, y of one forward of the reference
  train_small_nf16.npz   three steps of the reference's get_step_fn (losses, per-tensor parameter / update norms of the raw
                         and the EMA weights, probe tensors) and its eval step: the layout of train_small_ddpm.npz
The script also checks the two 1024-px presets against the reference's files and asserts that
oracle.unet_oracle.ncsnpp_forward reproduces the stored forward at 2e-5, with dropout = 0.0 and (eval mode) with the
dropout = 0.1 copy of the config, so that the tests may take gradients from autograd through the oracle and store none.
"""
import importlib
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
    import _gn_width_util as W
    from oracle import unet_oracle
    from score_sde_pytorch_amd import configs as my_cfgs
    import models.utils as ref_mutils            # noqa  (reference)
    import models.ncsnpp                         # noqa  registers 'ncsnpp' in the reference registry
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

    # ---- 1. the presets equal the reference's files
    for name in ["ve/ffhq_ncsnpp_continuous", "ve/celebahq_ncsnpp_continuous"]:
        ref = importlib.import_module("configs." + name.replace("/", ".")).get_config()
        mine = my_cfgs.get_config(name)
        for sec in ["training", "sampling", "eval", "data", "model", "optim"]:
            for k, v in ref[sec].items():
                if k == "tfrecords_path":
                    continue
                mv = mine[sec][k]
                same = (tuple(v) == tuple(mv)) if isinstance(v, (list, tuple)) else (v == mv)
                assert same, (name, sec, k, v, mv)
        assert ref["seed"] == mine["seed"]
        print("config preset ok:", name)

    # ---- 2. forward
    for dropout in (0.0, 0.1):
        cfg = W.small_config(dropout=dropout)
        cfg.device = torch.device("cpu")
        torch.manual_seed(0)
        model = ref_mutils.get_model("ncsnpp")(ref_cfg_like(cfg)).eval()
        sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model, seed=1), model)
        missing = model.load_state_dict(sd, strict=False)
        assert set(missing.missing_keys) <= {"sigmas"} and not missing.unexpected_keys, missing
        full_sd = dict(sd); full_sd["sigmas"] = model.sigmas
        x, sig = W.forward_inputs(cfg)
        with torch.no_grad():
            y = model(x, sig)
            y_orc = unet_oracle.ncsnpp_forward(cfg, full_sd, x, sig)
        err = float((y - y_orc).abs().max() / y.abs().max())
        print("unet_small_nf16 (dropout %.1f): out absmax %.4g  oracle-vs-reference rel err %.3g" % (dropout, float(y.abs().max()), err))
        assert err < 2e-5, err
        if dropout == 0.0:
            np.savez_compressed(os.path.join(out_dir, "unet_small_nf16.npz"), x=x.numpy(), cond=sig.numpy(), y=y.numpy())

    # ---- 3. training: the reference's own steps
    name, case = W.TRAIN_NAME, W.TRAIN_CASE
    cfg = W.train_config()
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
    probes = _util.train_probe_names([(n, tuple(init[n].shape)) for n in names_], limit=W.TRAIN_PROBE_LIMIT)
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
    path = os.path.join(out_dir, "train_small_nf16.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 20, os.path.getsize(path)
    print("training: losses %s eval %.6g, %d tensors, %d probes, %.2f MB"
          % (" ".join("%.6g" % v for v in losses_), float(eval_loss), len(names_), len(probes), os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
