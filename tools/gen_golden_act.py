#!/usr/bin/env python
"""Generate the fixtures of the elu / relu / lrelu tests under tests/golden/ by running the REFERENCE implementation on CPU.

    python tools/gen_golden_act.py        # needs the reference checkout oracle/gen_golden.py names; writes tests/golden/

The reference is imported from a scratch copy the way oracle/gen_golden.py does it; weights are never stored (both sides seed
them with tests/_util.load_seeded(model, seed=1)).  The cases are those of tests/_act_checks.py.  Written:
  unet_small_ncsnpp_{elu,relu,lrelu}.npz   x, cond, y of one forward of _util.small_config() with config.model.nonlinearity overridden
  unet_small_ddpmpp_elu.npz                the same for the DDPM++ shape of unet_small_ddpmpp.npz
  train_small_elu.npz                      the continuous VE loss on the small NCSN++ network with ELU and dropout 0.1: loss and
                                           gradients of the first batch (<name>/grad_loss, <name>/gnorms, <name>/g/<parameter>),
                                           then three steps of the reference's get_step_fn and its eval step -- the layout of
                                           train_small_ddpm.npz
Dropout: the reference's nn.Dropout draws from torch's generator, which no other implementation can replay.  Every Dropout_0 of
the reference model is replaced by the package's mask (tests/_act_checks.hash_dropout: a pure function of the seed word, the
block's salt and the element index, restated in numpy by tests/_train_checks.hash_keep), with the seed words the fused step uses.
"""
import os
import sys
import types

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
    import _act_checks as A
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

    # ---- 1. forwards
    for name in A.FORWARD_CASES:
        cfg = A.forward_config(name)
        cfg.device = torch.device("cpu")
        torch.manual_seed(0)
        model = ref_mutils.get_model("ncsnpp")(ref_cfg_like(cfg)).eval()
        assert type(model.act).__name__ == {"elu": "ELU", "relu": "ReLU", "lrelu": "LeakyReLU"}[A.FORWARD_CASES[name][1]]
        sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model, seed=1), model)
        missing = model.load_state_dict(sd, strict=False)
        assert set(missing.missing_keys) <= {"sigmas"} and not missing.unexpected_keys, missing
        x, cond = A.forward_inputs(name)
        with torch.no_grad():
            y = model(x, cond)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, x=x.numpy(), cond=cond.numpy(), y=y.numpy())
        assert os.path.getsize(path) < 2 ** 20
        print("%-26s out absmax %.4g, %d bytes" % (name, float(y.abs().max()), os.path.getsize(path)))

    # ---- 2. training: loss and gradients of the first batch, then the reference's own steps
    name, case = A.TRAIN_NAME, A.TRAIN_CASE
    cfg = A.train_config()
    cfg.device = torch.device("cpu")
    rcfg = ref_cfg_like(cfg)
    torch.manual_seed(0)
    model = ref_mutils.create_model(rcfg)
    sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model.module, seed=1), model.module)
    model.module.load_state_dict(sd, strict=False)
    holder = types.SimpleNamespace(seed=0)
    n_blocks = A.hash_dropout(model.module, A.TRAIN_DROPOUT, holder)
    sde = _util.train_case_sde(ref_sde_lib, case, rcfg)
    _, _, _, continuous, reduce_mean, lw = case
    params = [(n, p) for n, p in model.module.named_parameters() if p.requires_grad]
    names_ = [n for n, _ in params]
    init = {n: p.detach().clone() for n, p in params}
    probes = _util.train_probe_names([(n, tuple(init[n].shape)) for n in names_], limit=A.TRAIN_PROBE_LIMIT)
    inputs = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)
    out = {}
    loss_fn = ref_losses.get_sde_loss_fn(sde, train=True, reduce_mean=reduce_mean, continuous=continuous, likelihood_weighting=lw)
    batch, u, labels, z = inputs[0]
    holder.seed = A.GRAD_SEED
    with _util.inject_rng(u, labels, z):
        loss0 = loss_fn(model, batch)
    loss0.backward()
    loss0 = loss0.detach()
    out[name + "/grad_loss"] = np.asarray(float(loss0), dtype=np.float64)
    out[name + "/gnorms"] = np.asarray([float(p.grad.double().norm()) for _, p in params], dtype=np.float64)
    for n, p in params:
        if n in probes:
            out["%s/g/%s" % (name, n)] = p.grad.detach().numpy().copy()
    model.zero_grad()
    optimizer = ref_losses.get_optimizer(rcfg, model.parameters())
    ema = ref_ema.ExponentialMovingAverage(model.parameters(), decay=rcfg.model.ema_rate)
    state = dict(optimizer=optimizer, model=model, ema=ema, step=0)
    optimize_fn = ref_losses.optimization_manager(rcfg)
    kw = dict(optimize_fn=optimize_fn, reduce_mean=reduce_mean, continuous=continuous, likelihood_weighting=lw)
    train_step = ref_losses.get_step_fn(sde, train=True, **kw)
    eval_step = ref_losses.get_step_fn(sde, train=False, **kw)
    losses_, norms, ema_norms = [], [], []
    for step in range(_util.TRAIN_STEPS):
        batch, u, labels, z = inputs[step]
        holder.seed = A.step_seed(step)
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
    path = os.path.join(out_dir, "train_small_elu.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 20, os.path.getsize(path)
    print("training (%d blocks with the hashed mask): gradient-case loss %.6g, losses %s eval %.6g, %d tensors, %d probes, %.2f MB"
          % (n_blocks, float(loss0), " ".join("%.6g" % v for v in losses_), float(eval_loss), len(names_), len(probes),
             os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
