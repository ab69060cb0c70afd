#!/usr/bin/env python
"""Generate the fixtures of the channel-count tests under tests/golden/ by running the REFERENCE implementation on CPU.

    python tools/gen_golden_channels.py    # needs the reference checkout oracle/gen_golden.py names; writes tests/golden/

The reference is imported from a scratch copy the way oracle/gen_golden.py does it, unpatched; weights are never stored (both sides
seed them with tests/_util.load_seeded(model, seed=1)).  The cases are those of tests/_chan_cases.py: config.data.num_channels =
1, 2, 4, 6, 8, 13 and 20 on the small NCSN++ / DDPM++ / FFHQ / 'cat' networks and on the `ddpm` family.  Written:
  chan_state_dict_names.json   the reference's state-dict names and shapes per case
  unet_chan_<case>.npz         x, cond, y of one forward
  train_chan_<case>.npz        the training cases: loss and gradients of the continuous loss on the first batch
                               (<case>/grad_loss, <case>/gnorms, <case>/g/<parameter>: the layout of train_arch_<case>.npz),
                               and <case>/cot, <case>/dx = autograd.grad(sum(y * cot), x) on the forward case's inputs
"""
import json
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
    import _chan_cases as K
    import models.utils as ref_mutils            # noqa  (reference)
    import models.ncsnpp                         # noqa  registers 'ncsnpp' in the reference registry
    import models.ddpm                           # noqa  registers 'ddpm'
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

    def seed_weights(model):
        sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model, seed=1), model)
        missing = model.load_state_dict(sd, strict=False)
        assert set(missing.missing_keys) <= {"sigmas"} and not missing.unexpected_keys, missing

    # ---- 1. state-dict names and one forward per case
    names = {}
    for case in K.FORWARD_CASES:
        cfg = K.config(case)
        cfg.device = torch.device("cpu")
        torch.manual_seed(0)
        model = ref_mutils.get_model(K.family(case))(ref_cfg_like(cfg)).eval()
        names[case] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        seed_weights(model)
        x, cond = K.forward_inputs(case)
        assert x.shape[1] == K.channels(case)
        with torch.no_grad():
            y = model(x, cond)
        assert y.shape == x.shape and bool(torch.isfinite(y).all()), case
        path = os.path.join(out_dir, "unet_chan_%s.npz" % case)
        np.savez_compressed(path, x=x.numpy(), cond=cond.numpy(), y=y.numpy())
        assert os.path.getsize(path) < 2 ** 20
        print("%-12s %3d tensors, out absmax %.4g, %d bytes" % (case, len(names[case]), float(y.abs().max()), os.path.getsize(path)))
    path = os.path.join(out_dir, "chan_state_dict_names.json")
    with open(path, "w") as f:
        json.dump(names, f)
    assert os.path.getsize(path) < 2 ** 20

    # ---- 2. training cases: loss and parameter gradients of the first batch, and the input gradient of the forward case
    for case in K.TRAIN_CASES:
        tc = K.train_case(case)
        cfg = K.train_config(case)
        cfg.device = torch.device("cpu")
        rcfg = ref_cfg_like(cfg)
        torch.manual_seed(0)
        model = ref_mutils.create_model(rcfg)
        seed_weights(model.module)
        sde = _util.train_case_sde(ref_sde_lib, tc, rcfg)
        params = [(n, p) for n, p in model.module.named_parameters() if p.requires_grad]
        probes = _util.train_probe_names([(n, tuple(p.shape)) for n, p in params], limit=K.TRAIN_PROBE_LIMIT)
        batch, u, labels, z = K.train_inputs(case)[0]
        loss_fn = ref_losses.get_sde_loss_fn(sde, train=True, reduce_mean=False, continuous=True, likelihood_weighting=False)
        with _util.inject_rng(u, labels, z):
            loss0 = loss_fn(model, batch)
        loss0.backward()
        out = {case + "/grad_loss": np.asarray(float(loss0.detach()), dtype=np.float64),
               case + "/gnorms": np.asarray([float(p.grad.double().norm()) for _, p in params], dtype=np.float64)}
        for n, p in params:
            if n in probes:
                out["%s/g/%s" % (case, n)] = p.grad.detach().numpy().copy()
        model.zero_grad()
        model.eval()
        x, cond = K.forward_inputs(case)
        cot = K.cotangent(case)
        xg = x.clone().requires_grad_()
        dx, = torch.autograd.grad((model.module(xg, cond) * cot).sum(), xg)
        out[case + "/cot"], out[case + "/dx"] = cot.numpy(), dx.numpy()
        path = os.path.join(out_dir, "train_chan_%s.npz" % case)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 2 ** 20, os.path.getsize(path)
        print("training %-10s loss %.6g, %d tensors, %d probes, |dx| max %.4g, %.2f MB"
              % (case, float(loss0), len(params), len(probes), float(dx.abs().max()), os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
