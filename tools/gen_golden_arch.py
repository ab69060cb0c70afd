#!/usr/bin/env python
"""Generate the fixtures of the NCSN++ constructor-switch tests under tests/golden/ by running the REFERENCE implementation on CPU.

    python tools/gen_golden_arch.py        # needs the reference checkout oracle/gen_golden.py names; writes tests/golden/

The reference is imported from a scratch copy the way oracle/gen_golden.py does it, unpatched; weights are never stored (both sides
seed them with tests/_util.load_seeded(model, seed=1)).  The cases are those of tests/_arch_checks.py: resblock_type = 'ddpm',
progressive_combine = 'cat', and the residual input pyramid without FIR.  Written:
  ncsnpp_arch_state_dict_names.json   the reference's state-dict names and shapes per case
  unet_arch_<case>.npz                x, cond, y of one forward, inputs drawn as tests/_act_checks.forward_inputs draws them
  train_arch_<case>.npz               the training cases: loss and gradients of the continuous loss on the first batch
                                      (<case>/grad_loss, <case>/gnorms, <case>/g/<parameter>: the layout of train_small_ddpm.npz),
                                      and <case>/cot, <case>/dx = autograd.grad(sum(y * cot), x) on the forward case's inputs
The script asserts that the reference builds and runs every case of _arch_checks.CASES -- and that it builds the cases of
_arch_checks.UNRUNNABLE and raises on their first forward (every non-FIR layerspp.Upsample: F.interpolate(x, size, 'nearest') puts
the mode where scale_factor goes, models/layerspp.py:117).  Nothing is recorded for those, and the package's constructor refuses them.
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
    import _arch_checks as A
    import models.utils as ref_mutils            # noqa  (reference)
    import models.ncsnpp                         # noqa  registers 'ncsnpp' in the reference registry
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
    for case in A.CASES:
        cfg = A.config(case)
        cfg.device = torch.device("cpu")
        torch.manual_seed(0)
        model = ref_mutils.get_model("ncsnpp")(ref_cfg_like(cfg)).eval()
        names[case] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        seed_weights(model)
        x, cond = A.forward_inputs(case)
        with torch.no_grad():
            y = model(x, cond)
        assert bool(torch.isfinite(y).all()), case
        path = os.path.join(out_dir, "unet_arch_%s.npz" % case)
        np.savez_compressed(path, x=x.numpy(), cond=cond.numpy(), y=y.numpy())
        assert os.path.getsize(path) < 2 ** 20
        print("%-18s %3d tensors, out absmax %.4g, %d bytes" % (case, len(names[case]), float(y.abs().max()), os.path.getsize(path)))
    with open(os.path.join(out_dir, "ncsnpp_arch_state_dict_names.json"), "w") as f:
        json.dump(names, f)

    # ---- 1b. what the reference constructs but cannot run (A.UNRUNNABLE): the first forward raises in layerspp.Upsample.  A
    # reference that runs one of these makes this script fail: the case then belongs to A.CASES
    for case in A.UNRUNNABLE:
        cfg = A.config(case)
        cfg.device = torch.device("cpu")
        torch.manual_seed(0)
        model = ref_mutils.get_model("ncsnpp")(ref_cfg_like(cfg)).eval()
        x, cond = A.forward_inputs(case)
        try:
            with torch.no_grad():
                model(x, cond)
        except ValueError as e:
            assert "only one of size or scale_factor" in str(e), (case, e)
            print("%-18s the reference builds it and its forward raises: %s" % (case, e))
        else:
            raise AssertionError("the reference runs %s: record it (move it to _arch_checks.CASES)" % case)

    # ---- 2. training cases: loss and parameter gradients of the first batch, and the input gradient of the forward case
    for case in A.TRAIN_CASES:
        tc = A.train_case(case)
        cfg = A.train_config(case)
        cfg.device = torch.device("cpu")
        rcfg = ref_cfg_like(cfg)
        torch.manual_seed(0)
        model = ref_mutils.create_model(rcfg)
        seed_weights(model.module)
        sde = _util.train_case_sde(ref_sde_lib, tc, rcfg)
        params = [(n, p) for n, p in model.module.named_parameters() if p.requires_grad]
        probes = _util.train_probe_names([(n, tuple(p.shape)) for n, p in params], limit=A.TRAIN_PROBE_LIMIT)
        batch, u, labels, z = _util.train_case_inputs("arch_" + case, cfg.model.num_scales, size=cfg.data.image_size)[0]
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
        x, cond = A.forward_inputs(case)
        cot = A.cotangent(case)
        xg = x.clone().requires_grad_()
        dx, = torch.autograd.grad((model.module(xg, cond) * cot).sum(), xg)
        out[case + "/cot"], out[case + "/dx"] = cot.numpy(), dx.numpy()
        path = os.path.join(out_dir, "train_arch_%s.npz" % case)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 2 ** 20, os.path.getsize(path)
        print("training %-10s loss %.6g, %d tensors, %d probes, |dx| max %.4g, %.2f MB"
              % (case, float(loss0), len(params), len(probes), float(dx.abs().max()), os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
