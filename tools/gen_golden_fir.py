#!/usr/bin/env python
"""Generate the any-length `fir_kernel` fixtures under tests/golden/ by running the REFERENCE implementation on CPU.

    python tools/gen_golden_fir.py        # needs the reference checkout oracle/gen_golden.py names; writes tests/golden/

The reference is imported from a scratch copy the way oracle/gen_golden.py does it; weights are never stored (both sides seed
them with tests/_util.load_seeded(model, seed=1)).  Written (cases: tests/_fir_util.py):
  unet_small_fir3.npz, unet_small_fir6.npz   "<net>/x", "<net>/cond", "<net>/y" of one forward of the small NCSN++ net
                                             (resblock FIR up / down) and of the small FFHQ net (both image pyramids and
                                             the FIR in front of the stride-2 convolution), fir_kernel (1,2,1) / (1,5,10,10,5,1)
  train_small_fir6.npz                       loss, gradients and three optimizer steps of the continuous VE loss on the 6-tap
                                             small net, in the layout of train_small_ddpm.npz
The script asserts that oracle/unet_oracle.ncsnpp_forward reproduces every stored forward to 1e-6.
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
    import _fir_util as F
    from oracle import unet_oracle
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
    for fir in F.FIR_KERNELS:
        out = {}
        for net, (_, batch) in F.FORWARD_NETS.items():
            cfg = F.forward_config(net, fir)
            cfg.device = torch.device("cpu")
            torch.manual_seed(0)
            model = ref_mutils.get_model("ncsnpp")(ref_cfg_like(cfg)).eval()
            sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model, seed=1), model)
            missing = model.load_state_dict(sd, strict=False)
            assert set(missing.missing_keys) <= {"sigmas"} and not missing.unexpected_keys, missing
            x, cond = F.forward_inputs(cfg, batch)
            with torch.no_grad():
                y = model(x, cond)
                full_sd = dict(sd); full_sd["sigmas"] = model.sigmas
                y_orc = unet_oracle.ncsnpp_forward(cfg, full_sd, x, cond)
            err = float((y - y_orc).abs().max() / y.abs().max())
            print("%-6s %-8s out absmax %.4g  oracle-vs-reference rel err %.3g" % (fir, net, float(y.abs().max()), err))
            assert err < 1e-6, err
            out.update({net + "/x": x.numpy(), net + "/cond": cond.numpy(), net + "/y": y.numpy()})
        path = os.path.join(out_dir, "unet_small_%s.npz" % fir)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 46375, os.path.getsize(path)       # unet_small_ncsnpp_attn32.npz, the largest forward fixture

    # ---- 2. training: loss and gradients of the first batch, then the reference's own steps
    name, case = F.TRAIN_NAME, F.TRAIN_CASE
    cfg = _util.train_case_config(case)
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
    probes = _util.train_probe_names([(n, tuple(init[n].shape)) for n in names_])
    inputs = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)
    out = {}
    loss_fn = ref_losses.get_sde_loss_fn(sde, train=True, reduce_mean=reduce_mean, continuous=continuous, likelihood_weighting=lw)
    batch, u, labels, z = inputs[0]
    with _util.inject_rng(u, labels, z):
        loss0 = loss_fn(model, batch)
    loss0.backward()
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
        with _util.inject_rng(u, labels, z):
            losses_.append(float(train_step(state, batch)))
        cur = dict(model.module.named_parameters())
        norms.append([[float(cur[n].detach().double().norm()), float((cur[n].detach() - init[n]).double().norm())] for n in names_])
        ema_norms.append([[float(s.double().norm()), float((s - init[n]).double().norm())] for s, n in zip(ema.shadow_params, names_)])
    assert abs(losses_[0] - float(loss0)) <= 1e-6 * abs(float(loss0))
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
    path = os.path.join(out_dir, F.TRAIN_FILE)
    np.savez_compressed(path, **out)
    import glob
    others = [q for q in glob.glob(os.path.join(out_dir, "train_small*.npz")) if q != path]
    assert os.path.getsize(path) < min(2 ** 20, max(os.path.getsize(q) for q in others)), os.path.getsize(path)
    print("training: losses %s eval %.6g, %d tensors, %d probes, %.2f MB"
          % (" ".join("%.6g" % v for v in losses_), float(eval_loss), len(names_), len(probes), os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
