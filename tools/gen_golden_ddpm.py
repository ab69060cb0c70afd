#!/usr/bin/env python
"""Generate the `ddpm` family's fixtures under tests/golden/ by running the REFERENCE implementation on CPU.

    python tools/gen_golden_ddpm.py        # needs the reference checkout oracle/gen_golden.py names; writes tests/golden/

The reference is imported from a scratch copy the way oracle/gen_golden.py does it; weights are never stored (both sides seed
them with tests/_util.load_seeded(model, seed=1)).  Written:
  unet_small_ddpm.npz, unet_cifar_ddpm.npz, unet_cifar_ddpm_uncond.npz   x, cond, y of one forward
  ddpm_state_dict_names.json                                            the reference's state-dict names and shapes
  pc_cifar_ddpm_n10.npz                                                 a 10-step ancestral-sampling trajectory, injected noise
  train_small_ddpm.npz (+ train_small_ddpm_probes<k>.npz)               loss, gradients and three optimizer steps of the
                                                                        discrete VP loss (the layout of train_small.npz plus
                                                                        <name>/gnorms and <name>/g/<parameter>)
The script also asserts that tests/_ddpm_oracle.py reproduces every stored forward.

One repair is made to the scratch copy: the reference's DDPM constructor only creates its module list inside `if
conditional:` and cannot build configs/vp/ddpm/cifar10_unconditional.py as published; the copy gets an empty list in front.
"""
import importlib
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


def repair_unconditional(scratch):
    path = os.path.join(scratch, "models", "ddpm.py")
    src = open(path).read()
    marker = "    if conditional:\n"
    if "    modules = []\n" + marker not in src:
        assert src.count(marker) == 1
        with open(path, "w") as f:
            f.write(src.replace(marker, "    modules = []\n" + marker))


def main():
    G.import_reference()
    repair_unconditional(G.SCRATCH)
    import _util
    import _ddpm_util as D
    import _ddpm_oracle
    from score_sde_pytorch_amd import configs as my_cfgs
    import models.utils as ref_mutils            # noqa  (reference)
    import models.ddpm                           # noqa  registers 'ddpm' in the reference registry
    import models.ema as ref_ema                 # noqa
    import sde_lib as ref_sde_lib                # noqa
    import sampling as ref_sampling              # noqa
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
    for name in ["cifar10", "cifar10_continuous", "cifar10_unconditional", "church", "bedroom", "celebahq"]:
        ref = importlib.import_module("configs.vp.ddpm." + name).get_config()
        mine = my_cfgs.get_config("vp/ddpm/" + name)
        for sec in ["training", "sampling", "eval", "data", "model", "optim"]:
            for k, v in ref[sec].items():
                if k == "tfrecords_path":
                    continue
                mv = mine[sec][k]
                same = (tuple(v) == tuple(mv)) if isinstance(v, (list, tuple)) else (v == mv)
                assert same, (name, sec, k, v, mv)
        print("config preset ok: vp/ddpm/" + name)

    def ref_model_of(cfg):
        cfg.device = torch.device("cpu")
        torch.manual_seed(0)
        model = ref_mutils.get_model("ddpm")(ref_cfg_like(cfg)).eval()
        sd = _util.fix_top_level_groupnorm(_util.seeded_state_dict(model, seed=1), model)
        missing = model.load_state_dict(sd, strict=False)
        assert set(missing.missing_keys) <= {"sigmas"} and not missing.unexpected_keys, missing
        full_sd = dict(sd); full_sd["sigmas"] = model.sigmas
        return model, full_sd

    # ---- 2. state-dict names and shapes
    names = {}
    for key, make in D.STATE_DICT_CASES.items():
        model, _ = ref_model_of(make())
        names[key] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(out_dir, "ddpm_state_dict_names.json"), "w") as f:
        json.dump(names, f)

    # ---- 3. forwards
    for case in D.FORWARD_CASES:
        cfg = D.forward_config(case)
        model, full_sd = ref_model_of(cfg)
        x, labels = D.forward_inputs(cfg)
        with torch.no_grad():
            y = model(x, labels)
            y_orc = _ddpm_oracle.ddpm_forward(cfg, full_sd, x, labels)
        err = float((y - y_orc).abs().max() / y.abs().max())
        print("%-20s out absmax %.4g  restatement-vs-reference rel err %.3g" % (case, float(y.abs().max()), err))
        assert err < 2e-5, err
        np.savez_compressed(os.path.join(out_dir, "unet_%s.npz" % case), x=x.numpy(), cond=labels.numpy(), y=y.numpy())

    # ---- 4. ancestral-sampling trajectory
    pc = D.PC_CASE
    cfg = my_cfgs.get_config(pc["config"])
    model, _ = ref_model_of(cfg)
    B, N = pc["batch"], pc["sde_kwargs"]["N"]
    sde = ref_sde_lib.VPSDE(**pc["sde_kwargs"])
    x_T, noises = D.pc_inputs()
    it = iter([noises[i, 1] for i in range(N)])
    real_randn_like = torch.randn_like
    torch.randn_like = lambda t, **kw: next(it).to(t.device)
    sde.prior_sampling = lambda shape: x_T.clone()
    traj = []
    real_pred = ref_sampling.shared_predictor_update_fn

    def spy_pred(x, t, **kw):
        xn, xm = real_pred(x, t, **kw)
        traj.append(xn.clone())
        return xn, xm
    ref_sampling.shared_predictor_update_fn = spy_pred
    try:
        sampler = ref_sampling.get_pc_sampler(sde, (B, 3, 32, 32), ref_sampling.AncestralSamplingPredictor,
                                              ref_sampling.NoneCorrector, lambda v: v, snr=0.16, n_steps=1,
                                              probability_flow=False, continuous=False, denoise=pc["denoise"], eps=pc["eps"],
                                              device="cpu")
        samples, nfe = sampler(model)
    finally:
        torch.randn_like = real_randn_like
        ref_sampling.shared_predictor_update_fn = real_pred
    assert next(it, None) is None and len(traj) == N and torch.isfinite(samples).all()
    print("ancestral sampling: nfe %d, |x| max %.4g" % (nfe, float(samples.abs().max())))
    np.savez_compressed(os.path.join(out_dir, "pc_cifar_ddpm_n10.npz"), samples=samples.numpy(),
                        **{"x_step%d" % k: traj[k].numpy() for k in pc["steps_kept"]})

    # ---- 5. training: loss and gradients of the first batch, then the reference's own steps
    name, case = D.TRAIN_NAME, D.TRAIN_CASE
    cfg = D.train_config()
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
    probes = _util.train_probe_names([(n, tuple(init[n].shape)) for n in names_], limit=D.TRAIN_PROBE_LIMIT)
    inputs = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)
    out = {}
    loss_fn = ref_losses.get_ddpm_loss_fn(sde, train=True, reduce_mean=reduce_mean)
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
    # the widest probes go a few to a file, so that no fixture passes 1 MiB
    wide = sorted(k for k, v in out.items() if v.size * 4 > D.TRAIN_PROBE_FILE_ELEMS)
    paths = [os.path.join(out_dir, "train_small_ddpm.npz")]
    np.savez_compressed(paths[0], **{k: v for k, v in out.items() if k not in wide})
    part, parts = {}, []
    for k in wide:
        if part and sum(v.size for v in part.values()) + out[k].size > D.TRAIN_PROBE_FILE_ELEMS:
            parts.append(part); part = {}
        part[k] = out[k]
    if part:
        parts.append(part)
    for i, part in enumerate(parts):
        paths.append(os.path.join(out_dir, "train_small_ddpm_probes%d.npz" % i))
        np.savez_compressed(paths[-1], **part)
    assert all(os.path.getsize(p) < 2 ** 20 for p in paths), [os.path.getsize(p) for p in paths]
    print("training: losses %s eval %.6g, %d tensors, %d probes, %d files, largest %.2f MB"
          % (" ".join("%.6g" % v for v in losses_), float(eval_loss), len(names_), len(probes), len(paths),
             max(os.path.getsize(p) for p in paths) / 1e6))


if __name__ == "__main__":
    main()
