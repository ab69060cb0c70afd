"""Cases of the any-length `fir_kernel` fixtures, shared by tools/gen_golden_fir.py (which runs the reference) and the tests."""
import os

import numpy as np
import torch

import _util

FIR_KERNELS = {"fir3": (1, 2, 1), "fir6": (1, 5, 10, 10, 5, 1)}
# tests/golden/unet_small_<fir>.npz holds "<net>/x", "<net>/cond", "<net>/y" of one forward per net: (config, batch)
FORWARD_NETS = {
    "ncsnpp": (lambda: _util.small_config("ncsnpp"), 2),
    # one sample: the 32 x 32 net's x and y of two would pass the largest forward fixture the suite has
    "ffhq": (lambda: _util.small_config("ffhq", image_size=32, ch_mult=(1, 1, 2), attn=(16,)), 1),
}


def forward_config(net, fir):
    cfg = FORWARD_NETS[net][0]()
    cfg.model.fir_kernel = list(FIR_KERNELS[fir])
    return cfg


def forward_inputs(cfg, batch, seed=123):
    """data in [0, 1) perturbed at noise levels drawn log-uniformly from [0.01, 50] (the recipe of oracle/gen_golden.py)"""
    g = torch.Generator().manual_seed(seed)
    R = cfg.data.image_size
    x = torch.rand(batch, 3, R, R, generator=g) if not cfg.data.centered else torch.rand(batch, 3, R, R, generator=g) * 2 - 1
    cond = torch.exp(torch.rand(batch, generator=g) * (np.log(50.0) - np.log(0.01)) + np.log(0.01)).float()
    return x + cond[:, None, None, None] * torch.randn(batch, 3, R, R, generator=g), cond


# tests/golden/train_small_fir6.npz: the continuous VE loss (configs/ve/cifar10_ncsnpp_continuous.py) on the small net with the
# 6-tap kernel, in the layout of train_small_ddpm.npz
TRAIN_NAME = "ve_cont_fir6"
TRAIN_FILE = "train_small_fir6.npz"
TRAIN_CASE = ("ncsnpp", dict(fir_kernel=list(FIR_KERNELS["fir6"])), "vesde", True, False, False)


def train_gold():
    return np.load(os.path.join(_util.GOLDEN, TRAIN_FILE))


def check_training_loss_and_gradients(dev, gold, name, case):
    """the loss on the first batch of a training case, the norm of every parameter gradient and the probe tensors in full,
    against the reference's loss.backward(): the checks and tolerances of _ddpm_util.check_training_loss_and_gradients, with
    the fixture, its entry and the case (a tests/_util.TRAIN_CASES tuple) as arguments"""
    import _train_checks as T
    from _train_checks import TOL_GRAD
    from _util import rel_err
    cfg, _, state, train_step, _ = T._reference_train_state(dev, case)
    batch, u, labels, z = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)[0]
    fs = train_step.fused_for(state, batch.to(dev))
    assert fs is not None, "the fused training step must accept this model"
    with _util.inject_rng(u, labels, z):          # the step's own draws (t from u or the labels, z), as the reference made them
        loss = float(fs.loss_and_grads(batch.to(dev)))
    ref_loss = float(gold[name + "/loss"][0])
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    params = [(n, p) for n, p in state["model"].named_parameters() if p.requires_grad]
    gnorms = gold[name + "/gnorms"]
    assert len(params) == gnorms.shape[0]
    worst = 0.0
    for (n, p), ref in zip(params, gnorms):
        got = float(fs.flat.grad_view(p).double().norm())
        if ref < 1e-4:                   # analytically-zero gradients (the key bias of attention): compared absolutely
            assert got < 1e-4, (n, got)
            continue
        worst = max(worst, abs(got - ref) / ref)
        assert abs(got - ref) <= TOL_GRAD * ref, (n, got, ref)
    probes = [k.split("/", 2)[2] for k in gold.files if k.startswith(name + "/g/")]
    assert len(probes) >= 10
    cur = dict(params)
    for n in probes:
        ref = torch.from_numpy(gold["%s/g/%s" % (name, n)])
        got = fs.flat.grad_view(cur[n]).cpu()
        if float(ref.abs().max()) < 1e-4:
            assert float((got - ref).abs().max()) < 1e-4, n
            continue
        assert rel_err(got, ref) < TOL_GRAD, (n, rel_err(got, ref))
    print("%s training gradients: worst norm error %.3g over %d tensors, %d probes" % (name, worst, len(params), len(probes)))


def check_step_fn_against_reference_run(dev, gold, name, case):
    """losses.get_step_fn(...)(state, batch), train and eval branches, against the reference's own three steps: the checks and
    bounds of _train_checks.check_step_fn_against_reference_run with the fixture, its entry and the case as arguments"""
    import _train_checks as T
    cfg, init, state, train_step, eval_step = T._reference_train_state(dev, case)
    inputs = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)
    ref_loss = gold[name + "/loss"]
    for step in range(_util.TRAIN_STEPS):
        batch, u, labels, z = inputs[step]
        with _util.inject_rng(u, labels, z):
            loss = train_step(state, batch.to(dev))
        assert state["step"] == step + 1 and state["ema"].num_updates == step + 1
        assert abs(float(loss) - ref_loss[step]) <= 1e-5 * abs(ref_loss[step]), (name, step, float(loss), ref_loss[step])
        T._compare_with_reference_step(gold, name, step, state, init, last=step == _util.TRAIN_STEPS - 1)
    assert int(gold[name + "/num_updates"]) == state["ema"].num_updates
    batch, u, labels, z = inputs[_util.TRAIN_STEPS]
    with _util.inject_rng(u, labels, z):
        eval_loss = eval_step(state, batch.to(dev))
    ref_eval = float(gold[name + "/eval_loss"])
    assert abs(float(eval_loss) - ref_eval) <= 1e-5 * abs(ref_eval), (name, float(eval_loss), ref_eval)
    assert state["step"] == _util.TRAIN_STEPS and state["ema"].num_updates == _util.TRAIN_STEPS
