"""Cases of the `ddpm` model family shared by tools/gen_golden_ddpm.py (which runs the reference) and the tests."""
import torch

import _util
from score_sde_pytorch_amd import configs as cfgs

# 32 GroupNorm groups of at least 4 channels force nf = 128
SMALL = dict(image_size=16, nf=128, ch_mult=(1, 2), num_res_blocks=1, attn=(8,))
FORWARD_BATCH = 2


def small_config(**model_overrides):
    kw = dict(nf=SMALL["nf"], ch_mult=SMALL["ch_mult"], num_res_blocks=SMALL["num_res_blocks"],
              attn_resolutions=SMALL["attn"], dropout=0.0)
    kw.update(model_overrides)
    cfg = cfgs.get_config("vp/ddpm/cifar10", **kw)
    cfg.data.image_size = SMALL["image_size"]
    return cfg


def forward_config(case):
    """configs of tests/golden/unet_<case>.npz"""
    if case == "small_ddpm":
        return small_config()
    return cfgs.get_config({"cifar_ddpm": "vp/ddpm/cifar10", "cifar_ddpm_uncond": "vp/ddpm/cifar10_unconditional"}[case])


FORWARD_CASES = ("small_ddpm", "cifar_ddpm", "cifar_ddpm_uncond")
STATE_DICT_CASES = {"small": small_config, "cifar10": lambda: cfgs.get_config("vp/ddpm/cifar10"),
                    "cifar10_unconditional": lambda: cfgs.get_config("vp/ddpm/cifar10_unconditional")}


def forward_inputs(cfg, batch=FORWARD_BATCH, seed=123):
    """centred data in [-1, 1) and integer-valued noise labels (the discrete VP loss and the ancestral sampler pass t (N - 1))"""
    g = torch.Generator().manual_seed(seed)
    R = cfg.data.image_size
    x = torch.rand(batch, 3, R, R, generator=g) * 2 - 1 + 0.5 * torch.randn(batch, 3, R, R, generator=g)
    labels = torch.randint(0, 1000, (batch,), generator=g).float()
    return x, labels


# the sampler case: vp/ddpm/cifar10's own sampler (ancestral sampling, no corrector, discrete labels) for 10 steps.
# beta_max = 5: the discrete betas of beta_max = 20 exceed 1 at N = 10 (tests/_util.PC_VARIANTS has the same note)
PC_CASE = dict(config="vp/ddpm/cifar10", batch=4, sde_kwargs=dict(beta_min=0.1, beta_max=5.0, N=10), eps=1e-3, denoise=True,
               seed=29, steps_kept=(0, 4, 9))


def pc_inputs():
    return _util.pc_case_inputs(PC_CASE["batch"], PC_CASE["sde_kwargs"]["N"], sigma_max=1.0, size=32, seed=PC_CASE["seed"])


# the training case: the discrete VP (DDPM) loss of configs/vp/ddpm/cifar10.py on the small network, dropout 0
TRAIN_NAME = "ddpm_vp"
TRAIN_CASE = ("ddpm", {}, "vpsde", False, True, False)      # (kind, overrides, sde, continuous, reduce_mean, likelihood_weighting)
# probes stored in full: one tensor of every leaf class of at most this many elements (tests/_util.train_probe_names) -- 20 of
# the network's 22 classes (the 3x3 weights of 128 x 128 x 9 stay out).  The widest ones (Linear / Dense_0 / NIN at 256 channels,
# 65536 floats each) go three to a file into train_small_ddpm_probes<k>.npz so that no fixture passes 1 MiB.
TRAIN_PROBE_LIMIT = 65536
TRAIN_PROBE_FILE_ELEMS = 3 * 65536


class TrainGold:
    """train_small_ddpm.npz and its probe files read as one mapping (`files`, `[key]`), the interface of an NpzFile"""

    def __init__(self, golden_dir):
        import glob
        import os
        import numpy as np
        paths = [os.path.join(golden_dir, "train_small_ddpm.npz")] + sorted(glob.glob(os.path.join(golden_dir, "train_small_ddpm_probes*.npz")))
        self._parts = [np.load(p) for p in paths]
        self.files = [k for part in self._parts for k in part.files]
        assert len(set(self.files)) == len(self.files)

    def __getitem__(self, key):
        for part in self._parts:
            if key in part.files:
                return part[key]
        raise KeyError(key)


def train_config():
    cfg = small_config(num_scales=24)
    cfg.training.continuous = False
    cfg.optim.warmup = _util.TRAIN_WARMUP
    return cfg


def train_state(dev):
    from score_sde_pytorch_amd.models import ema as ema_mod
    from score_sde_pytorch_amd import losses, sde_lib
    _, _, _, continuous, reduce_mean, lw = TRAIN_CASE
    cfg = train_config()
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model("ddpm")(cfg)
    init = {k: v.clone() for k, v in _util.load_seeded(model, seed=1).items()}
    model = model.to(dev)
    sde = _util.train_case_sde(sde_lib, TRAIN_CASE, cfg)
    opt = losses.get_optimizer(cfg, model.parameters())
    ema = ema_mod.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    optimize_fn = losses.optimization_manager(cfg)
    kw = dict(optimize_fn=optimize_fn, reduce_mean=reduce_mean, continuous=continuous, likelihood_weighting=lw)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    return cfg, init, state, losses.get_step_fn(sde, train=True, **kw), losses.get_step_fn(sde, train=False, **kw)


def check_training_loss_and_gradients(dev):
    """the discrete VP loss on the first batch of the training case: loss, the norm of every parameter gradient and the probe
    tensors in full against the reference's loss.backward()"""
    from _train_checks import TOL_GRAD
    from _util import rel_err
    name = TRAIN_NAME
    gold = TrainGold(_util.GOLDEN)
    cfg, _, state, train_step, _ = train_state(dev)
    batch, u, labels, z = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)[0]
    fs = train_step.fused_for(state, batch.to(dev))
    assert fs is not None, "the fused training step must accept a DDPM model"
    loss = float(fs.loss_and_grads(batch.to(dev), t=labels.to(dev), z=z.to(dev)))
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
    print("ddpm training gradients: worst norm error %.3g over %d tensors, %d probes" % (worst, len(params), len(probes)))


def check_step_fn_against_reference_run(dev, graph_expected=None):
    """losses.get_step_fn(...)(state, batch), train and eval branches, against the reference's own three steps; the bounds are
    those of _train_checks.check_step_fn_against_reference_run.  graph_expected: whether the step must have run as a captured graph"""
    import _train_checks as T
    name = TRAIN_NAME
    gold = TrainGold(_util.GOLDEN)
    cfg, init, state, train_step, eval_step = train_state(dev)
    inputs = _util.train_case_inputs(name, cfg.model.num_scales, size=cfg.data.image_size)
    ref_loss = gold[name + "/loss"]
    for step in range(_util.TRAIN_STEPS):
        batch, u, labels, z = inputs[step]
        with _util.inject_rng(u, labels, z):
            loss = train_step(state, batch.to(dev))
        assert state["step"] == step + 1 and state["ema"].num_updates == step + 1
        assert abs(float(loss) - ref_loss[step]) <= 1e-5 * abs(ref_loss[step]), (step, float(loss), ref_loss[step])
        T._compare_with_reference_step(gold, name, step, state, init, last=step == _util.TRAIN_STEPS - 1)
    fs = train_step.fused_for(state, inputs[0][0].to(dev))
    if graph_expected is not None:
        assert (getattr(fs, "_graph", None) is not None) == graph_expected
    batch, u, labels, z = inputs[_util.TRAIN_STEPS]
    with _util.inject_rng(u, labels, z):
        eval_loss = eval_step(state, batch.to(dev))
    ref_eval = float(gold[name + "/eval_loss"])
    assert abs(float(eval_loss) - ref_eval) <= 1e-5 * abs(ref_eval), (float(eval_loss), ref_eval)
