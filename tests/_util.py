"""Shared test helpers: deterministic weights, small configs, tolerances."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from score_sde_pytorch_amd import configs as cfgs  # noqa: E402


def load_tool(name):
    """tools/<name>.py as a module: a test that recomputes a recorded fixture takes its cases from the tool that recorded it"""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def small_config(kind="ncsnpp", image_size=16, nf=32, ch_mult=(1, 2), num_res_blocks=1, attn=(8,)):
    """Down-sized variants of the BASELINE configs that keep every code path of the full ones."""
    base = {"ncsnpp": "ve/cifar10_ncsnpp_continuous", "ddpmpp": "subvp/cifar10_ddpmpp_continuous",
            "ffhq": "ve/ffhq_256_ncsnpp_continuous"}[kind]
    cfg = cfgs.get_config(base, nf=nf, ch_mult=tuple(ch_mult), num_res_blocks=num_res_blocks,
                          attn_resolutions=tuple(attn), dropout=0.0)
    cfg.data.image_size = image_size
    return cfg


def seeded_state_dict(model_or_shapes, seed=1):
    """Deterministic, non-degenerate weights for any ncsnpp-style state dict.

    The reference initialises the last conv of every block at scale 1e-10, which
    makes a random-init network an identity map; parity tests re-randomise EVERY tensor so that
    all branches carry signal.  Only torch's CPU generator is used, so the same seed gives the
    same weights in the build container (reference import) and on the GPU box.
    """
    shapes = model_or_shapes if isinstance(model_or_shapes, dict) else \
        {k: tuple(v.shape) for k, v in model_or_shapes.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in shapes.items():
        leaf = name.split(".")[-1]
        if name == "sigmas":
            continue
        if "GroupNorm" in name or (len(shape) == 1 and name.split(".")[-2].isdigit() and False):
            t = (1.0 + 0.1 * torch.randn(shape, generator=g)) if leaf == "weight" else 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1 and leaf == "W":           # Fourier frequencies
            t = torch.randn(shape, generator=g) * 16.0
        elif len(shape) == 1:                           # biases (and top-level GroupNorm handled below)
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            if leaf == "W":                             # NIN: [in, out]
                fan_in, fan_out = shape[0], shape[1]
            else:
                rf = int(np.prod(shape[2:])) if len(shape) > 2 else 1
                fan_in, fan_out = shape[1] * rf, shape[0] * rf
            bound = math.sqrt(3.0 / ((fan_in + fan_out) / 2.0))
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        out[name] = t.to(torch.float32)
    return out


def fix_top_level_groupnorm(sd, model):
    """Top-level nn.GroupNorm modules (all_modules.<i>.weight with 1-D shape) need scale ~1, not a bias-like draw."""
    import torch.nn as nn
    for i, m in enumerate(model.all_modules):
        if isinstance(m, nn.GroupNorm):
            sd["all_modules.%d.weight" % i] = 1.0 + sd["all_modules.%d.weight" % i]
    return sd


def load_seeded(model, seed=1):
    sd = fix_top_level_groupnorm(seeded_state_dict(model, seed), model)
    missing = model.load_state_dict(sd, strict=False)
    assert set(missing.missing_keys) <= {"sigmas"}, missing
    return sd


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def per_sample_err(a, b):
    """max over the batch of (max-abs error of a sample / max-abs of that sample's reference): a sample whose values are small
    next to the batch maximum cannot hide behind it (rel_err normalises by the maximum of the whole tensor)"""
    a, b = a.double().cpu().reshape(a.shape[0], -1), b.double().cpu().reshape(b.shape[0], -1)
    return float(((a - b).abs().amax(1) / (b.abs().amax(1) + 1e-30)).max())


# Trajectory yardsticks.  Measured on the MI355X against the reference run: pixel-MSE / max|x|^2 =
# 1.7e-15 .. 3.8e-15 and max-abs error / max|x| = 3.5e-7 .. 5e-7 at every step (profiles/r3_f4x4_trajectory_error_growth.txt,
# F(4x4,3x3) kernels, the coarsest-rounding mode).  The bounds sit ~10x above the observed max-abs error; the former
# 1e-8 max^2 yardstick could not fail (the state is dominated by the prior and the injected noise).
TRAJ_MSE = 1e-12
TRAJ_MAXABS = 5e-6


def assert_trajectory_close(x, ref, what=""):
    x, ref = x.double().cpu(), ref.double().cpu()
    mx = float(ref.abs().max())
    mse = float(((x - ref) ** 2).mean())
    assert mse <= TRAJ_MSE * mx ** 2, (what, "pixel MSE / max^2", mse / mx ** 2)
    err = float((x - ref).abs().max()) / mx
    assert err <= TRAJ_MAXABS, (what, "max-abs error / max", err)


def pc_variant_inputs(name, batch, n_steps, size, sigma_max):
    """x_T and injected noises of one entry of tests/golden/pc_small_variants.npz (oracle/gen_golden_variants.py)"""
    import zlib
    return pc_case_inputs(batch, n_steps, sigma_max, size, seed=zlib.crc32(name.encode()) & 0xffff)


def pc_case_inputs(batch=8, n_steps=10, sigma_max=50.0, size=32, seed=7):
    """x_T and injected noises of the PC-sampler golden case (BASELINE config #1); shared by
    oracle/gen_golden.py and the tests so the fixture need not store them."""
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(batch, 3, size, size, generator=g) * sigma_max
    noises = torch.randn(n_steps, 2, batch, 3, size, size, generator=g)
    return x_T, noises


# entries of tests/golden/pc_small_variants.npz (made by oracle/gen_golden_variants.py from the reference sampler):
# name -> (small-config kind, sde kind, sde kwargs, predictor, corrector, n_steps, continuous, probability_flow, denoise, eps)
PC_VARIANT_BATCH, PC_VARIANT_SIZE = 4, 16
# (the VP entries use beta_max=3: at N=6 the DDPM betas of beta_max=20 exceed 1 and sqrt(1-beta) is NaN)
PC_VARIANTS = {
    "ve_ancestral_ald": ("ncsnpp", "vesde", dict(sigma_min=0.01, sigma_max=50, N=6), "ancestral_sampling", "ald", 2, True, False, True, 1e-5),
    "ve_rd_none": ("ncsnpp", "vesde", dict(sigma_min=0.01, sigma_max=50, N=6), "reverse_diffusion", "none", 1, True, False, False, 1e-5),
    "ve_none_langevin": ("ncsnpp", "vesde", dict(sigma_min=0.01, sigma_max=50, N=6), "none", "langevin", 2, True, False, True, 1e-5),
    # (euler_maruyama with probability_flow=True raises TypeError in the reference: RSDE.sde returns a float diffusion,
    #  sde_lib.py:99 vs sampling.py:186 -- not a usable combination, so no entry)
    "ve_em_langevin": ("ncsnpp", "vesde", dict(sigma_min=0.01, sigma_max=50, N=6), "euler_maruyama", "langevin", 1, True, False, True, 1e-5),
    "vp_ancestral_ald_discrete": ("ddpmpp", "vpsde", dict(beta_min=0.1, beta_max=3, N=6), "ancestral_sampling", "ald", 1, False, False, True, 1e-3),
    "vp_em_langevin": ("ddpmpp", "vpsde", dict(beta_min=0.1, beta_max=3, N=6), "euler_maruyama", "langevin", 1, True, False, True, 1e-3),
    "vp_rd_langevin_discrete": ("ddpmpp", "vpsde", dict(beta_min=0.1, beta_max=3, N=6), "reverse_diffusion", "langevin", 1, False, False, False, 1e-3),
    "subvp_em_none": ("ddpmpp", "subvpsde", dict(beta_min=0.1, beta_max=20, N=6), "euler_maruyama", "none", 1, True, False, True, 1e-3),
    "subvp_rd_none_pflow": ("ddpmpp", "subvpsde", dict(beta_min=0.1, beta_max=20, N=6), "reverse_diffusion", "none", 1, True, True, True, 1e-3),
}


# entries of tests/golden/controllable_small.npz (oracle/gen_golden_controllable.py, from the reference's
# controllable_generation.py): name -> (task, variant of PC_VARIANTS supplying model / sde / predictor / corrector)
CONTROLLABLE_CASES = {
    "inpaint_ve_rd_langevin": ("inpaint", "ve_em_langevin", "reverse_diffusion", "langevin"),
    "inpaint_vp_ancestral_none": ("inpaint", "vp_ancestral_ald_discrete", "ancestral_sampling", "none"),
    "colorize_ve_rd_langevin": ("colorize", "ve_em_langevin", "reverse_diffusion", "langevin"),
    "colorize_subvp_em_none": ("colorize", "subvp_em_none", "euler_maruyama", "none"),
}


def controllable_inputs(name, batch, n_steps, size, sigma_max):
    """data (or grey-scale image), mask, prior sample and the four noise streams of a controllable-generation case"""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0xffff)
    data = torch.rand(batch, 3, size, size, generator=g)
    if name.startswith("colorize"):
        data = data.mean(dim=1, keepdim=True).repeat(1, 3, 1, 1)
    mask = torch.ones(batch, 3, size, size)
    mask[:, :, :, size // 2:] = 0.                     # right half unknown (the notebook's inpainting mask)
    prior = torch.randn(batch, 3, size, size, generator=g) * sigma_max
    noises = torch.randn(n_steps, 4, batch, 3, size, size, generator=g)
    return data, mask, prior, noises


# tests/golden/ode_small.npz (oracle/gen_golden_ode.py, from the reference's get_ode_sampler / get_likelihood_fn):
# BASELINE config #5's path (sub-VP DDPM++, RK45 rtol = atol = 1e-5) on the small DDPM++ network
ODE_CASE = dict(sde_kwargs=dict(beta_min=0.1, beta_max=20, N=1000), batch=2, size=16, rtol=1e-5, atol=1e-5,
                sample_eps=1e-3, lik_eps=1e-5, t_probe=0.37)


def ode_inverse_scaler(v):
    return (v + 1.) / 2.


def ode_case_inputs():
    """latent z (ode_sampler's argument), data in [-1, 1) and the Rademacher probe of the likelihood case"""
    g = torch.Generator().manual_seed(77)
    B, R = ODE_CASE["batch"], ODE_CASE["size"]
    z = torch.randn(B, 3, R, R, generator=g)
    data = torch.rand(B, 3, R, R, generator=g) * 2 - 1
    epsilon = torch.randint(0, 2, data.shape, generator=g).float() * 2 - 1.
    return z, data, epsilon


# tests/golden/train_small.npz + ref_checkpoint_small.pth (oracle/gen_golden_train.py, from the reference's losses.get_step_fn,
# optimization_manager, get_optimizer and models/ema.ExponentialMovingAverage run on CPU):
# name -> (small-config kind, config overrides, sde kind, continuous, reduce_mean, likelihood_weighting)
TRAIN_BATCH, TRAIN_STEPS, TRAIN_WARMUP = 3, 3, 2
TRAIN_CASES = {
    "ve_cont": ("ncsnpp", {}, "vesde", True, False, False),                       # configs/ve/cifar10_ncsnpp_continuous.py
    "subvp_cont": ("ddpmpp", {}, "subvpsde", True, False, False),                 # configs/subvp/cifar10_ddpmpp_continuous.py
    "smld": ("ncsnpp", dict(embedding_type="positional", num_scales=24), "vesde", False, False, False),   # configs/ve/cifar10_ncsnpp.py
    "ddpm": ("ddpmpp", dict(num_scales=24), "vpsde", False, False, False),        # configs/vp/cifar10_ddpmpp.py
    "ve_cont_lw": ("ncsnpp", {}, "vesde", True, False, True),                     # likelihood_weighting (losses.py:94-97)
    "vp_cont_rm": ("ddpmpp", {}, "vpsde", True, True, False),                     # reduce_mean (losses.py:71)
    "subvp_cont_lw_rm": ("ddpmpp", {}, "subvpsde", True, True, True),
}
# the resume case: the checkpoint is written after 2 steps by the reference's save_checkpoint dict (utils.py:22-29), the
# fixture also holds the reference's third step
TRAIN_CKPT_CASE = ("ncsnpp", dict(ch_mult=(1, 1)), "vesde", True, False, False)


def train_case_config(case):
    """config of a TRAIN_CASES entry (model overrides applied, warm-up shortened so that all three lr regimes occur)"""
    kind, over, sde_kind, continuous, _, _ = case
    over = dict(over)
    kw = {}
    if "ch_mult" in over:
        kw["ch_mult"] = over.pop("ch_mult")
    cfg = small_config(kind, **kw)
    for k, v in over.items():
        cfg.model[k] = v
    cfg.training.continuous = continuous
    cfg.optim.warmup = TRAIN_WARMUP
    return cfg


def train_case_sde(sde_lib, case, cfg):
    sde_kind = case[2]
    if sde_kind == "vesde":
        return sde_lib.VESDE(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=cfg.model.num_scales)
    cls = {"vpsde": sde_lib.VPSDE, "subvpsde": sde_lib.subVPSDE}[sde_kind]
    return cls(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)


def train_case_inputs(name, n_scales, steps=TRAIN_STEPS + 1, size=16):
    """per step: data batch in [0,1), the uniform draw behind t (losses.py:84), integer noise levels (losses.py:116,136),
    and z (losses.py:85); the last entry feeds the eval step"""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(("train_" + name).encode()) & 0xffff)
    out = []
    for _ in range(steps):
        batch = torch.rand(TRAIN_BATCH, 3, size, size, generator=g)
        u = torch.rand(TRAIN_BATCH, generator=g)
        labels = torch.randint(0, n_scales, (TRAIN_BATCH,), generator=g)
        z = torch.randn(TRAIN_BATCH, 3, size, size, generator=g)
        out.append((batch, u, labels, z))
    return out


class inject_rng:
    """Replace the three draws of a loss closure (torch.rand -> u, torch.randint -> labels, torch.randn_like -> z;
    losses.py:84-85,116-118,136-140) by given tensors, moved to the device the call asks for."""

    def __init__(self, u, labels, z):
        self.u, self.labels, self.z = u, labels, z

    def __enter__(self):
        self._real = (torch.rand, torch.randint, torch.randn_like)
        torch.rand = lambda *a, **kw: self.u.to(kw.get("device", "cpu"))
        torch.randint = lambda *a, **kw: self.labels.to(kw.get("device", "cpu"))
        torch.randn_like = lambda t, **kw: self.z.to(t.device)
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randint, torch.randn_like = self._real
        return False


def train_probe_names(named_shapes, limit=10000):
    """parameter tensors stored in full per step: the first tensor of every leaf class (Conv_0.weight, NIN_1.b, ...) that has
    at most `limit` elements"""
    seen, out = set(), []
    for name, shape in named_shapes:
        parts = name.split(".")
        leaf = ".".join(parts[2:]) if len(parts) > 3 else "top." + parts[-1] + str(len(shape))
        if leaf in seen or int(np.prod(shape)) > limit:
            continue
        seen.add(leaf)
        out.append(name)
    return out
