"""The cases of the channel-count tests (config.data.num_channels = C for any C >= 1): configs and inputs, shared by
tests/_chan_checks.py and by tools/gen_golden_channels.py, which records the reference's outputs for them.  16-px images,
nf = 32, batch 3, dropout 0 (tests/_util.small_config); the `ddpm` family's case is tests/_ddpm_util.small_config (nf = 128: the
narrowest width its 32-group GroupNorm allows on the HIP path)."""
import zlib

import numpy as np
import torch

import _util
import _arch_checks as A
import _ddpm_util as D

BATCH = 3
COT_SEED = 321
TRAIN_PROBE_LIMIT = 5000

# name -> (model family, small-config kind, small_config keywords, config.model overrides, channels)
FORWARD_CASES = {
    # what already worked with the image padded to one quad
    "ncsnpp_c1": ("ncsnpp", "ncsnpp", {}, {}, 1),
    "ncsnpp_c2": ("ncsnpp", "ncsnpp", {}, {}, 2),
    "ffhq_c4": ("ncsnpp", "ffhq", {}, {}, 4),
    # the residual input pyramid with FIR, pyr_c = 8
    "ncsnpp_c6": ("ncsnpp", "ncsnpp", {}, {}, 6),
    # input-skip and output-skip: a head per level, FIR upsampling of the pyramid, a combine GEMM with K = 8
    "ffhq_c8": ("ncsnpp", "ffhq", {}, {}, 8),
    "ddpmpp_c6": ("ncsnpp", "ddpmpp", {}, {}, 6),
    "cat_c6": ("ncsnpp",) + A.CASES["cat"] + (6,),
    # ragged last quad, cpad = 16
    "ncsnpp_c13": ("ncsnpp", "ncsnpp", {}, {}, 13),
    # above the head kernel's range: the direct route
    "ncsnpp_c20": ("ncsnpp", "ncsnpp", {}, {}, 20),
    "ddpm_c6": ("ddpm", "ddpm", {}, {}, 6),
}
# name -> SDE of the continuous loss
TRAIN_CASES = {"ncsnpp_c1": "vesde", "ncsnpp_c6": "vesde", "ffhq_c8": "vesde"}


def channels(case):
    return FORWARD_CASES[case][4]


def family(case):
    return FORWARD_CASES[case][0]


def config(case):
    fam, kind, kw, over, c = FORWARD_CASES[case]
    if fam == "ddpm":
        cfg = D.small_config()          # (nf = 128: the family's GroupNorm has 32 groups, and the HIP path wants groups of 4 channels)
    else:
        cfg = _util.small_config(kind, **kw)
    for k, v in over.items():
        cfg.model[k] = v
    cfg.data.num_channels = c
    assert cfg.data.image_size == 16 and cfg.model.nf == (128 if fam == "ddpm" else 32) and float(cfg.model.dropout) == 0.0
    return cfg


def forward_inputs(case):
    """tests/_arch_checks.forward_inputs with the case's channel count: batch 3, generator seed 123 (+ the channel count, so
    that no two counts share a prefix); integer-valued labels for the `ddpm` family (tests/_ddpm_util.forward_inputs)"""
    cfg = config(case)
    c, R = channels(case), cfg.data.image_size
    g = torch.Generator().manual_seed(123 + 1000 * c)
    x = torch.rand(BATCH, c, R, R, generator=g) if not cfg.data.centered else torch.rand(BATCH, c, R, R, generator=g) * 2 - 1
    if family(case) == "ddpm":
        x = x + 0.5 * torch.randn(BATCH, c, R, R, generator=g)
        cond = torch.randint(0, 1000, (BATCH,), generator=g).float()
    elif cfg.model.embedding_type == "fourier":
        cond = torch.exp(torch.rand(BATCH, generator=g) * (np.log(50.0) - np.log(0.01)) + np.log(0.01)).float()
        x = x + cond[:, None, None, None] * torch.randn(BATCH, c, R, R, generator=g)
    else:
        cond = (torch.rand(BATCH, generator=g) * 999).float()
    return x, cond


def cotangent(case):
    x, _ = forward_inputs(case)
    return torch.randn(x.shape, generator=torch.Generator().manual_seed(COT_SEED))


def train_case(case):
    """the layout of a tests/_util.TRAIN_CASES entry"""
    return (FORWARD_CASES[case][1], {}, TRAIN_CASES[case], True, False, False)


def train_config(case):
    cfg = config(case)
    cfg.training.continuous = True
    cfg.optim.warmup = _util.TRAIN_WARMUP
    return cfg


def train_inputs(case, steps=2):
    """tests/_util.train_case_inputs with the case's channel count: per step the data batch in [0, 1), the uniform draw behind
    t, integer noise levels and z"""
    cfg = config(case)
    c, R = channels(case), cfg.data.image_size
    g = torch.Generator().manual_seed(zlib.crc32(("train_chan_" + case).encode()) & 0xffff)
    out = []
    for _ in range(steps):
        batch = torch.rand(BATCH, c, R, R, generator=g)
        u = torch.rand(BATCH, generator=g)
        labels = torch.randint(0, cfg.model.num_scales, (BATCH,), generator=g)
        z = torch.randn(BATCH, c, R, R, generator=g)
        out.append((batch, u, labels, z))
    return out


def pc_inputs(batch, n_steps, sigma_max, size, c, seed=29, streams=2):
    """tests/_util.pc_case_inputs with a channel count: x_T and the injected noises [n_steps, streams, ...]"""
    g = torch.Generator().manual_seed(seed + 1000 * c)
    x_T = torch.randn(batch, c, size, size, generator=g) * sigma_max
    noises = torch.randn(n_steps, streams, batch, c, size, size, generator=g)
    return x_T, noises
