"""Cases shared by tools/gen_golden_attn_long.py and the long-attention tests: the small NCSN++ network at 32 px with
attn_resolutions = (32, 16) -- attention over L = 1024 tokens at C = 32 and over L = 256 at C = 64 -- and the small DDPM network
at 32 px with attention at 32 x 32 (L = 1024, C = 128)."""
import torch

import _util
import _ddpm_util as D

NCSNPP = dict(image_size=32, attn=(32, 16))            # nf = 32, ch_mult = (1, 2), one block per level
DDPM = dict(image_size=32, attn=(32,))                 # nf = 128, ch_mult = (1, 2)
BATCH = 2
TRAIN_NAME = "ve_cont_attn32"
TRAIN_CASE = ("ncsnpp", {}, "vesde", True, False, False)      # the layout of tests/_util.TRAIN_CASES entries
TRAIN_PROBE_LIMIT = 2500


def small_config():
    return _util.small_config("ncsnpp", **NCSNPP)


def train_config():
    cfg = small_config()
    cfg.training.continuous = True
    cfg.optim.warmup = _util.TRAIN_WARMUP
    return cfg


def ddpm_config():
    cfg = D.small_config(attn_resolutions=DDPM["attn"])
    cfg.data.image_size = DDPM["image_size"]
    return cfg


def forward_inputs(cfg, batch=BATCH, seed=31):
    g = torch.Generator().manual_seed(seed)
    R = cfg.data.image_size
    x = torch.randn(batch, 3, R, R, generator=g) * 3
    sig = torch.exp(torch.rand(batch, generator=g) * 6 - 3)
    return x, sig


def ddpm_inputs(cfg):
    return D.forward_inputs(cfg, batch=BATCH, seed=131)
