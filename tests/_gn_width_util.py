"""Cases shared by tools/gen_golden_gn_width.py and the GroupNorm-width tests: the small nf = 16 network whose decoder
normalises 192 = 128 + 64 channels in 32 groups of 6 (nn.GroupNorm(min(C // 4, 32), C), models/layerspp.py:219,231)."""
import torch

import _util

SMALL = dict(image_size=32, nf=16, ch_mult=(1, 2, 4, 8), num_res_blocks=1, attn=(16,))
BATCH = 2
TRAIN_NAME = "ve_cont_nf16"
TRAIN_CASE = ("ffhq", {}, "vesde", True, False, False)        # the layout of tests/_util.TRAIN_CASES entries
TRAIN_PROBE_LIMIT = 2500


def small_config(dropout=0.0, **over):
    """ve/ffhq_256_ncsnpp_continuous (fir, progressive='output_skip', progressive_input='input_skip') cut down to 32 px"""
    kw = dict(SMALL)
    kw.update(over)
    cfg = _util.small_config("ffhq", **kw)
    cfg.model.dropout = dropout
    return cfg


def train_config():
    cfg = small_config()
    cfg.training.continuous = True
    cfg.optim.warmup = _util.TRAIN_WARMUP
    return cfg


def forward_inputs(cfg, batch=BATCH, seed=21):
    g = torch.Generator().manual_seed(seed)
    R = cfg.data.image_size
    x = torch.randn(batch, 3, R, R, generator=g) * 3
    sig = torch.exp(torch.rand(batch, generator=g) * 6 - 3)
    return x, sig
