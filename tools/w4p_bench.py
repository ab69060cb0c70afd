#!/usr/bin/env python
"""Micro-benchmark of the 4x4-map 3x3 convolutions (GPU only): the direct kernel against the position-batched F(4x4,3x3)
form (conv_wino4p.hip) with 1 / 2 / 4 reduction shares and with the library's own choice, GroupNorm + SiLU prologue, at the
sampler's and the training step's batches.  The numbers behind engine.W4P_MIN_BATCH and conv_wino4p.hip's split rule."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from score_sde_pytorch_amd import _lib as L  # noqa: E402
import conv_bench as cb  # noqa: E402

if __name__ == "__main__":
    batches = [int(v) for v in sys.argv[1:]] or [256, 128, 64, 16]
    for n in batches:
        for cin, cout in ((256, 256), (512, 256), (768, 256)):
            best = lambda tile, fl: min(cb.time_conv(n, cin, cout, 4, tile, 1, reps=20, flags=fl)[1] for _ in range(3))  # noqa: E731
            d = best(L.TILE_AUTO, 0)
            row = [("auto", best(L.TILE_WINOGRAD4P, 0))]
            row += [("ks%d" % k, best(L.TILE_WINOGRAD4P, f)) for k, f in ((1, L.CONVF_NO_KSPLIT), (2, L.CONVF_KSPLIT2), (4, L.CONVF_KSPLIT4))]
            print("B=%3d %4d->%4d @4x4 gn  direct %.4f ms   position-batched %s" % (n, cin, cout, d, "  ".join("%s %.4f" % r for r in row)),
                  flush=True)
