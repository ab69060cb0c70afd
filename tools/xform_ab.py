#!/usr/bin/env python
"""A/B of the F(4x4,3x3) input-transform pass (wino4_xform.hip) alone (GPU only): the two-kernel launch (pass + register-fed
matrix kernel) and the matrix kernel on a given V, HIP events around `reps` launches each, per variant of the pass and shape;
pass = two kernels - matrix kernel.  The variants are launch flags (SSDE_CONVF_XFORM_PLAIN or not), taken in turn A-B-A-B in one process.

    python tools/xform_ab.py [batch [reps [rounds]]]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bench as cb  # noqa: E402
from score_sde_pytorch_amd import _lib as L  # noqa: E402

SHAPES = [(128, 128, 32), (256, 128, 32), (256, 256, 16), (512, 256, 16)]      # (cin, cout, map): the sampler's F(4x4,3x3) layers
VARIANTS = [("plain stores", L.CONVF_XFORM_PLAIN), ("library's choice", 0)]

if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    for cin, cout, h in SHAPES:
        for gn in (1, 0):
            _, given = cb.time_conv(n, cin, cout, h, L.TILE_WINOGRAD4R, gn, reps=reps, flags=L.CONVF_V_GIVEN)
            for r in range(rounds):
                for name, fl in VARIANTS:
                    _, ms = cb.time_conv(n, cin, cout, h, L.TILE_WINOGRAD4R, gn, reps=reps, flags=fl)
                    print("B=%d %4d->%4d @%2dx%-2d gn=%d round %d  %-18s two kernels %.4f ms  matrix kernel on a given V %.4f ms  pass %.4f ms"
                          % (n, cin, cout, h, h, gn, r, name, ms, given, ms - given), flush=True)
