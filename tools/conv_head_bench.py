#!/usr/bin/env python
"""The image heads of data with more than four channels (3x3 onto 8 / 12 / 16 channels, GroupNorm + SiLU prologue): conv_small.hip's
2- and 4-quad instantiations (SSDE_CONVF_SMALL_COUT_WIDE) against the direct kernel (the same launch without the flag), with
today's c_out = 4 launch beside them for scale.  GPU only.

    python tools/conv_head_bench.py [rounds] > profiles/chan_head_bench.txt

Per shape the variants are timed in alternation -- `rounds` rounds (default 15), in each round every variant runs `reps` launches
between two device events -- and the table gives the median, the minimum and the maximum of a variant's rounds: the spread of the
session next to every difference.  The two outputs are compared before anything is timed (relative difference, direct kernel's
tolerance 2e-5).  engine.HEAD_WIDE_QUADS is decided from this table."""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from score_sde_pytorch_amd import hipops as ops, _lib as L  # noqa: E402
from score_sde_pytorch_amd.engine import pack_conv_weight  # noqa: E402

# (batch, input channels, output channels, map): the CIFAR-sized head at the sampler's batch, the 256-px head
SHAPES = [(256, 128, 8, 32), (256, 128, 12, 32), (256, 128, 16, 32), (8, 128, 8, 256), (8, 128, 16, 256)]


def make_launch(n, cin, cout, h, flags):
    dev = "cuda"
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(n, h, h, cin, generator=g).to(dev)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(dev)
    G = min(cin // 4, 32)
    mean, rstd = ops.groupnorm_stats(x, G, 1e-6)
    gnt = (mean, rstd, torch.ones(cin, device=dev), torch.zeros(cin, device=dev), G)
    a = L.ConvArgs()
    ops._fill_src(a.main, x, None, L.PRO_GN_SILU, gnt)
    wp, bias = pack_conv_weight(w), torch.zeros(cout, device=dev)
    dst = torch.empty(n, h, h, cout, device=dev)
    a.w_main, a.ksize, a.stride, a.pad, a.h_in, a.w_in = wp.data_ptr(), 3, 1, 1, h, h
    a.n, a.h_out, a.w_out, a.c_out, a.out_scale, a.dst, a.tile = n, h, h, cout, 1.0, dst.data_ptr(), L.TILE_AUTO
    a.bias, a.flags = bias.data_ptr(), L.conv_route_flags() | flags
    return a, dst, (x, w, gnt, wp, bias)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    lib, st = L.load(), ops._stream()
    print("# rounds %d, variants alternate within a round; ms per launch: median [min .. max]" % rounds)
    for n, cin, cout, h in SHAPES:
        variants = [("conv_small wide", make_launch(n, cin, cout, h, L.CONVF_SMALL_COUT_WIDE)),
                    ("direct", make_launch(n, cin, cout, h, 0)),
                    ("conv_small c_out=4", make_launch(n, cin, 4, h, 0))]
        lds = [lib.ssde_conv_lds_bytes(C.byref(v[1][0])) for v in variants]
        for _, (a, _, _) in variants:                       # warm-up: code objects, the LDS opt-in
            for _ in range(3):
                L.check(lib.ssde_conv2d(C.byref(a), st))
        torch.cuda.synchronize()
        diff = float((variants[0][1][1] - variants[1][1][1]).abs().max() / variants[1][1][1].abs().max())
        assert diff < 2e-5, diff
        reps = max(50, int(400 * 256 * 32 * 32 / (n * h * h)))         # windows of 35-80 ms
        times = [[] for _ in variants]
        for _ in range(rounds):
            for i, (_, (a, _, _)) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    L.check(lib.ssde_conv2d(C.byref(a), st))
                e1.record()
                torch.cuda.synchronize()
                times[i].append(e0.elapsed_time(e1) / reps)
        gb = n * h * h * cin * 4 / 1e9
        row = ["%s (%d B LDS) %.4f [%.4f .. %.4f]" % (name, lds[i], statistics.median(times[i]), min(times[i]), max(times[i]))
               for i, (name, _) in enumerate(variants)]
        print("%d->%d @%dx%d n=%d (%.3f GB read, wide vs direct rel diff %.2g) | " % (cin, cout, h, h, n, gb, diff) + " | ".join(row), flush=True)


if __name__ == "__main__":
    main()
