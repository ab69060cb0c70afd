#!/usr/bin/env python
"""A/B of DDPM's Downsample convolution (F.pad(x, (0, 1, 0, 1)) + 3x3 / stride 2): one end-padded launch (pad_end = 1) against the
form the kernels offered before it -- an identity upfirdn that materialises the padded copy, then stride 2 / pad 0 on the copy.
Forward and weight gradient at the three CIFAR Downsample shapes of vp/ddpm/cifar10:

    python tools/pad_end_ab.py [batch=256] [rounds=9]

Both forms are warmed up, then timed alternately for `rounds` windows of `reps` launches each (device events around a window);
the table gives the median window and, as the run-to-run spread, (max - min) / median of the copy form's windows.  The
weight-gradient rows time the whole of what a training step would run for that form: for the copy form the pad copy is the
forward's by-product, so only the gradient launch on the copy is timed (the favourable case for it).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from score_sde_pytorch_amd import hipops as ops  # noqa: E402

SHAPES = [(32, 128), (16, 256), (8, 256)]           # (map, channels) of the Downsample modules, ch_mult (1, 2, 2, 2), nf 128
ONE = torch.ones(1, 1)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(fa, fb, rounds, reps):
    for _ in range(3):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, reps))
        tb.append(window(fb, reps))
    ta.sort(); tb.sort()
    med = lambda v: v[len(v) // 2]          # noqa: E731
    return med(ta), (ta[-1] - ta[0]) / med(ta), med(tb), (tb[-1] - tb[0]) / med(tb)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    print("end-padded 3x3 / stride 2 convolution against pad copy + stride 2 / pad 0, batch %d, %d alternating windows" % (n, rounds))
    print("%-28s %12s %8s %12s %8s %8s" % ("launch", "copy form ms", "spread", "pad_end ms", "spread", "ratio"))
    g = torch.Generator().manual_seed(1)
    for h, c in SHAPES:
        x = torch.randn(n, h, h, c, generator=g).cuda()
        w = (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).cuda()
        b = torch.randn(c, generator=g).cuda()
        gy = torch.randn(n, h // 2, h // 2, c, generator=g).cuda()
        dw = torch.zeros(c, c, 3, 3, device="cuda")
        reps = 20 if h == 32 else 50

        def fwd_copy():
            xp = ops.upfirdn2d_nhwc(x, ONE, pad=(0, 1))
            return ops.conv2d(xp, w, b, stride=2, pad=0)

        def fwd_pad_end():
            return ops.conv2d(x, w, b, stride=2, pad=0, pad_end=1)

        ya, yb = fwd_copy(), fwd_pad_end()
        assert ya.shape == yb.shape and torch.equal(ya, yb), "the two forms must agree bit for bit"
        xp = ops.upfirdn2d_nhwc(x, ONE, pad=(0, 1))

        def wg_copy():
            return ops.conv_wgrad(xp, gy, 3, dw, stride=2, pad=0)

        def wg_pad_end():
            return ops.conv_wgrad(x, gy, 3, dw, stride=2, pad=0, pad_end=1)

        da = wg_copy().clone(); dw.zero_()
        db = wg_pad_end().clone(); dw.zero_()
        assert torch.equal(da, db), "the two weight gradients must agree bit for bit"
        for name, fa, fb in (("forward", fwd_copy, fwd_pad_end), ("weight gradient", wg_copy, wg_pad_end)):
            a, sa, p, sp = ab(fa, fb, rounds, reps)
            print("%-28s %12.4f %7.1f%% %12.4f %7.1f%% %8.3f" % ("%s %dx%d %d->%d" % (name, h, h, c, c), a, 100 * sa, p, 100 * sp, p / a),
                  flush=True)


if __name__ == "__main__":
    main()
