#!/usr/bin/env python
"""Attention kernels on the GPU, warm, HIP events, alternating A-B-A-B on one box.

    python tools/attn_bench.py             # the sampler's 16 x 16 shapes: fp32-MFMA kernel / BF16-pipe kernel / forced streaming
    python tools/attn_bench.py --long      # (64, 1024, 256): streaming forward against attn_kernel at (256, 256, 256) (the same
                                           # FLOPs) and against the eager three-op form in torch; the streaming backward
    python tools/attn_bench.py --shape N L C [--stream]     # one forward shape; --stream sets SSDE_ATTN_STREAM=1 (any L)

Rates are EXECUTED FLOP/s of the contractions: 4 N L^2 C forward; backward 14 N L^2 C up to 256 tokens (S, dP, dQ in the dQ
kernel; S^T, dV, dP^T, dK in the dK / dV kernel) and 16 N L^2 C above (one more Q K^T in the statistics pass); the algorithm's
own minimum is 10.  Per-kernel times of the backward's launches come from rocprofv3 --kernel-trace --stats on `--shape ... --bwd`."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from score_sde_pytorch_amd import hipops as ops, _lib as L  # noqa: E402

ROUTE_NAMES = {L.ATTN_ROUTE_F32: "attn_kernel", L.ATTN_ROUTE_X6: "attn_x6_kernel", L.ATTN_ROUTE_STREAM: "attn_stream_kernel"}


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def forward_mode(qkv, c, mode, reps):
    """mode: 'f32' | 'x6' | 'stream' (the environment is what hipops.attention turns into flags)"""
    os.environ["SSDE_MATRIX"] = "bf16x6" if mode == "x6" else "f32"
    os.environ["SSDE_ATTN_X6"] = "1"
    os.environ["SSDE_ATTN_STREAM"] = "1" if mode == "stream" else "0"
    route = ROUTE_NAMES[ops.attention_route(qkv.shape[0], qkv.shape[1], c)]
    return route, timed(lambda: ops.attention(qkv, c), reps)


def eager(qkv, c):
    q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    return torch.softmax(torch.bmm(q, k.transpose(1, 2)) * (c ** -0.5), dim=-1) @ v


def report(tag, n, l, c, ms, flop_factor=4.0):
    fl = flop_factor * n * l * l * c
    print("%-44s N=%3d L=%5d C=%3d  %.4f ms  %.1f TF/s" % (tag, n, l, c, ms, fl / ms / 1e9), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--shape", type=int, nargs=3, metavar=("N", "L", "C"))
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--bwd", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    if a.shape:
        n, l, c = a.shape
        qkv = torch.randn(n, l, 3 * c, device="cuda", generator=g)
        route, ms = forward_mode(qkv, c, "stream" if a.stream else "f32", a.reps)
        report("forward " + route, n, l, c, ms)
        if a.bwd:
            y, d_o = ops.attention(qkv, c), torch.randn(n, l, c, device="cuda", generator=g)
            report("backward (all launches)", n, l, c, timed(lambda: ops.attention_bwd(qkv, y, d_o, c), a.reps), 16.0 if l > 256 else 14.0)
        return
    if a.long:
        n, l, c = 64, 1024, 256
        big = torch.randn(n, l, 3 * c, device="cuda", generator=g)
        small = torch.randn(4 * n, 256, 3 * c, device="cuda", generator=g)       # the same 4 N L^2 C
        err = float((ops.attention(big[:4], c) - eager(big[:4], c)).abs().max())
        print("streaming forward vs eager torch on the timed inputs: max abs difference %.3g" % err)
        for r in range(a.rounds):
            report("round %d: streaming forward" % r, n, l, c, forward_mode(big, c, "f32", a.reps)[1])
            report("round %d: attn_kernel (single tile)" % r, 4 * n, 256, c, forward_mode(small, c, "f32", a.reps)[1])
            report("round %d: eager torch bmm/softmax/bmm" % r, n, l, c, timed(lambda: eager(big, c), a.reps))
        y, d_o = ops.attention(big, c), torch.randn(n, l, c, device="cuda", generator=g)
        os.environ["SSDE_ATTN_STREAM"] = "0"
        for r in range(a.rounds):
            report("round %d: streaming backward (3 launches)" % r, n, l, c, timed(lambda: ops.attention_bwd(big, y, d_o, c), a.reps), 16.0)
        return
    for n, c in [(256, 256), (128, 256), (64, 256), (256, 128), (256, 64)]:
        qkv = torch.randn(n, 256, 3 * c, device="cuda", generator=g)
        for r in range(a.rounds):
            for mode in ("f32", "x6", "stream"):
                route, ms = forward_mode(qkv, c, mode, a.reps)
                report("round %d: %s" % (r, route), n, 256, c, ms)


if __name__ == "__main__":
    main()
