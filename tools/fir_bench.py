#!/usr/bin/env python
"""Micro-benchmark of ssde_upfirdn2d at the shapes the BASELINE networks use (GPU only): algorithmic bytes
(input + output(s), fp32) / time against the 8 TB/s HBM peak.  `dual` = act(GroupNorm(x)) and x filtered in one launch.

    python tools/fir_bench.py            # the 4-tap shapes
    python tools/fir_bench.py wide       # the same launches with 3 .. 16 taps, the 4x4 FIR with cropping pads and a 4x3
                                         # kernel: the LDS-tiled any-tap-count kernel (SSDE_FIRF_TILED) against the
                                         # one-lane-per-output kernel (SSDE_FIRF_GENERAL), alternated A-B-A-B in one process
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from score_sde_pytorch_amd import hipops as ops, _lib as L  # noqa: E402
from score_sde_pytorch_amd.engine import fir_taps  # noqa: E402


def time_fir(n, c, h, up, down, pad, pro, dual, reps=10, taps=(1, 3, 3, 1), flags=0, window_ms=0.0):
    """one launch record built once, launched reps times between two device events -- no host work but the C call inside the
    window.  window_ms > 0: reps is raised until the timed window is at least that long."""
    x = torch.randn(n, h, h, c, device="cuda")
    G = min(c // 4, 32)
    k = np.ascontiguousarray(taps if np.ndim(taps) == 2 else fir_taps(list(taps), gain=float(up * up)), dtype=np.float32)
    kh, kw = k.shape
    h_out, w_out = (h * up + pad[0] + pad[1] - kh) // down + 1, (h * up + pad[0] + pad[1] - kw) // down + 1
    y = torch.empty(n, h_out, w_out, c, device="cuda")
    y2 = torch.empty_like(y) if dual else None
    a = L.UpfirdnArgs()
    a.src.p0, a.src.c0 = x.data_ptr(), c
    if pro:
        mean, rstd = ops.groupnorm_stats(x, G, 1e-6)
        gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
        a.src.pro_mode, a.src.gn_groups = L.PRO_GN_SILU, G
        a.src.gn_mean, a.src.gn_rstd, a.src.gn_gamma, a.src.gn_beta = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    a.n, a.h_in, a.w_in, a.c, a.h_out, a.w_out = n, h, h, c, h_out, w_out
    a.up, a.down, a.pad0, a.pad1, a.kh, a.kw, a.flags = up, down, pad[0], pad[1], kh, kw, flags
    if kh <= 4 and kw <= 4:
        for i, v in enumerate(k.reshape(-1).tolist()):
            a.k[i] = v
    else:
        kd = torch.from_numpy(k).cuda()
        a.taps = kd.data_ptr()
    a.dst, a.dst2 = y.data_ptr(), y2.data_ptr() if dual else None
    lib, ref, st = L.load(), C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.ssde_upfirdn2d(ref, st), "ssde_upfirdn2d")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        e0.record()
        for _ in range(reps):
            lib.ssde_upfirdn2d(ref, st)
        e1.record()
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1)
        if total >= window_ms or reps >= 5000:
            break
        reps = min(5000, int(reps * max(2.0, 1.3 * window_ms / max(total, 1e-3))))
    ms = total / reps
    nbytes = 4.0 * (x.numel() + y.numel() * (2 if dual else 1))
    return nbytes / ms / 1e9, ms, nbytes      # bytes / ms / 1e9 = TB/s


def wide_ab():
    """the networks' launches with other kernels than the 4x4 FIR: pads from engine.fir_pads; tiled = FIRF_TILED, general =
    FIRF_GENERAL; each pair timed twice, alternating, every timing a window of at least 5 ms"""
    from score_sde_pytorch_amd.engine import fir_pads
    shapes = [(256, 128, 32, 1, 2, 1), (256, 256, 16, 1, 2, 1), (256, 256, 8, 1, 2, 1),
              (256, 256, 4, 2, 1, 1), (256, 256, 8, 2, 1, 1), (256, 256, 16, 2, 1, 1),
              (256, 128, 32, 1, 1, 3), (256, 256, 16, 1, 1, 3),
              (16, 128, 256, 1, 2, 1), (16, 128, 128, 2, 1, 1)]
    # (label, taps, pads: None = the networks' for that length)
    kernels = [("6", (1, 5, 10, 10, 5, 1), None), ("3", (1, 2, 1), None), ("5", (1, 4, 6, 4, 1), None), ("8", tuple([1] * 8), None),
               ("12", tuple([1] * 12), None), ("16", tuple([1] * 16), None),
               ("4 pads-1", (1, 3, 3, 1), (-1, -1)),                       # the 4x4 FIR cropping: off its own kernel
               ("4x3", np.outer([1, 3, 3, 1], [1, 2, 1]) / 32.0, None)]      # rectangular; pads of the 3-tap kernel
    for label, taps, fixed in kernels:
        n_taps = len(taps) if np.ndim(taps) == 1 else taps.shape[1]
        for n, c, h, up, down, conv in shapes:
            pad = fixed or fir_pads(n_taps, up=up == 2, conv=conv)
            for pro, dual in ((0, 0), (1, 1)) if conv == 1 else ((0, 0),):
                runs = [time_fir(n, c, h, up, down, pad, pro, dual, taps=taps, flags=f, window_ms=5.0)
                        for f in (L.FIRF_TILED, L.FIRF_GENERAL, L.FIRF_TILED, L.FIRF_GENERAL)]
                t, g = min(runs[0][1], runs[2][1]), min(runs[1][1], runs[3][1])
                print("taps=%-8s N=%3d C=%3d %3dx%-3d up=%d down=%d pad=%s pro=%d dual=%d  %7.1f MB  tiled %.4f %.4f ms  general %.4f %.4f ms  "
                      "tiled %.2f TB/s  general %.2f TB/s  tiled/general time %.2f"
                      % (label, n, c, h, h, up, down, pad, pro, dual, runs[0][2] / 1e6, runs[0][1], runs[2][1], runs[1][1], runs[3][1],
                         runs[0][2] / t / 1e9, runs[0][2] / g / 1e9, t / g), flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["wide"]:
        wide_ab()
        sys.exit(0)
    shapes = [(256, 128, 32, 1, 2, (1, 1)), (256, 256, 16, 1, 2, (1, 1)), (256, 256, 8, 1, 2, (1, 1)),
              (256, 256, 4, 2, 1, (2, 1)), (256, 256, 8, 2, 1, (2, 1)), (256, 256, 16, 2, 1, (2, 1)),
              (16, 128, 256, 1, 2, (1, 1)), (16, 128, 128, 2, 1, (2, 1))]
    for n, c, h, up, down, pad in shapes:
        for pro, dual in ((0, 0), (1, 0), (1, 1)):
            tbs, ms, nb = time_fir(n, c, h, up, down, pad, pro, dual, window_ms=5.0)
            print("N=%3d C=%3d %3dx%-3d up=%d down=%d pro=%d dual=%d  %7.1f MB  %.3f ms  %.2f TB/s = %.0f%% of 8 TB/s"
                  % (n, c, h, h, up, down, pro, dual, nb / 1e6, ms, tbs, tbs / 8.0 * 100.0), flush=True)
