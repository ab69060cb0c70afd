#!/usr/bin/env python
"""Dump what the kernels of conv1x1.hip write, bit for bit, to compare two builds of the library.

    python tools/gemm1x1_dump.py out.npz            # the CPU emulator (tests/emu), no GPU needed
    python tools/gemm1x1_dump.py out.npz --cuda     # the library on cuda:0 (SSDE_LIB_PATH picks another build)
    python tools/gemm1x1_dump.py --compare a.npz b.npz

Every case goes through hipops.conv2d with seeded inputs: the 1x1 GEMM cases of tests/test_emulated_kernels.py (every
matrix mode, the persistent kernel on a pretend 3-CU device, the row / load-ahead shapes and the wide tile of the split
kernel) and three more: a dropout prologue, GroupNorm partials of whole-image entries (H*W = 16) and GroupNorm
partials written by the persistent kernel.  The .npz holds `dst` of each case and, where the launch can write them
(ssde_conv_gn_slices > 0), the raw GroupNorm partial buffer.  --compare asks np.array_equal of every array.
Each launch is checked to have the LDS size of a kernel shape of conv1x1.hip (ssde_conv_lds_bytes); a case the library
keeps on the general kernel (fewer than 128 pixels) is dumped with a note.
"""
import argparse
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (n, h, cin1, cin2, cout, prologue, extras): the tests' own lists
from test_emulated_kernels import GEMM1X1_CASES, GEMM1X1_ROWS_CASES, GEMM1X1_ROWS_SHAPES, GEMM1X1_WIDE_CASES  # noqa: E402

# LDS bytes of the kernel shapes of conv1x1.hip (ssde_conv_lds_bytes): every launch must report one of them, and a case that
# forces a shape the one of that shape -- a launch the library routed to another file would not
LDS_F32, LDS_X128, LDS_X64, LDS_WIDE, LDS_PIPE = 36864, 49152, 36864, 73728, 57856
PIPE_ENV = {"SSDE_GEMM_PIPE": "2", "SSDE_NUM_CUS": "3"}


def cases():
    """(name, environment, shape, dropout p)"""
    out = []
    for matrix in ("f32", "bf16x6"):
        for pipe in ("0", "2"):
            env = dict(SSDE_MATRIX=matrix, **(PIPE_ENV if pipe == "2" else {"SSDE_GEMM_PIPE": "0"}))
            out += [("gemm_%s_pipe%s_%d" % (matrix, pipe, i), env, c, 0.0) for i, c in enumerate(GEMM1X1_CASES)]
    for bm, pf in GEMM1X1_ROWS_SHAPES:
        env = dict(SSDE_MATRIX="bf16x6", SSDE_GEMM_PIPE="0", SSDE_X6_BM=bm, SSDE_X6_PF=pf, SSDE_X6_WIDE="0")
        out += [("rows_bm%s_pf%s_%d" % (bm, pf, i), env, c, 0.0) for i, c in enumerate(GEMM1X1_ROWS_CASES)]
    env = dict(SSDE_MATRIX="bf16x6", SSDE_GEMM_PIPE="0", SSDE_X6_WIDE="1")
    out += [("wide_%d" % i, env, c, 0.0) for i, c in enumerate(GEMM1X1_WIDE_CASES)]
    for matrix, pipe in (("f32", "0"), ("bf16x6", "0"), ("bf16x6", "2")):
        env = dict(SSDE_MATRIX=matrix, **(PIPE_ENV if pipe == "2" else {"SSDE_GEMM_PIPE": "0"}))
        out.append(("dropout_%s_pipe%s" % (matrix, pipe), env, (2, 16, 64, 32, 256, 2, True), 0.25))
        out.append(("gn_part_hw16_%s_pipe%s" % (matrix, pipe), env, (9, 4, 64, 0, 128, 3, True), 0.0))
    out.append(("gn_part_hw64_pipe", dict(SSDE_MATRIX="bf16x6", **PIPE_ENV), (3, 8, 40, 0, 96, 0, True), 0.0))
    return out


@contextlib.contextmanager
def environment(env):
    keys = ("SSDE_MATRIX", "SSDE_GEMM_PIPE", "SSDE_NUM_CUS", "SSDE_X6_BM", "SSDE_X6_PF", "SSDE_X6_WIDE")
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@contextlib.contextmanager
def launch_extras(dev, dropout, parts):
    """hipops.conv2d has no dropout or GroupNorm-partial argument: both are set on the launch arguments on their way to the library"""
    from score_sde_pytorch_amd import _lib as L, hipops
    lib = L.load()
    real = lib.ssde_conv2d
    seed = torch.tensor([12345], dtype=torch.int32, device=dev)

    def conv2d(ref, stream):
        a = ref._obj
        if dropout:
            hipops.set_dropout(a.aux, dropout, seed, 7)
        slices = int(lib.ssde_conv_gn_slices(C.byref(a)))
        if slices > 0:
            part = torch.zeros(a.n, slices, a.c_out // 4, 3, device=dev)
            a.gn_part = hipops._p(part)
            parts.append(part)
        # which kernel: the LDS bytes of the launch (ssde_conv_lds_bytes) are those of a shape of conv1x1.hip, and of the forced shape
        # where the case forces one (the persistent kernel takes GroupNorm partials for H*W % 64 == 0, a per-image addend for % 8)
        env, hw, lds = os.environ, a.h_out * a.w_out, int(lib.ssde_conv_lds_bytes(ref))
        if a.c_out < 96 or a.n * hw < 128:          # (ssde_conv1x1_wants: such a launch stays on the general kernel)
            print("note: n=%d hw=%d cout=%d is no launch of conv1x1.hip (fewer than 128 pixels or 96 output channels); dumped all the same" % (a.n, hw, a.c_out))
            return real(ref, stream)
        x6 = env["SSDE_MATRIX"] == "bf16x6"
        pipe = x6 and env["SSDE_GEMM_PIPE"] == "2" and a.c_out % 4 == 0 and (slices == 0 or hw % 64 == 0) and (not a.chan_add or hw % 8 == 0)
        want = (LDS_PIPE if pipe else LDS_WIDE if x6 and env.get("SSDE_X6_WIDE") == "1" else LDS_X64 if x6 and env.get("SSDE_X6_BM") == "64"
                else None if x6 else LDS_F32)
        if lds not in (LDS_F32, LDS_X128, LDS_X64, LDS_WIDE, LDS_PIPE) or (want is not None and lds != want):
            raise SystemExit("a case did not take the kernel of conv1x1.hip it was written for: LDS %d, expected %s" % (lds, want))
        return real(ref, stream)
    lib.ssde_conv2d = conv2d
    try:
        yield
    finally:
        lib.ssde_conv2d = real


def run_case(shape, dropout, dev):
    from score_sde_pytorch_amd import hipops
    n, h, c1, c2, cout, pro, extras = shape
    g = torch.Generator().manual_seed(n * 1000 + cout)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    xa = torch.randn(n, c1, h, h, generator=g)
    xb = torch.randn(n, c2, h, h, generator=g) if c2 else None
    k = c1 + c2
    w = torch.randn(cout, k, generator=g) / np.sqrt(k)
    gn = None
    if pro in (1, 2):
        G = k // 4 if k // 4 <= 32 else 32
        while k % G or (k // G) % 4:
            G -= 1
        gam, bet = 1 + 0.1 * torch.randn(k, generator=g), 0.1 * torch.randn(k, generator=g)
        mean, rstd = hipops.groupnorm_stats(nhwc(xa), G, x2=None if xb is None else nhwc(xb))
        gn = (mean, rstd, gam.to(dev), bet.to(dev), G)
    kw = {}
    if extras:
        bias, tproj, res = torch.randn(cout, generator=g), torch.randn(n, cout, generator=g), torch.randn(n, cout, h, h, generator=g)
        kw = dict(bias=bias.to(dev), chan_add=tproj.to(dev), resid=nhwc(res), scale=float(1 / np.sqrt(2)))
    parts = []
    with launch_extras(dev, dropout, parts):
        y = hipops.conv2d(aux=nhwc(xa), aux2=None if xb is None else nhwc(xb), aux_weight=w.to(dev), aux_pro=pro, aux_gn=gn, **kw)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return y.cpu().numpy(), [p.cpu().numpy() for p in parts]


def dump(path, cuda):
    import emu
    dev = torch.device("cuda:0" if cuda else "cpu")
    arrays = {}
    with contextlib.nullcontext() if cuda else emu.emulated():
        for name, env, shape, dropout in cases():
            with environment(env):
                y, parts = run_case(shape, dropout, dev)
            arrays[name + ".dst"] = y
            for i, p in enumerate(parts):
                arrays["%s.gn_part%d" % (name, i)] = p
    np.savez(path, **arrays)
    print("%d arrays of %d cases -> %s" % (len(arrays), len(cases()), path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        if not np.array_equal(A[k], B[k]):
            bad.append(k)
            print("DIFFERS %s: %d of %d elements" % (k, int((A[k] != B[k]).sum()) if A[k].shape == B[k].shape else -1, A[k].size))
    print("%d arrays, %d differ or are missing" % (len(set(A.files) | set(B.files)), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--cuda", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.out, args.cuda)
