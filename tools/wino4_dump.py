#!/usr/bin/env python
"""Dump what the F(4x4,3x3) kernels write, bit for bit, to compare two builds of the library (the kernels of conv_wino4.hip,
conv_wino4r.hip, conv_wino4p.hip, wino4_xform.hip and wgrad_wino4.hip, which share csrc/wino4_common.h).

    python tools/wino4_dump.py out.npz            # the CPU emulator (tests/emu), no GPU needed
    python tools/wino4_dump.py out.npz --cuda     # the library on cuda:0 (SSDE_LIB_PATH picks another build)
    python tools/wino4_dump.py --compare a.npz b.npz [--unstable p1.npz p2.npz]

The cases are the tests' own rows (tests/_conv_shape_checks.py: _wino_rows("f4"), _wino_rows("f4r"), _f4p_rows()), each in every
form of FORMS, plus the f4 row 2x(128+128)->64 @8x12.  The rows of 8 workgroups with 128 input channels or more split their
reduction: they run once as listed and once each on a pretend device of 16 and of 32 CUs (SSDE_NUM_CUS), where the rules
ssde_conv_wino4_splits / ssde_conv_wino4r_splits give two and four shares (f4: four need 256 channels) -- asserted by calling
the rule itself -- so every kKs instantiation of both kernels is launched.  The f4 rows run with and without the V by-product
(kEmitV).  Arrays: `dst`, its error against fp64 (`err`), the raw GroupNorm partial buffer where ssde_conv_gn_slices > 0,
`v` = the V by-product (f4) or what the transform pass wrote (f4r); and of the f4 weight-gradient rows of WGRAD_CASES `dw` and
the whole scratch (V, Z and the dU slabs).

--compare asks bit equality of every array (NaN prefills included).  The split rows of f4 / f4r hand partial sums over in
arrival order and need not repeat their own bits on a device: --unstable names two dumps of ONE build; an array that differs
between them is excused from equality, listed, and its `err` must stay below the suites' TOL_OP in both dumps compared.
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

import _conv_shape_checks as K  # noqa: E402
from score_sde_pytorch_amd import _lib as L  # noqa: E402

# the C++ names of the two rules (csrc/ssde_common.h: int f(int wgs, int ctot, int c_out, unsigned flags))
RULES = {"f4": "_Z22ssde_conv_wino4_splitsiiij", "f4r": "_Z23ssde_conv_wino4r_splitsiiij"}


def forward_cases():
    """(row, SSDE_NUM_CUS or None, shares expected or None, with V by-product)"""
    out = []
    rows = K._wino_rows("f4") + [K.fwd("f4", 2, 128, 128, 64, 8, 12)] + K._wino_rows("f4r") + K._f4p_rows()
    for c in rows:
        emits = (False, True) if c.route == "f4" else (False,)
        for ev in emits:
            out.append((c, None, None, ev))
            if c.route in RULES and c.c0 + c.c1 >= 128 and not c.flags & L.CONVF_NO_KSPLIT:
                assert K.wino_tiling(c.route, c.n, c.h, c.w) and c.cout <= 64          # 8 workgroups: one group of 8 pixel tiles
                out.append((c, "16", 2, ev))
                out.append((c, "32", 4 if c.c0 + c.c1 >= 256 else 2, ev))
    return out


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def run_forward(dev, lib, ops, c, form, shares, emit_v, arrays, name):
    from score_sde_pytorch_amd.engine import wino4_v_floats
    a, dst, keep = K.fwd_args(c, form, dev)
    if shares is not None:
        rule = getattr(lib, RULES[c.route])
        rule.restype, rule.argtypes = C.c_int, (C.c_int, C.c_int, C.c_int, C.c_uint)
        got = rule(8, c.c0 + c.c1, c.cout, a.flags) if form != K.FORMS[3] else 1      # (in place: dst is the hand-over buffer, no split)
        want = shares if form != K.FORMS[3] else 1
        assert got == want, (name, "shares", got, want)
    v = None
    if emit_v or c.route == "f4r":
        v = torch.full((wino4_v_floats(c.n, c.h, c.w, c.c0 + c.c1),), float("nan")).to(dev)
        a.wino_v = v.data_ptr()
    assert lib.ssde_conv_lds_bytes(C.byref(a)) > 0, (name, lib.ssde_last_error())
    if c.tile == L.TILE_WINOGRAD4P:
        need = int(lib.ssde_conv_ws_floats(C.byref(a)))
        ws = torch.full((need,), float("nan")).to(dev)
        a.wino_ws, a.wino_ws_floats = ws.data_ptr(), need
    sl = lib.ssde_conv_gn_slices(C.byref(a)) if form != K.FORMS[3] else 0
    part = None
    if sl > 0:
        part = torch.full((c.n, sl, c.cout // 4, 3), float("nan")).to(dev)
        a.gn_part = part.data_ptr()
    L.check(lib.ssde_conv2d(C.byref(a), ops._stream()), "ssde_conv2d")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    arrays[name + ".dst"] = bits(dst)
    arrays[name + ".err"] = np.array([K.rel_err(dst.cpu(), K.fwd_ref(c, form))])
    if part is not None:
        arrays[name + ".gn_part"] = bits(part)
    if v is not None:
        arrays[name + ".v"] = bits(v)


def run_wgrad(dev, lib, ops, c, arrays, name):
    route, need = K.wg_plan(c)
    assert route == "f4", (name, route)
    k = K.wg_inputs(c)
    a, keep = K.wg_shape_args(c), []
    K._fill(ops, a.src, dev, k["src"], c.c0, c.c1, c.pro, c.drop, K.SALT, keep)
    gy = k["gy"].to(dev)
    dw = torch.zeros(c.cout, c.cin_store, 3, 3).to(dev)
    ho, wo = K.wg_out_size(c)
    cin = c.c0 + c.c1
    if c.splits:
        need = max(need, 36 * c.n * (ho // 4) * (wo // 4) * (cin + c.cout) + 36 * c.cout * cin * c.splits)
    scratch = torch.full((need,), float("nan")).to(dev)
    a.g, a.splits, a.scale, a.dw, a.scratch, a.scratch_floats = gy.data_ptr(), c.splits, 0.5, dw.data_ptr(), scratch.data_ptr(), need
    L.check(lib.ssde_conv_wgrad(C.byref(a), ops._stream()), "ssde_conv_wgrad")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    arrays[name + ".dw"] = bits(dw)
    arrays[name + ".err"] = np.array([K.rel_err(dw.cpu(), 0.5 * k["ref"])])
    arrays[name + ".scratch"] = bits(scratch)


def dump(path, cuda):
    import emu
    dev = torch.device("cuda:0" if cuda else "cpu")
    arrays, launches = {}, 0
    with contextlib.nullcontext() if cuda else emu.emulated():
        ops, lib = K._ops()
        for c, cus, shares, ev in forward_cases():
            for form in K.FORMS:
                name = "%s%s%s|%s" % (K.fwd_id(c), "-cus" + cus if cus else "", "-emitv" if ev else "", form)
                with K._Env({"SSDE_NUM_CUS": cus} if cus else {}):
                    run_forward(dev, lib, ops, c, form, shares, ev, arrays, name)
                launches += 1
        for c in K.WGRAD_CASES:
            if c.form == "f4" and c.runs == "f4":
                run_wgrad(dev, lib, ops, c, arrays, "wgrad-" + K.wg_id(c))
                launches += 1
    np.savez(path, **arrays)
    print("%d arrays of %d launches -> %s" % (len(arrays), launches, path))


def differing(A, B):
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        if not k.endswith(".err") and not np.array_equal(A[k], B[k]):
            bad.append(k)
    return bad


def compare(a, b, unstable):
    A, B = np.load(a), np.load(b)
    excused = set(differing(np.load(unstable[0]), np.load(unstable[1]))) if unstable else set()
    bad = []
    for k in differing(A, B):
        if k in excused:
            e = k.rsplit(".", 1)[0] + ".err"
            ea, eb = float(A[e][0]), float(B[e][0])
            print("not reproduced by one build either: %s (fp64 error %.3g / %.3g)" % (k, ea, eb))
            if not (ea < K.TOL_OP and eb < K.TOL_OP):
                bad.append(k)
            continue
        bad.append(k)
        print("DIFFERS %s: %d of %d words" % (k, int((A[k] != B[k]).sum()) if k in A.files and k in B.files and A[k].shape == B[k].shape else -1,
                                               A[k].size if k in A.files else -1))
    worst = max(float(X[k][0]) for X in (A, B) for k in X.files if k.endswith(".err"))
    print("%d arrays, %d differ or are missing, %d excused; largest fp64 error %.3g" % (len(set(A.files) | set(B.files)), len(bad), len(excused), worst))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--cuda", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--unstable", nargs=2, metavar=("P1", "P2"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.unstable))
    dump(args.out, args.cuda)
