#!/usr/bin/env python
"""Record how the library plans weight-gradient launches: tests/golden/wgrad_plan_queries.json, which tests/test_host_cpu.py
(queries) and tests/test_emulated_kernels.py (launches) recompute and compare.  Run it on the commit whose answers are to be kept,
BEFORE a change to the dispatch (csrc/wgrad.hip and the routes behind it) that is meant to leave them alone.

(a) Queries (CPU only: they touch no device).  ssde_wgrad_scratch_floats, ssde_wgrad_wants_winograd4 and the route prefix of
ssde_last_error() on refusal.  A combination is (SSDE_NUM_CUS, ksize, stride, pad_end, transpose_out, prologue, short cin_store,
g_off, columns of g beyond the block, flags); its points are (map, batch, input channels as (c0, c1), output channels), last axis
fastest: the FULL grid for the combinations that reach a route's accepting shapes, the SMALL one for the rest.  Every combination
is recorded a second time with SSDE_WGRADF_DIRECT added.  The file holds the axes, `answers` (the distinct [scratch floats,
wants F(4x4,3x3), error prefix]), `strings` (the distinct strings of `width` base-36 digits per point: the index into `answers`)
and per combination the index of its string.

(b) Launches under the kernel emulator (tests/emu, built without floating-point contraction: its bits are reproducible).  The
split a launch takes decides the order of its sums, hence the bits of dw: `launches` maps each case of CASES to the SHA-256 of dw
after ssde_conv_wgrad.  The fixture is only written when the splits=1 and splits=2 cases of every route differ and every case
agrees with fp64 autograd.

usage: record_wgrad_plans.py [out.json]             record everything
       record_wgrad_plans.py --amend [out.json]     after a change that makes the Winograd routes refuse what the direct
           kernels always refused: re-record the query points that differ, and only if the file accepted them on a Winograd
           route and refused them with SSDE_WGRADF_DIRECT added (anything else is reported and nothing is written)"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from score_sde_pytorch_amd import _lib as L   # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "wgrad_plan_queries.json")

# ---------------------------------------------------------------------------------------------------------------- queries
MAPS, BATCHES, C_OUT = [4, 6, 8, 12, 16, 32, 64], [1, 16, 128], [3, 4, 32, 96, 256, 768]
C_IN = [(c, 0) for c in (4, 8, 12, 32, 128, 512, 2048)] + [(c // 2, c // 2) for c in (4, 8, 12, 32, 128, 512, 2048)]
FULL = list(itertools.product(MAPS, BATCHES, C_IN, C_OUT))
SMALL = list(itertools.product([4, 8, 16], [16], [(8, 0), (128, 0), (2048, 0), (64, 64)], [4, 96, 256]))
BITS = [0, L.WGRADF_DIRECT, L.WGRADF_F2, L.WGRADF_F4_FORCE, L.WGRADF_NO_STREAMK, L.WGRADF_NO_XCD_ORDER, L.WGRADF_1X1_CHUNKED,
        L.WGRADF_XVEC1]
G_COLUMNS = [(0, 0), (0, 8), (4, 0), (4, 8)]     # (g_off, g_ld - c_out rounded up to 4): (4, 0) puts the block beyond the row
ROUTES = ("f4", "f2", "1x1", "direct")         # (the shape-only queries look at no pointer: none is set)


def combinations():
    """[((cus, ksize, stride, pad_end, transpose_out, pro, cin_short, g_off, g_extra, flags), points)]"""
    base = []
    for ksize in (3, 1):
        # stride 1, no end padding: where the routes accept
        for pro, short, (g_off, g_extra) in itertools.product((0, 1), (0, 1), G_COLUMNS):
            for tr in range(1 if ksize == 3 else 2):
                base.append(((256, ksize, 1, 0, tr, pro, short, g_off, g_extra, 0), FULL))
        # the switches that reach a plan: every flag and the CU count (the stream-K groups of F(4x4,3x3))
        for flags in BITS[1:]:
            base.append(((256, ksize, 1, 0, 0, 1, 0, 0, 8, flags), FULL))
        for flags in (0, L.WGRADF_NO_STREAMK):
            base.append(((128, ksize, 1, 0, 0, 1, 0, 0, 8, flags), FULL))
        # stride 2, end padding, a transposed 3x3
        for stride, pad_end, tr, pro in itertools.product((1, 2), (0, 1), (0, 1), (0, 1)):
            if (stride, pad_end) != (1, 0) or (ksize == 3 and tr):
                base.append(((256, ksize, stride, pad_end, tr, pro, 0, 0, 0, 0), SMALL))
    out = []
    for combo, points in base:
        out.append((combo, points))
        if not combo[-1] & L.WGRADF_DIRECT:
            out.append((with_direct(combo), points))
    return out


def with_direct(combo):
    return combo[:-1] + (combo[-1] | L.WGRADF_DIRECT,)


def key_of(combo):
    return "/".join(str(v) for v in combo)


def _groups(ctot):
    g = 32                                     # GroupNorm with 32 groups, or the most the channel count divides by
    while ctot % g:
        g //= 2
    return g


def args_of(combo, point=None, a=None):
    """the shape-only arguments of a point; a: the previous point's structure of the same combination, refilled"""
    _, ksize, stride, pad_end, tr, pro, short, g_off, g_extra, flags = combo
    if a is None:
        a = L.WgradArgs()
        a.ksize, a.stride, a.pad, a.pad_end, a.transpose_out, a.flags, a.scale = ksize, stride, int(ksize == 3), pad_end, tr, flags, 1.0
        a.g_off = g_off
        if pro:
            a.src.pro_mode = L.PRO_GN_SILU
    if point is not None:
        hw, n, (c0, c1), c_out = point
        a.n, a.h_out, a.w_out, a.c_out = n, hw, hw, c_out
        a.h_in = a.w_in = hw * stride
        a.src.c0, a.src.c1 = c0, c1
        a.src.gn_groups = _groups(c0 + c1) if pro else 0
        a.g_ld = -(-c_out // 4) * 4 + g_extra
        a.cin_store = c0 + c1 - short
    return a


def route_of(combo, point, wants4):
    """the row of the library's route table that a point reaches (wants4: what ssde_wgrad_wants_winograd4 said)"""
    _, ksize, stride, pad_end, tr, pro, short, g_off, g_extra, flags = combo
    hw, n, (c0, c1), c_out = point
    if wants4:
        return "f4"
    if ksize == 1:
        return "direct" if flags & L.WGRADF_1X1_CHUNKED else "1x1"
    ctot = c0 + c1
    if (not flags & L.WGRADF_DIRECT and stride == 1 and pad_end == 0 and not tr and hw % 8 == 0 and c_out % 64 == 0
            and ctot % 64 == 0 and not short and (c1 == 0 or c0 % 64 == 0) and n * hw * hw < 2 ** 30):
        return "f2"
    return "direct"


def record():
    """{combination key: [(scratch floats, wants F(4x4,3x3), error prefix) per point]}; sets SSDE_NUM_CUS and restores it."""
    lib = L.load()
    saved = os.environ.get("SSDE_NUM_CUS")
    out = {}
    try:
        for combo, points in combinations():
            os.environ["SSDE_NUM_CUS"] = str(combo[0])
            row, a = [], args_of(combo)
            ref = C.byref(a)
            for pt in points:
                args_of(combo, pt, a)
                need = int(lib.ssde_wgrad_scratch_floats(ref))
                prefix = lib.ssde_last_error().decode().split(":")[0] if need < 0 else ""
                row.append((need, int(lib.ssde_wgrad_wants_winograd4(ref)), prefix))
            out[key_of(combo)] = row
    finally:
        if saved is None:
            os.environ.pop("SSDE_NUM_CUS", None)
        else:
            os.environ["SSDE_NUM_CUS"] = saved
    return out


def census(got):
    """{route: [accepted, refused]} of a recording"""
    seen = {r: [0, 0] for r in ROUTES}
    for combo, points in combinations():
        for pt, ans in zip(points, got[key_of(combo)]):
            seen[route_of(combo, pt, ans[1])][ans[0] < 0] += 1
    return seen


def differences(got, want):
    """(allowed, other) points where two recordings differ.  Allowed: `want` accepted the point on a Winograd route and refused
    it with SSDE_WGRADF_DIRECT added -- the direct kernels' argument checks reject it and the Winograd routes had not asked."""
    allowed, other = [], []
    for combo, points in combinations():
        key, dkey = key_of(combo), key_of(with_direct(combo))
        for i, pt in enumerate(points):
            g, w = got[key][i], want[key][i]
            if g != w:
                ok = w[0] >= 0 and route_of(combo, pt, w[1]) in ("f4", "f2") and want[dkey][i][0] < 0 and g[0] < 0
                (allowed if ok else other).append((key, pt, g, w, want[dkey][i]))
    return allowed, other


_DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"


def encode(got):
    answers = sorted({ans for row in got.values() for ans in row})
    width = 1
    while 36 ** width < len(answers):
        width += 1
    index = {}
    for i, ans in enumerate(answers):
        index[ans] = "".join(_DIGITS[i // 36 ** k % 36] for k in reversed(range(width)))
    rows = {k: "".join(index[ans] for ans in row) for k, row in got.items()}
    strings = sorted(set(rows.values()))         # (most combinations answer like another one: each distinct string once)
    return dict(axes=dict(maps=MAPS, batch=BATCHES, c_in=C_IN, c_out=C_OUT, bits=BITS, g_columns=G_COLUMNS, small=SMALL),
                answers=answers, width=width, strings=strings, rows={k: strings.index(v) for k, v in rows.items()})


def decode(rec):
    w, answers = rec["width"], [tuple(a) for a in rec["answers"]]
    strings = [[answers[int(s[i:i + w], 36)] for i in range(0, len(s), w)] for s in rec["strings"]]
    return {k: strings[i] for k, i in rec["rows"].items()}


# --------------------------------------------------------------------------------------------------------------- launches
# The smallest shapes at which each route's plan can still go wrong.  scratch: "pref" = what the query asks for (and what an
# explicit split needs, if that is more), "pref-1" = one float less, (k, extra) = the route's fixed floats + k slabs + extra.
_DEFAULTS = dict(n=2, h=8, w=8, c0=8, c1=0, c_out=12, ksize=3, stride=1, pad=1, pad_end=0, h_in=None, w_in=None, gn=0,
                 cin_store=None, g_off=0, g_extra=0, transpose_out=0, flags=0, splits=0, scratch="pref", cus=256)


def _cases():
    out = {}

    def add(name, route, **kw):
        out[name] = dict(_DEFAULTS, route=route, **kw)
    # F(4x4,3x3), forced.  n=2, 16x16: T = 32 tiles = two K stages of 16
    f4 = dict(flags=L.WGRADF_F4_FORCE, h=16, w=16, c0=32, c_out=32)
    add("f4/32-32", "f4", **f4)
    add("f4/32-32/gn", "f4", **dict(f4, gn=1))
    add("f4/16+16-64", "f4", **dict(f4, c0=16, c1=16, c_out=64))
    add("f4/16+16-64/gn", "f4", **dict(f4, c0=16, c1=16, c_out=64, gn=1))
    add("f4/ragged-stage", "f4", **dict(f4, n=3, h=8, w=8))               # T = 12
    add("f4/cus3", "f4", **dict(f4, cus=3))
    for name, bit in (("no-streamk", L.WGRADF_NO_STREAMK), ("xvec1", L.WGRADF_XVEC1), ("no-xcd-order", L.WGRADF_NO_XCD_ORDER)):
        add("f4/" + name, "f4", **dict(f4, flags=f4["flags"] | bit))
    add("f4/splits1", "f4", **dict(f4, splits=1))
    add("f4/splits2", "f4", **dict(f4, splits=2))
    add("f4/scratch-one-slab", "f4", **dict(f4, scratch=(1, 0)))
    add("f4/scratch-one-float-short", "f4", **dict(f4, scratch="pref-1"))
    # n=3, 16x16: T = 48 tiles = three K stages, which the stream-K runs of 8 stages cut inside a position (two stages per
    # position are whole positions per run: the same sums as one split)
    sk = dict(f4, n=3)
    add("f4/streamk-cut", "f4", **sk)
    add("f4/streamk-cut/no-streamk", "f4", **dict(sk, flags=sk["flags"] | L.WGRADF_NO_STREAMK))
    # F(2x2,3x3)
    f2 = dict(flags=L.WGRADF_F2, c0=64, c_out=64)
    add("f2/64-64", "f2", **f2)
    add("f2/64+64-64/gn", "f2", **dict(f2, n=1, h=4, c1=64, gn=1))
    add("f2/splits1", "f2", **dict(f2, splits=1))
    add("f2/splits2", "f2", **dict(f2, splits=2))
    add("f2/scratch-one-slab", "f2", **dict(f2, splits=2, scratch=(1, 0)))
    # the direct 3x3 kernel
    add("direct/8-12", "direct")
    add("direct/cin-store3", "direct", c0=4, cin_store=3)
    add("direct/stride2-pad-end", "direct", stride=2, pad=0, pad_end=1, h=4, w=4, h_in=9, w_in=9)
    add("direct/4+4/gn", "direct", c0=4, c1=4, gn=1)
    add("direct/splits1", "direct", splits=1)
    add("direct/splits2", "direct", splits=2)
    add("direct/scratch-one-slab", "direct", splits=2, scratch=(1, 0))
    # 1x1: the pipelined GEMM and the chunked kernel.  n=2, 8x8: 128 rows = 8 stages of 16
    for route, bit in (("1x1", 0), ("chunked", L.WGRADF_1X1_CHUNKED)):
        for tr in (0, 1):
            k1 = dict(ksize=1, pad=0, c0=72, c_out=72, g_off=4, g_extra=4, transpose_out=tr, flags=bit)
            tag = "%s/%s" % (route, "transposed" if tr else "plain")
            add(tag, route, **k1)
            add(tag + "/splits1", route, **dict(k1, splits=1))
            add(tag + "/splits2", route, **dict(k1, splits=2))
            add(tag + "/short-scratch", route, **dict(k1, splits=4, scratch=(2, 1)))      # room for two slabs and a float
    return out


CASES = _cases()
# per route, a pair of cases that differ in the split alone: their hashes must differ, or the cases do not see the split
SPLIT_PAIRS = [("f4/splits1", "f4/splits2"), ("f4/streamk-cut", "f4/streamk-cut/no-streamk"), ("f2/splits1", "f2/splits2"),
               ("direct/splits1", "direct/splits2"), ("1x1/plain/splits1", "1x1/plain/splits2"), ("1x1/transposed/splits1", "1x1/transposed/splits2"),
               ("chunked/plain/splits1", "chunked/plain/splits2"), ("chunked/transposed/splits1", "chunked/transposed/splits2")]
TOLERANCE = 2e-5                               # tests/test_emulated_kernels.py: fp32, per contraction


def _slab_floats(c):
    """(fixed, per split) scratch floats of a case's route"""
    ctot, c_out, cin = c["c0"] + c["c1"], c["c_out"], c["cin_store"] or c["c0"] + c["c1"]
    if c["route"] == "f4":
        tiles = c["n"] * (c["h"] // 4) * (c["w"] // 4)
        return 36 * tiles * (ctot + c_out), 36 * c_out * ctot
    if c["route"] == "f2":
        return 0, (c_out // 64) * (ctot // 64) * 16 * 64 * 64
    edge = 64 if c["ksize"] == 3 else 128
    return 0, c["ksize"] ** 2 * (-(-c_out // edge) * edge) * (-(-cin // edge) * edge)


def _uniform(rs, *shape):
    """seeded values in [-1, 1) with full mantissas, by integer arithmetic alone: the same bits on every machine"""
    return (rs.random_sample(shape) * 2.0 - 1.0).astype(np.float32)


def launch(lib, c, check=True):
    """run one case under the emulator: (SHA-256 of dw's bytes, relative error against fp64 autograd or None when not checked)"""
    import torch
    import torch.nn.functional as F
    n, h, w, c0, c1, c_out, ks = c["n"], c["h"], c["w"], c["c0"], c["c1"], c["c_out"], c["ksize"]
    h_in, w_in = c["h_in"] or h, c["w_in"] or w
    ctot, cin = c0 + c1, c["cin_store"] or c0 + c1
    rs = np.random.RandomState(1000 * n + 100 * h_in + 10 * ctot + c_out)
    x = torch.from_numpy(_uniform(rs, n, h_in, w_in, ctot))
    gy = torch.from_numpy(_uniform(rs, n, h, w, c_out))
    x0, x1 = x[..., :c0].contiguous(), (x[..., c0:].contiguous() if c1 else None)
    g_ld = c["g_off"] + c_out + c["g_extra"]
    g = torch.from_numpy(_uniform(rs, n, h, w, g_ld))
    g[..., c["g_off"]:c["g_off"] + c_out] = gy
    a = L.WgradArgs()
    a.src.p0, a.src.c0, a.src.p1, a.src.c1 = x0.data_ptr(), c0, (x1.data_ptr() if c1 else None), c1
    act = x.double()
    if c["gn"]:
        # GroupNorm apply with seeded statistics (the kernels take mean and rstd as given), no SiLU: no libm in the bits
        groups = ctot // 4
        mean = torch.from_numpy(0.25 * _uniform(rs, n, groups))
        rstd = torch.from_numpy(1.0 + 0.25 * _uniform(rs, n, groups))
        gamma = torch.from_numpy(1.0 + 0.25 * _uniform(rs, ctot))
        beta = torch.from_numpy(0.25 * _uniform(rs, ctot))
        a.src.pro_mode, a.src.gn_groups = L.PRO_GN, groups
        a.src.gn_mean, a.src.gn_rstd, a.src.gn_gamma, a.src.gn_beta = (t.data_ptr() for t in (mean, rstd, gamma, beta))
        m, r = (t.double().repeat_interleave(4, dim=1)[:, None, None, :] for t in (mean, rstd))
        act = (act - m) * r * gamma.double() + beta.double()
    a.g, a.g_ld, a.g_off = g.data_ptr(), g_ld, c["g_off"]
    a.n, a.h_in, a.w_in, a.h_out, a.w_out, a.c_out = n, h_in, w_in, h, w, c_out
    a.ksize, a.stride, a.pad, a.pad_end = ks, c["stride"], c["pad"], c["pad_end"]
    a.cin_store, a.transpose_out, a.flags, a.scale = cin, c["transpose_out"], c["flags"], 0.5
    dw = torch.zeros((cin, c_out) if c["transpose_out"] else (c_out, cin, ks, ks))
    a.dw = dw.data_ptr()
    saved = os.environ.get("SSDE_NUM_CUS")
    os.environ["SSDE_NUM_CUS"] = str(c["cus"])
    try:
        pref = int(lib.ssde_wgrad_scratch_floats(C.byref(a)))
        L.check(min(pref, 0), "ssde_wgrad_scratch_floats")
        fixed, per = _slab_floats(c)
        if c["scratch"] == "pref":
            floats = max(pref, fixed + per * c["splits"])
        elif c["scratch"] == "pref-1":
            floats = pref - 1
        else:
            floats = fixed + per * c["scratch"][0] + c["scratch"][1]
        scratch = torch.full((max(floats, 1),), float("nan"))
        a.splits, a.scratch, a.scratch_floats = c["splits"], scratch.data_ptr(), floats
        L.check(lib.ssde_conv_wgrad(C.byref(a), None), "ssde_conv_wgrad")
    finally:
        if saved is None:
            os.environ.pop("SSDE_NUM_CUS", None)
        else:
            os.environ["SSDE_NUM_CUS"] = saved
    digest = hashlib.sha256(dw.numpy().tobytes()).hexdigest()
    if not check:
        return digest, None
    wt = torch.zeros(c_out, ctot, ks, ks, dtype=torch.float64, requires_grad=True)
    act = F.pad(act.permute(0, 3, 1, 2), (0, c["pad_end"], 0, c["pad_end"]))
    y = F.conv2d(act, wt, stride=c["stride"], padding=c["pad"])[:, :, :h, :w]
    y.backward(gy.double().permute(0, 3, 1, 2))
    ref = 0.5 * wt.grad[:, :cin]
    if c["transpose_out"]:
        ref = ref[:, :, 0, 0].t()
    err = float((dw.double() - ref).abs().max() / ref.abs().max())
    return digest, err


def launch_hashes(names=None, check=True):
    """{case: (hash, error against fp64 if checked)} under the emulator"""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import emu
    lib = emu.lib()
    return {name: launch(lib, CASES[name], check) for name in (names or CASES)}


def _write(path, rec, launches):
    with open(path, "w") as f:                 # one line per key, one per launch, combination and distinct string
        for k in ("answers", "axes", "width"):
            f.write('%s"%s":%s,\n' % ("{" if k == "answers" else "", k, json.dumps(rec[k], separators=(",", ":"))))
        f.write('"launches":{\n' + ",\n".join('"%s":"%s"' % kv for kv in sorted(launches.items())) + "\n},\n")
        f.write('"rows":{\n' + ",\n".join('"%s":%d' % kv for kv in sorted(rec["rows"].items())) + "\n},\n")
        f.write('"strings":[\n' + ",\n".join('"%s"' % v for v in rec["strings"]) + "\n]}\n")


def main(argv):
    amend = "--amend" in argv
    argv = [v for v in argv if v != "--amend"]
    path = argv[0] if argv else FIXTURE
    got = record()
    print("%d combinations, %d points" % (len(got), sum(len(r) for r in got.values())))
    for route, (ok, refused) in census(got).items():
        print("%-7s accepted %6d  refused %6d" % (route, ok, refused))
    if amend:
        with open(path) as f:
            old = json.load(f)
        allowed, other = differences(got, decode(old))
        print("%d points differ as allowed (by the direct kernels' refusal: %s), %d otherwise"
              % (len(allowed), sorted({d[4][2] for d in allowed}), len(other)))
        for d in other[:20]:
            print("  ", d)
        if other:
            raise SystemExit("not written")
        _write(path, encode(got), old["launches"])
        return
    runs = launch_hashes()
    for name, (digest, err) in runs.items():
        print("%-34s %s  %.2e" % (name, digest[:16], err))
    same = [p for p in SPLIT_PAIRS if runs[p[0]][0] == runs[p[1]][0]]
    wrong = [n for n, (_, err) in runs.items() if not err < TOLERANCE]
    if same or wrong:
        raise SystemExit("not written: split pairs with equal hashes %s, cases beyond %g of fp64 %s" % (same, TOLERANCE, wrong))
    _write(path, encode(got), {n: r[0] for n, r in runs.items()})


if __name__ == "__main__":
    main(sys.argv[1:])
