#!/usr/bin/env python
"""Record what the library's three plan queries -- ssde_conv_lds_bytes, ssde_conv_gn_slices, ssde_conv_ws_floats -- answer over a
grid of convolution launches (CPU only: the queries touch no device): tests/golden/conv_plan_queries.json, which
tests/test_host_cpu.py recomputes and compares.  Run it on the commit whose answers are to be kept, BEFORE a change to the
dispatch (csrc/conv_mfma.hip and the launchers behind it) that is meant to leave them alone.

A combination is (SSDE_NUM_CUS, tile, ksize, aux, stride, pad_end, prologue, gn_part, flags, weights given); its points are (map, batch, input
channels as (c0, c1), output channels), last axis fastest: the FULL grid for the combinations that reach a route's accepting
shapes, the SMALL one for the rest (a fused 1x1 source, stride 2, end padding, tile ids nobody owns).  The file holds the axes,
`answers` (the distinct [lds_bytes, gn_slices, ws_floats, route prefix of ssde_last_error() when lds_bytes < 0]) and per
combination one string of `width` base-36 digits per point: the index into `answers`.
usage: record_conv_plans.py [out.json]"""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from score_sde_pytorch_amd import _lib as L   # noqa: E402

MAPS, BATCHES, C_OUT = [4, 6, 8, 12, 16, 32, 64], [1, 16, 256], [3, 4, 32, 96, 256, 768]
C_IN = [(c, 0) for c in (4, 8, 12, 32, 128, 512, 2048)] + [(c // 2, c // 2) for c in (4, 8, 12, 32, 128, 512, 2048)]
FULL = list(itertools.product(MAPS, BATCHES, C_IN, C_OUT))
SMALL = list(itertools.product([4, 8, 16], [16], [(8, 0), (128, 0), (2048, 0), (64, 64)], [4, 96, 256]))
TILES = list(range(L.TILE_AUTO, L.TILE_WINOGRAD4P + 1))
FLAGS = [0, L.CONVF_NO_KSPLIT, L.CONVF_BF16X6, L.CONVF_NO_SMALL_COUT]
ROUTES = ("f2", "f4", "f4r", "f4p", "1x1", "small", "direct")
_WINO = {L.TILE_WINOGRAD: "f2", L.TILE_WINOGRAD4: "f4", L.TILE_WINOGRAD4R: "f4r", L.TILE_WINOGRAD4P: "f4p"}
_PTR = 0x1000                                  # the queries look at pointers only to see whether they are there


def combinations():
    """[((cus, tile, ksize, aux, stride, pad_end, pro, gn_part, flags, weights), points)]"""
    out = []
    for tile in TILES:
        owned = tile not in (7, 8)               # (7, 8: tile ids of kernels that are no longer built)
        for pro, gn_part in itertools.product((0, 1), (0, 1)):
            # plain 3x3 and 1x1-only launches: where every route accepts
            out.append(((256, tile, 3, 0, 1, 0, pro, gn_part, 0, 1), FULL if owned else SMALL))
            out.append(((256, tile, 0, 1, 1, 0, pro, gn_part, 0, 1), FULL if tile <= L.TILE_256x32 else SMALL))
            # a fused 1x1 source, stride 2, end padding
            for aux, stride, pad_end in itertools.product((0, 1), (1, 2), (0, 1)):
                if (aux, stride, pad_end) != (0, 1, 0):
                    out.append(((256, tile, 3, aux, stride, pad_end, pro, gn_part, 0, 1), SMALL))
        out.append(((256, tile, 0, 0, 1, 0, 0, 0, 0, 1), SMALL))                    # neither source
        for ksize in (3, 0):                                                         # no weights
            out.append(((256, tile, ksize, int(ksize == 0), 1, 0, 0, 0, 0, 0), SMALL))
    # the switches that reach a plan: flags and the CU count (the shares of the position-batched route, the GEMM's tile shapes)
    for tile, ksize in ((L.TILE_AUTO, 3), (L.TILE_WINOGRAD4P, 3), (L.TILE_AUTO, 0)):
        for cus, flags in [(256, f) for f in FLAGS[1:]] + [(128, 0), (128, L.CONVF_BF16X6)]:
            out.append(((cus, tile, ksize, int(ksize == 0), 1, 0, 1, int(ksize == 0), flags, 1), FULL))
    return out


def key_of(combo):
    return "/".join(str(v) for v in combo)


def args_of(combo, point):
    _, tile, ksize, aux, stride, pad_end, pro, gn_part, flags, weights = combo
    hw, n, (c0, c1), c_out = point
    a = L.ConvArgs()
    a.dst, a.n, a.h_out, a.w_out, a.c_out, a.tile, a.flags, a.out_scale = _PTR, n, hw, hw, c_out, tile, flags, 1.0
    a.h_in = a.w_in = hw * stride
    a.ksize, a.stride, a.pad, a.pad_end = ksize, stride, int(ksize == 3), pad_end
    a.gn_part = _PTR if gn_part else None

    def fill(s, c0, c1, pro):
        s.p0, s.c0, s.c1, s.p1 = _PTR, c0, c1, (_PTR if c1 else None)
        if pro:                                  # GroupNorm + SiLU with 32 groups, or the most the channel count divides by
            g = 32
            while (c0 + c1) % g:
                g //= 2
            s.pro_mode, s.gn_groups = L.PRO_GN_SILU, g
            s.gn_mean = s.gn_rstd = s.gn_gamma = s.gn_beta = _PTR
    if ksize == 3:
        fill(a.main, c0, c1, pro)
        a.w_main = _PTR if weights else None
        if aux:
            fill(a.aux, c0 + c1, 0, 0)
            a.w_aux = _PTR if weights else None
    elif aux:
        fill(a.aux, c0, c1, pro)
        a.w_aux = _PTR if weights else None
    return a


def route_of(combo, point):
    """the row of the library's route table that a launch reaches (its `wants`, in the table's order)"""
    _, tile, ksize, aux, stride, pad_end, pro, gn_part, flags, weights = combo
    hw, n, (c0, c1), c_out = point
    if tile in _WINO:
        return _WINO[tile]
    if ksize == 0 and aux and tile == L.TILE_AUTO and c_out >= 96 and n * hw * hw >= 128:
        return "1x1"
    if (ksize == 3 and not aux and tile == L.TILE_AUTO and not (flags & L.CONVF_NO_SMALL_COUT) and stride == 1 and pad_end == 0
            and 1 <= c_out <= 4 and (c0 + c1) >= 8 and (c0 + c1) % 8 == 0 and c0 % 4 == 0 and not gn_part):
        return "small"
    return "direct"


def record():
    """{combination key: [(lds_bytes, gn_slices, ws_floats, error prefix) per point]}; sets SSDE_NUM_CUS and restores it."""
    lib = L.load()
    saved = os.environ.get("SSDE_NUM_CUS")
    out = {}
    try:
        for combo, points in combinations():
            os.environ["SSDE_NUM_CUS"] = str(combo[0])
            row = []
            for pt in points:
                ref = C.byref(args_of(combo, pt))
                lds = lib.ssde_conv_lds_bytes(ref)
                prefix = lib.ssde_last_error().decode().split(":")[0] if lds < 0 else ""
                row.append((lds, lib.ssde_conv_gn_slices(ref), int(lib.ssde_conv_ws_floats(ref)), prefix))
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
            seen[route_of(combo, pt)][ans[0] < 0] += 1
    return seen


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
    return dict(axes=dict(maps=MAPS, batch=BATCHES, c_in=C_IN, c_out=C_OUT, tiles=TILES, flags=FLAGS, small=SMALL),
                answers=answers, width=width, rows=rows)


def decode(rec):
    w, answers = rec["width"], [tuple(a) for a in rec["answers"]]
    return {k: [answers[int(s[i:i + w], 36)] for i in range(0, len(s), w)] for k, s in rec["rows"].items()}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_plan_queries.json")
    got = record()
    with open(path, "w") as f:
        rec = encode(got)                      # one line per key, one per combination
        for k in ("answers", "axes", "width"):
            f.write('%s"%s":%s,\n' % ("{" if k == "answers" else "", k, json.dumps(rec[k], separators=(",", ":"))))
        f.write('"rows":{\n' + ",\n".join('"%s":"%s"' % kv for kv in sorted(rec["rows"].items())) + "\n}}\n")
    print("%d combinations, %d points" % (len(got), sum(len(r) for r in got.values())))
    for route, (ok, refused) in census(got).items():
        print("%-7s accepted %6d  refused %6d" % (route, ok, refused))
