"""Checks of the 3x3 convolution routes (ssde_conv2d: the rows f2, f4, f4r, f4p, 1x1, small and direct of kRoutes in
csrc/conv_mfma.hip) and of the weight-gradient routes (ssde_conv_wgrad: f4, f2, direct of kRoutes in csrc/wgrad.hip) on the maps
their plans accept but the square power-of-two cases of the older checks never reach: rectangular maps, maps that are no
multiple of a workgroup's tile (partial last tile column / row), several whole images per workgroup with a ragged batch tail,
strides, end padding, cropped outputs, explicit and preferred splits.  Shared by the emulator suite
(tests/test_conv_shapes_cpu.py) and the GPU suite (tests/test_conv_shapes_gpu.py).

Reference: fp64 torch on the CPU (F.conv2d of the fp64 prologue; fp64 autograd for the weight gradient; the dropout mask is the
numpy restatement of the hash, _train_checks.hash_keep).  The kernels are handed the fp32 rounding of the fp64 GroupNorm
statistics of their source, so every figure is the convolution's own.  Error: max-abs error over max-abs reference value
(_util.rel_err) against TOL_OP = 2e-5 for every tensor; GroupNorm partials of the result, merged by ssde_gn_finalize, against
the fp64 statistics of the fp64 REFERENCE output (1e-5 on the mean, 1e-4 relative on rstd) -- never against statistics of the
kernel's own output, which would let a wrong output and matching wrong statistics pass together.

Every launch is planned first (ssde_conv_lds_bytes / ssde_wgrad_scratch_floats): a listed case that its plan refuses is a
failure.  A forced Winograd tile never falls back, so acceptance plus the forced tile proves the forward route; the route of a
weight gradient is read from ssde_wgrad_wants_winograd4 and from the scratch its plan asks for (the three routes size it
differently), and a row whose flag falls back to another kernel is listed under the kernel it runs.

The tiling states each case is listed for (the `states` of a row) are restated from the plan functions below (wino_tiling,
direct_tiling, wgrad_direct_tiling) and asserted by check_table_states, so a row cannot claim a state it does not hit.

The fourth form of every forward row, "accumulate-in-place", is the launch the backward lowering issues for every input
gradient (TrainEngine._bwd_branch): dst preloaded with a base, resid == dst, resid_post = 1, out_scale = 0.7, no bias / addend /
partials, against fp64 0.7 conv + base.  Every kernel reads the residual it overwrites, and the split reductions use dst as
the hand-over buffer between workgroups: the rows where the alias changes the plan (direct 128+0-64-4x8 t3, f4 128+0-64-8x12,
f4r 128+128-64-8x12, f4p ks2 / ks4) are the point of the form -- see check_forward.  Two 1x1 rows force the persistent and the
128 x 256 GEMM kernels, so that three GEMM kernels run aliased.

Largest errors seen (every check prints its own); the bound is 2e-5 everywhere, 1e-5 / 1e-4 for the finalized mean / rstd:
                                   emulator (exact fp32)   MI355X (both matrix modes; the first three forms)
  forward  f2                      2.7e-7                  2.7e-7
           f4 / f4r / f4p          6.0e-6 / 6.7e-6 / 5.8e-6   5.0e-6 / 6.7e-6 / 6.0e-6
           direct / small / 1x1    1.0e-6 / 3.5e-7 / 5.0e-7   1.0e-6 / 3.5e-7 / 3.5e-7
           partials: mean, rstd    7.5e-7, 5.3e-7          4.7e-7, 6.2e-7
  of these, accumulate-in-place (not measured on the MI355X yet):
           f2                      2.2e-7                  -
           f4 / f4r / f4p          6.0e-6 / 6.5e-6 / 5.6e-6   -
           direct / small / 1x1    1.0e-6 / 2.5e-7 / 4.5e-7   -
  wgrad    f4 / f2 / direct        1.7e-6 / 4.2e-7 / 5.5e-7   1.7e-6 / 2.7e-7 / 4.9e-7
The sweep (emulator only): 330 draws, 20 refused, 21 to 30 accepted launches per route and form of the weight gradient, 45 to 50
forward launches per form, largest error 4.2e-6.  The forms are drawn from a stream of their own, so the drawn shapes are
those of the sweep before the fourth form.
The tables found no kernel wrong.  The sweep found one fault: conv_wino.hip and conv_wino4.hip put the gamma / beta table,
which they read as float4, in LDS behind 2 x images x groups floats of (mean, rstd) -- 8 bytes off a 16-byte boundary when one
image per workgroup meets an odd number of GroupNorm groups (12 channels in 3 groups on a 16x24 map: the emulator's aligned
16-byte load faults; the networks' 32 groups never get there).  The kernels and their plans now round that table up to whole
float4s; the f2 row 1-12+0-72-16x24 and the f4 row 1-12+0-40-20x32 keep the layout in the table.
"""
import ctypes as C
import functools
import math
import os
import random
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import _train_checks as T
from _util import rel_err
from score_sde_pytorch_amd import _lib as L

TOL_OP = T.TOL_OP
assert TOL_OP == 2e-5
TOL_MEAN, TOL_RSTD = 1e-5, 1e-4          # finalized GroupNorm partials (_wino4p_checks.run_case, _train_checks.check_conv_winograd4)
DROP_P, SALT, SEED_WORD = 0.25, 0x2545F49, 91
EPS = 1e-6

# the tiling states a row can be listed for
COL, ROW, IMGS_TAIL, MANY_TILES = "partial-column", "partial-row", "images-per-workgroup-ragged-tail", "tiles-per-image>1"


def _ops():
    from score_sde_pytorch_amd import hipops as ops
    return ops, L.load()


def pow2_floor(v):
    q = 1
    while q * 2 <= v:
        q *= 2
    return q


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the plans, restated
def _states(n, h, w, tw, th, imgs):
    """the states of a tiling of h x w output pixels by tiles of th x tw pixels, imgs whole images per workgroup"""
    s = set()
    if w % tw:
        s.add(COL)
    if h % th:
        s.add(ROW)
    if imgs > 1 and n % imgs:
        s.add(IMGS_TAIL)
    if cdiv(w, tw) * cdiv(h, th) > 1:
        s.add(MANY_TILES)
    return s


def wino_tiling(route, n, h, w):
    """ssde_wino_tiling_fill (csrc/ssde_common.h): a workgroup owns `tiles` output tiles of edge x edge pixels, twt x tht of each
    of imgs images.  Returns (pixels per workgroup tile along w, along h, images per workgroup)."""
    edge, tiles = (2, 64) if route == "f2" else (4, 32)
    twt = pow2_floor(min(w // edge, 8))
    tht = pow2_floor(min(tiles // twt, h // edge))
    return edge * twt, edge * tht, tiles // (twt * tht)


DIRECT_TILES = {L.TILE_256x64: (256, 64), L.TILE_128x64: (128, 64), L.TILE_64x64: (64, 64), L.TILE_256x32: (256, 32)}


def direct_tiling(tile, h_out, w_out, stride):
    """halo_px / make_plan (csrc/conv_mfma.hip) for an explicit tile: (the tile that runs, tw, th, imgs).  A tile whose halo exceeds
    the staging plan (5 x 256 float4 items, two channel quads per pixel) is exchanged for the next smaller one."""
    while True:
        bm = DIRECT_TILES[tile][0]
        tw = pow2_floor(min(w_out, 16))
        th = pow2_floor(min(bm // tw, h_out))
        imgs = bm // (tw * th)
        if imgs * ((th - 1) * stride + 3) * ((tw - 1) * stride + 3) * 2 <= 5 * 256:
            return tile, tw, th, imgs
        assert tile != L.TILE_64x64
        tile = L.TILE_64x64 if tile == L.TILE_256x32 else tile + 1


def wgrad_direct_tiling(h_out, w_out, stride):
    """chunked_plan_params (csrc/wgrad.hip), ksize 3: (tw, th, imgs) of a chunk of px output pixels"""
    px = 32 if stride == 2 else (128 if h_out * w_out >= 128 else 64)
    tw = pow2_floor(min(w_out, 16))
    th = pow2_floor(min(px // tw, h_out))
    return tw, th, px // (tw * th)


def out_size(c):
    if c.out_hw is not None:
        return c.out_hw
    if c.route == "1x1":
        return c.h, c.w
    return ((c.h + 2 * c.pad + c.pad_end - 3) // c.stride + 1, (c.w + 2 * c.pad + c.pad_end - 3) // c.stride + 1)


# ------------------------------------------------------------------------------------------------ forward: the case table
Fwd = namedtuple("Fwd", "route n c0 c1 cout h w tile flags stride pad pad_end out_hw aux drop states")
TILE_OF = {"f2": L.TILE_WINOGRAD, "f4": L.TILE_WINOGRAD4, "f4r": L.TILE_WINOGRAD4R, "f4p": L.TILE_WINOGRAD4P, "small": L.TILE_AUTO,
           "1x1": L.TILE_AUTO}
# what the message of a refusal calls the route (the prefix of every SSDE_REQUIRE of its plan)
ROUTE_IN_MESSAGE = {"f2": "conv(winograd):", "f4": "conv(winograd 4x4):", "f4r": "conv(winograd 4x4, register-fed):",
                    "f4p": "conv(winograd 4x4, position-batched):", "direct": "conv:"}
FLAG_NAMES = {L.CONVF_NO_KSPLIT: "noksplit", L.CONVF_BKC8: "bkc8", L.CONVF_KSPLIT2: "ks2", L.CONVF_KSPLIT4: "ks4",
              L.CONVF_NO_SMALL_COUT: "nosmall", L.CONVF_BF16X6: "x6", L.CONVF_GEMM_PIPE: "pipe", L.CONVF_X6_WIDE: "wide"}
# the 1x1 rows that force a GEMM kernel of conv1x1.hip other than the one the launch would get (both exist in the 3-way bf16 split
# only, so the rows pin that matrix mode): the persistent pipelined kernel on a pretend 3-CU device, where 8 workgroups share
# the tiles and some own several (SSDE_NUM_CUS is read by the library at every plan), and the 128 x 256 tile
GEMM_FORCED = L.CONVF_GEMM_PIPE | L.CONVF_X6_WIDE


def row_env(c):
    return {"SSDE_NUM_CUS": "3"} if c.route == "1x1" and c.flags & L.CONVF_GEMM_PIPE else {}


class _Env:
    """the environment of a row around its plan queries and launches, put back afterwards"""

    def __init__(self, env):
        self.env, self.saved = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.saved[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fwd(route, n, c0, c1, cout, h, w, tile=None, flags=0, stride=1, pad=1, pad_end=0, out_hw=None, aux=None, drop=False, states=()):
    return Fwd(route, n, c0, c1, cout, h, w, TILE_OF[route] if tile is None else tile, flags, stride, pad, pad_end, out_hw, aux, drop,
               tuple(states))


def fwd_id(c):
    s = "%s-n%d-%d+%d-%d-%dx%d" % (c.route, c.n, c.c0, c.c1, c.cout, c.h, c.w)
    if c.route == "direct":
        s += "-t%d-s%dp%de%d" % (c.tile, c.stride, c.pad, c.pad_end)
    if c.out_hw:
        s += "-crop%dx%d" % c.out_hw
    if c.aux:
        s += "-aux%d+%d" % c.aux
    for bit, name in FLAG_NAMES.items():
        if c.flags & bit:
            s += "-" + name
    return s + ("-drop" if c.drop else "")


def _wino_rows(route):
    """f2, f4, f4r share ssde_wino_tiling_fill; f4 / f4r: 32 tiles of 4x4 pixels per workgroup (within 24 pixels per side every
    tiling has 2 images or more per workgroup), f2: 64 tiles of 2x2 pixels."""
    c8 = route != "f4"           # (f4r: input channels % 8; f2: concat boundary % 8)
    rows = [
        fwd(route, 2, 8, 0, 64, 8, 12, states=[COL, IMGS_TAIL, MANY_TILES]),           # 12 px: one tile column of 8 and half a one
        fwd(route, 3, 16, 0, 40, 12, 8, states=[ROW, IMGS_TAIL, MANY_TILES]),          # cout does not fill the 64 tile; 3 of 8 images
        fwd(route, 1, 32, 32, 72, 12, 20, states=[COL, ROW, IMGS_TAIL, MANY_TILES], drop=True),   # both; a concat source; cout 64 + 8
        fwd(route, 3, 24 if c8 else 20, 0, 132, 20, 12, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),   # three cout tiles, the last of 4
        fwd(route, 5, 8, 0, 64, 24, 8, states=[ROW, IMGS_TAIL, MANY_TILES]),           # 24 rows: a tile row of 16 and half a one
        fwd(route, 9, 16, 16, 64, 8, 8, states=[IMGS_TAIL]),                           # whole images, 9 = 8 + 1: GroupNorm partials
        fwd(route, 5, 32, 0, 96, 8, 16, states=[IMGS_TAIL]),                           # whole 8x16 images, partials, 5 = 4 + 1 / 2 + 2 + 1
    ]
    if route == "f2":
        rows += [
            fwd(route, 3, 8, 8, 64, 10, 14, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),     # even, no multiple of 4: f2 only
            fwd(route, 2, 16, 0, 40, 20, 20, states=[COL, ROW, MANY_TILES]),             # one image per workgroup (16x16 px): partials
            fwd(route, 1, 8, 0, 64, 24, 16, states=[ROW, MANY_TILES]),                   # one image per workgroup, partial rows only
            # 12 channels in 3 GroupNorm groups, one image per workgroup: an odd number of (mean, rstd) pairs in front of the
            # gamma / beta table in LDS, which is read as float4 (it stood 8 bytes off a 16-byte boundary: the sweep found it)
            fwd(route, 1, 12, 0, 72, 16, 24, states=[COL, MANY_TILES]),
        ]
    if route == "f4":
        # 128 channels on 8 workgroups: the reduction is split over two workgroups per tile (ssde_conv_wino4_splits), and not
        rows += [fwd(route, 2, 128, 0, 64, 8, 12, states=[COL, IMGS_TAIL, MANY_TILES]),
                 fwd(route, 2, 128, 0, 64, 8, 12, flags=L.CONVF_NO_KSPLIT, states=[COL, IMGS_TAIL, MANY_TILES]),
                 # one image per workgroup (16x32 px) and 3 GroupNorm groups: the same LDS layout as the f2 row of 12 channels
                 fwd(route, 1, 12, 0, 40, 20, 32, states=[ROW, MANY_TILES])]
    if route == "f4r":
        # 256 channels on 8 workgroups: the register-fed kernel's own split, four shares (ssde_conv_wino4r_splits), and not
        rows += [fwd(route, 2, 128, 128, 64, 8, 12, states=[COL, IMGS_TAIL, MANY_TILES]),
                 fwd(route, 2, 128, 128, 64, 8, 12, flags=L.CONVF_NO_KSPLIT, states=[COL, IMGS_TAIL, MANY_TILES])]
    return rows


def _f4p_rows():
    """f4p has no tile grid: 36 GEMMs over T = n * h/4 * w/4 tile rows in blocks of 64 (every T below is no multiple of 64: a
    partial block), one GroupNorm slice per tile; the shares of the reduction are forced.  192 channels take 1 / 2 / 2 shares."""
    rows = []
    for ks in (L.CONVF_NO_KSPLIT, L.CONVF_KSPLIT2, L.CONVF_KSPLIT4):
        rows += [fwd("f4p", 3, 32, 0, 40, 4, 8, flags=ks), fwd("f4p", 2, 32, 32, 132, 8, 4, flags=ks, drop=ks == L.CONVF_KSPLIT2),
                 fwd("f4p", 1, 64, 0, 64, 12, 12, flags=ks), fwd("f4p", 5, 128, 64, 8, 24, 8, flags=ks)]
    return rows


def _direct_rows():
    t1, t2, t3, t4 = L.TILE_256x64, L.TILE_128x64, L.TILE_64x64, L.TILE_256x32
    return [
        # stride 1 / pad 1, every tile, 12x20: 16 pixels wide tiles leave a column of 4
        fwd("direct", 3, 8, 0, 64, 12, 20, tile=t1, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),      # 8x16 px, 2 images
        fwd("direct", 2, 16, 0, 40, 12, 20, tile=t2, states=[COL, ROW, MANY_TILES]),                # 8x16 px, 1 image: partials
        fwd("direct", 1, 32, 32, 72, 12, 20, tile=t3, states=[COL, MANY_TILES], drop=True),         # 4x16 px; 64-channel stages
        fwd("direct", 1, 32, 32, 72, 12, 20, tile=t3, flags=L.CONVF_BKC8, states=[COL, MANY_TILES]),  # the same on 8-channel stages
        fwd("direct", 3, 12, 0, 20, 12, 20, tile=t4, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),     # 32 couts per tile
        # odd maps: 7x9 and 9x7
        fwd("direct", 3, 8, 0, 132, 7, 9, tile=t3, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),       # 4x8 px, 2 images; 3 cout tiles
        fwd("direct", 2, 16, 0, 64, 9, 7, tile=t2, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),       # 8x4 px, 4 images
        fwd("direct", 5, 8, 0, 64, 9, 7, tile=t1, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),        # 8x4 px, 8 images
        # stride 1 / pad 0: the output is 2 smaller
        fwd("direct", 3, 8, 0, 40, 7, 9, tile=t3, pad=0, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),   # 5x7 out: 4x4 px, 4 images
        fwd("direct", 2, 16, 0, 64, 12, 20, tile=t2, pad=0, states=[COL, ROW, MANY_TILES]),           # 10x18 out
        # stride 2: pad 0, pad 1, pad 0 + end padding (DDPM's Downsample)
        fwd("direct", 3, 8, 0, 64, 7, 9, tile=t3, stride=2, pad=0, states=[ROW, IMGS_TAIL, MANY_TILES]),           # 3x4 out: 2x4 px, 8 images
        fwd("direct", 2, 16, 0, 40, 12, 20, tile=t2, stride=2, pad=0, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),   # 5x9 out
        fwd("direct", 3, 8, 0, 64, 9, 7, tile=t3, stride=2, pad=1, states=[ROW, IMGS_TAIL, MANY_TILES]),           # 5x4 out: 4x4 px, 4 images
        fwd("direct", 1, 32, 32, 72, 12, 20, tile=t3, stride=2, pad=1, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),  # 6x10 out: 4x8 px, 2 images
        fwd("direct", 3, 8, 0, 64, 7, 9, tile=t3, stride=2, pad=0, pad_end=1, states=[ROW, IMGS_TAIL, MANY_TILES]),   # 3x4 out (an odd map: no pixel of the end padding is read)
        fwd("direct", 2, 16, 0, 40, 12, 20, tile=t2, stride=2, pad=0, pad_end=1, states=[COL, ROW, IMGS_TAIL, MANY_TILES], drop=True),  # 6x10 out: the last row and column read the end padding
        fwd("direct", 5, 8, 0, 64, 12, 20, tile=t2, stride=2, pad=0, pad_end=1, states=[COL, ROW, IMGS_TAIL, MANY_TILES]),   # 4x8 px, 5 = 4 + 1 images
        # (at stride 2 the halo of 256 output pixels exceeds the staging plan: the 256-pixel tiles are exchanged for a smaller one)
        # the top-left crop of a pad 2 convolution (strided input gradients): 17x17 of 19x19, 7x9 of 9x11
        fwd("direct", 2, 8, 0, 24, 17, 17, tile=t3, pad=2, out_hw=(17, 17), states=[COL, ROW, MANY_TILES]),
        fwd("direct", 3, 8, 0, 64, 7, 9, tile=t2, pad=2, out_hw=(7, 9), states=[COL, ROW, IMGS_TAIL, MANY_TILES]),
        # a fused 1x1 source with its own concat, at output resolution
        fwd("direct", 3, 16, 0, 72, 7, 9, tile=t3, aux=(32, 8), states=[COL, ROW, IMGS_TAIL, MANY_TILES]),
        fwd("direct", 2, 8, 0, 64, 12, 20, tile=t2, stride=2, pad=0, pad_end=1, aux=(12, 0), states=[COL, ROW, IMGS_TAIL, MANY_TILES]),
        # cin >= 128 on a map of at most 4x8: the reduction is split over two workgroups (make_plan: ksplit), and not
        fwd("direct", 3, 128, 0, 64, 4, 8, tile=t3, states=[IMGS_TAIL]),
        fwd("direct", 3, 128, 0, 64, 4, 8, tile=t3, flags=L.CONVF_NO_KSPLIT, states=[IMGS_TAIL]),
        fwd("direct", 2, 96, 64, 40, 4, 4, tile=t3, states=[IMGS_TAIL]),                               # 4 images per tile, 2 there; a concat
    ]


def _small_rows():
    """conv_small.hip: 8x8 output pixels per workgroup, 128-channel chunks; 12x20 and 6x10 leave partial tiles on both axes"""
    return [fwd("small", 2, 8, 0, 1, 6, 10, states=[COL, ROW, MANY_TILES]), fwd("small", 1, 16, 0, 2, 12, 20, states=[COL, ROW, MANY_TILES]),
            fwd("small", 3, 24, 0, 3, 6, 10, states=[COL, ROW, MANY_TILES]), fwd("small", 2, 40, 0, 4, 12, 20, states=[COL, ROW, MANY_TILES]),
            fwd("small", 2, 96, 64, 4, 12, 20, states=[COL, ROW, MANY_TILES], drop=True),    # concat; 160 channels: a ragged second chunk
            fwd("small", 1, 128, 136, 3, 6, 10, states=[COL, ROW, MANY_TILES])]              # three chunks, the last of 8 channels


def _gemm_rows():
    """the 1x1 row of the table: a 1x1-only launch of at least 128 rows onto at least 96 channels; rows = n * h * w are no
    multiple of the 64 / 128-row tiles"""
    return [fwd("1x1", 3, 40, 0, 96, 7, 9), fwd("1x1", 1, 32, 32, 132, 12, 20), fwd("1x1", 5, 64, 0, 200, 6, 10, drop=True),
            # two more GEMM kernels, so that more than one runs with resid == dst (shapes of test_ops_gpu.py: GEMM1X1_CASES and the
            # wide-tile cases).  The persistent kernel: 2 x 2 tiles of 128 x 128 on 8 workgroups, two of which own two tiles each,
            # and it fetches a unit's residual rows while it still stores the unit before; the 128 x 256 tile: 192 = 128 + 64 rows
            fwd("1x1", 1, 32, 24, 200, 16, 16, flags=L.CONVF_BF16X6 | L.CONVF_GEMM_PIPE),
            fwd("1x1", 3, 40, 0, 256, 8, 8, flags=L.CONVF_BF16X6 | L.CONVF_X6_WIDE)]


FWD_CASES = _wino_rows("f2") + _wino_rows("f4") + _wino_rows("f4r") + _f4p_rows() + _direct_rows() + _small_rows() + _gemm_rows()
assert len(set(FWD_CASES)) == len(FWD_CASES)
FORMS = ("plain", "fused-resid-before-scale", "fused-resid-after-scale", "accumulate-in-place")
INPLACE, INPLACE_SCALE = FORMS[3], 0.7

# Shapes just outside a route's limits: (row, a word of the message beyond the route's name).  The plan query refuses them; nothing
# is launched.  (small has no refusal of its own: what it does not want goes to the direct kernel -- check_small_edges.)
REFUSALS = [
    (fwd("f2", 1, 8, 0, 64, 6, 8), "8x8"), (fwd("f2", 1, 8, 0, 64, 8, 9), "even"), (fwd("f2", 1, 12, 8, 64, 8, 8), "boundary"),
    (fwd("f4", 1, 8, 0, 64, 10, 12), "multiples of 4"), (fwd("f4", 1, 8, 0, 64, 4, 8), "at least 8x8"), (fwd("f4", 1, 6, 0, 64, 8, 8), "multiples of 4"),
    (fwd("f4r", 1, 8, 0, 64, 12, 10), "multiples of 4"), (fwd("f4r", 1, 12, 0, 64, 8, 8), "multiple of 8"), (fwd("f4r", 1, 8, 0, 64, 8, 4), "at least 8x8"),
    (fwd("f4p", 1, 40, 0, 64, 4, 4), "multiple of 32"), (fwd("f4p", 1, 32, 0, 6, 4, 4), "multiple of 4"), (fwd("f4p", 1, 32, 0, 64, 6, 8), "multiples of 4"),
    (fwd("direct", 1, 16, 8, 64, 8, 8, tile=L.TILE_64x64), "boundary"), (fwd("direct", 1, 8, 0, 64, 8, 8, tile=L.TILE_64x64, stride=3), "stride"),
    (fwd("direct", 1, 8, 0, 64, 7, 9, tile=L.TILE_64x64, stride=2, pad=0, out_hw=(4, 4)), "larger"),
    (fwd("f4", 1, 8, 0, 64, 8, 8, pad_end=1), "pad_end 1 with Winograd tile 6"),      # (refused in front of the route's plan)
]


def check_table_states():
    """every row hits the tiling states it is listed for (restated plans), every explicit direct tile is the one that runs, and the
    table as a whole gives every route every state its tiling has"""
    seen = {}
    for c in FWD_CASES:
        ho, wo = out_size(c)
        if c.route in ("f2", "f4", "f4r"):
            tw, th, imgs = wino_tiling(c.route, c.n, ho, wo)
        elif c.route == "direct":
            tile, tw, th, imgs = direct_tiling(c.tile, ho, wo, c.stride)
            assert tile == c.tile, (fwd_id(c), "the halo rule exchanges this tile for", tile)
        elif c.route == "small":
            tw, th, imgs = 8, 8, 1
        else:
            continue
        assert _states(c.n, ho, wo, tw, th, imgs) == set(c.states), (fwd_id(c), sorted(_states(c.n, ho, wo, tw, th, imgs)), (tw, th, imgs))
        seen.setdefault(c.route, set()).update(c.states)
    for route in ("f2", "f4", "f4r", "direct"):
        assert seen[route] >= {COL, ROW, IMGS_TAIL, MANY_TILES}, (route, seen[route])
    assert seen["small"] >= {COL, ROW}
    for c in FWD_CASES:
        if c.route == "f4p":
            assert (c.n * (c.h // 4) * (c.w // 4)) % 64 != 0        # a partial block of GEMM rows
        if c.route == "1x1":
            # (the rows that force a GEMM kernel take their shapes from test_ops_gpu.py, whole 64-row tiles among them)
            assert ((c.n * c.h * c.w) % 64 != 0 or c.flags & GEMM_FORCED) and c.n * c.h * c.w >= 128 and c.cout >= 96
    for tile in DIRECT_TILES:
        assert any(c.route == "direct" and c.tile == tile for c in FWD_CASES)
    for form, cases in (("wgrad direct", [c for c in WGRAD_CASES if c.runs == "direct"]),):
        st = set()
        for c in cases:
            ho, wo = wg_out_size(c)
            st |= _states(c.n, ho, wo, *wgrad_direct_tiling(ho, wo, c.stride))
            assert _states(c.n, ho, wo, *wgrad_direct_tiling(ho, wo, c.stride)) >= set(c.states), (wg_id(c), c.states)
        assert st >= {COL, ROW, IMGS_TAIL, MANY_TILES}, (form, st)


# ------------------------------------------------------------------------------------------------ forward: inputs and references
def _seed(c):
    return zlib.crc32(repr(tuple(c)).encode())


def _groups(c):
    return 32 if c % 128 == 0 else c // 4


def _keep(shape, salt):
    """the mask the kernels regenerate: the hash of the element's index in the NHWC (concat) tensor"""
    thresh = min(int(round(DROP_P * 2.0 ** 32)), 2 ** 32 - 1)
    keep = T.hash_keep(np.arange(int(np.prod(shape)), dtype=np.uint64), (SEED_WORD ^ salt) & 0xFFFFFFFF, thresh, 1.0 / (1.0 - DROP_P))
    keep = torch.from_numpy(keep).reshape(shape)
    assert 0.6 < float((keep > 0).float().mean()) < 0.9
    return keep


def _gn64(x, G):
    """fp64 (mean, rstd) [n, G] of an NHWC tensor"""
    n, c = x.shape[0], x.shape[-1]
    xg = x.double().reshape(n, -1, G, c // G).permute(0, 2, 1, 3).reshape(n, G, -1)
    return xg.mean(-1), 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + EPS)


def _pro64(x, mode, G, gamma, beta, keep):
    """the fp64 prologue of an NHWC source: GroupNorm (fp64 statistics) / SiLU, then the dropout mask"""
    y = x.double()
    if mode in (L.PRO_GN, L.PRO_GN_SILU):
        mean, rstd = _gn64(x, G)
        cpg = x.shape[-1] // G
        y = (y - mean.repeat_interleave(cpg, 1)[:, None, None, :]) * rstd.repeat_interleave(cpg, 1)[:, None, None, :]
        y = y * gamma.double() + beta.double()
    if mode in (L.PRO_GN_SILU, L.PRO_SILU):
        y = F.silu(y)
    return y * keep.double() if keep is not None else y


def _source(g, n, h, w, c):
    """off centre, channels of different levels: a dropped mean or a wrong group shows"""
    return dict(x=torch.randn(n, h, w, c, generator=g) * 1.5 + 0.3 + torch.randn(1, 1, 1, c, generator=g), gamma=torch.randn(c, generator=g),
                beta=0.5 * torch.randn(c, generator=g), G=_groups(c))


@functools.lru_cache(maxsize=None)
def fwd_inputs(c):
    """the tensors of a row and its fp64 references, made once and shared by its forms and by both suites (nothing writes to them)"""
    g = torch.Generator().manual_seed(_seed(c))
    ho, wo = out_size(c)
    k = dict(ho=ho, wo=wo)
    if c.route != "1x1":
        cin = c.c0 + c.c1
        k["main"] = _source(g, c.n, c.h, c.w, cin)
        k["w"] = torch.randn(c.cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
        k["main"]["keep"] = _keep((c.n, c.h, c.w, cin), SALT) if c.drop else None
    aux = (c.c0, c.c1) if c.route == "1x1" else c.aux
    if aux:
        ca = aux[0] + aux[1]
        k["aux"] = _source(g, c.n, ho, wo, ca)
        k["wa"] = torch.randn(c.cout, ca, generator=g) / math.sqrt(ca)
        k["aux"]["keep"] = _keep((c.n, ho, wo, ca), SALT + 1) if c.drop and c.route == "1x1" else None
    k["bias"], k["chan_add"] = torch.randn(c.cout, generator=g), torch.randn(c.n, c.cout, generator=g)
    k["resid"] = torch.randn(c.n, ho, wo, c.cout, generator=g)
    k["ref"] = {}
    return k


def _modes(c, form):
    """(prologue of main, prologue of aux, dropout armed) of a form: the fused forms put GroupNorm + SiLU on the (concatenated)
    k x k source -- on the 1x1 source of a 1x1-only launch -- and SiLU on the 1x1 source beside a k x k one"""
    if form in ("plain", INPLACE):
        return L.PRO_NONE, L.PRO_NONE, False
    if c.route == "1x1":
        return L.PRO_NONE, L.PRO_GN_SILU, c.drop
    return L.PRO_GN_SILU, L.PRO_SILU, c.drop


def fwd_ref(c, form):
    k = fwd_inputs(c)
    if form not in k["ref"]:
        pm, pa, drop = _modes(c, form)
        y = torch.zeros(c.n, k["ho"], k["wo"], c.cout, dtype=torch.float64)
        if "main" in k:
            s = k["main"]
            t = _pro64(s["x"], pm, s["G"], s["gamma"], s["beta"], s["keep"] if drop else None).permute(0, 3, 1, 2)
            if c.pad_end:
                t = F.pad(t, (0, c.pad_end, 0, c.pad_end))
            y = y + F.conv2d(t, k["w"].double(), stride=c.stride, padding=c.pad)[:, :, :k["ho"], :k["wo"]].permute(0, 2, 3, 1)
        if "aux" in k:
            s = k["aux"]
            y = y + _pro64(s["x"], pa, s["G"], s["gamma"], s["beta"], s["keep"] if drop else None) @ k["wa"].double().t()
        if form == INPLACE:
            y = INPLACE_SCALE * y + k["resid"].double()
        else:
            y = y + k["bias"].double()
        if form not in ("plain", INPLACE):
            y = y + k["chan_add"].double()[:, None, None, :]
            r, sc = k["resid"].double(), 1.0 / math.sqrt(2.0)
            y = (y + r) * sc if form == FORMS[1] else y * sc + r
        k["ref"][form] = y
    return k["ref"][form]


# ------------------------------------------------------------------------------------------------ forward: arguments, plan, launch
def _fill(ops, s, dev, src, c0, c1, mode, drop, salt, keep):
    """an ssde_src over the channel split (c0, c1) of a source; the statistics are the fp32 rounding of the fp64 ones"""
    x0 = src["x"][..., :c0].contiguous().to(dev)
    x1 = src["x"][..., c0:].contiguous().to(dev) if c1 else None
    gn = None
    if mode in (L.PRO_GN, L.PRO_GN_SILU):
        mean, rstd = _gn64(src["x"], src["G"])
        gn = (mean.float().to(dev), rstd.float().to(dev), src["gamma"].to(dev), src["beta"].to(dev), src["G"])
    ops._fill_src(s, x0, x1, mode, gn)
    keep += [x0, x1, gn]
    if drop:
        seed = torch.tensor([SEED_WORD], dtype=torch.int32).to(dev)
        ops.set_dropout(s, DROP_P, seed, salt)
        keep.append(seed)


def fwd_args(c, form, dev=None):
    """the ssde_conv_args of a row in a form.  dev None: the shape only, every pointer a dummy -- all a plan query reads.
    Returns (args, dst, whatever must stay alive)."""
    from score_sde_pytorch_amd.engine import conv3_route_of_tile, pack_matrix, wino4_v_floats
    ho, wo = out_size(c)
    pm, pa, drop = _modes(c, form)
    a, keep, dst = L.ConvArgs(), [], None
    dummy = 0x1000
    aux = (c.c0, c.c1) if c.route == "1x1" else c.aux
    if dev is None:
        for s, cc, on, mode in ((a.main, (c.c0, c.c1), c.route != "1x1", pm), (a.aux, aux, bool(aux), pa)):
            if on:
                s.p0, s.c0, s.p1, s.c1, s.pro_mode = dummy, cc[0], (dummy if cc[1] else None), cc[1], mode
                if mode in (L.PRO_GN, L.PRO_GN_SILU):
                    s.gn_groups, s.gn_mean, s.gn_rstd, s.gn_gamma, s.gn_beta = _groups(cc[0] + cc[1]), dummy, dummy, dummy, dummy
        a.w_main, a.w_aux, a.dst = (dummy if c.route != "1x1" else None), (dummy if aux else None), dummy
        if form == INPLACE:
            a.resid = a.dst
    else:
        ops, _ = _ops()
        k = fwd_inputs(c)
        if c.route != "1x1":
            _fill(ops, a.main, dev, k["main"], c.c0, c.c1, pm, drop, SALT, keep)
            wp = conv3_route_of_tile(c.tile).pack(k["w"].to(dev))
            a.w_main = wp.data_ptr()
            keep.append(wp)
        if aux:
            _fill(ops, a.aux, dev, k["aux"], aux[0], aux[1], pa, drop and c.route == "1x1", SALT + 1, keep)
            wa = pack_matrix(k["wa"].to(dev))
            a.w_aux = wa.data_ptr()
            keep.append(wa)
        if form == INPLACE:
            dst = k["resid"].clone().to(dev)
            a.dst = a.resid = dst.data_ptr()
        else:
            dst = torch.full((c.n, ho, wo, c.cout), float("nan")).to(dev)
            a.dst = dst.data_ptr()
            b = k["bias"].to(dev)
            a.bias = b.data_ptr()
            keep.append(b)
        if form not in ("plain", INPLACE):
            ca, r = k["chan_add"].to(dev), k["resid"].to(dev)
            a.chan_add, a.chan_add_ld, a.resid = ca.data_ptr(), c.cout, r.data_ptr()
            keep += [ca, r]
        if c.tile == L.TILE_WINOGRAD4R:
            v = torch.full((wino4_v_floats(c.n, c.h, c.w, c.c0 + c.c1),), float("nan")).to(dev)
            a.wino_v = v.data_ptr()
            keep.append(v)
    if c.route != "1x1":
        a.ksize, a.stride, a.pad, a.pad_end, a.h_in, a.w_in = 3, c.stride, c.pad, c.pad_end, c.h, c.w
    else:
        a.ksize, a.stride, a.pad = 0, 1, 0
    a.n, a.h_out, a.w_out, a.c_out, a.tile = c.n, ho, wo, c.cout, c.tile
    a.flags = L.conv_route_flags() | c.flags                    # (the matrix mode of the run: SSDE_MATRIX)
    if form == INPLACE:
        a.out_scale, a.resid_post = INPLACE_SCALE, 1
    elif form != "plain":
        a.out_scale, a.resid_post = 1.0 / math.sqrt(2.0), int(form == FORMS[2])
    else:
        a.out_scale = 1.0
    return a, dst, keep


def fwd_plan(c, form="plain"):
    """the plan query on the shape alone: the LDS bytes of the launch; raises SsdeError with the library's message on a refusal"""
    with _Env(row_env(c)):
        return _fwd_plan(c, form)


def _fwd_plan(c, form):
    _, lib = _ops()
    a, _, _ = fwd_args(c, form)
    rc = lib.ssde_conv_lds_bytes(C.byref(a))
    if rc < 0:
        raise L.SsdeError(lib.ssde_last_error().decode())
    if c.route == "1x1" and c.flags & GEMM_FORCED:
        # a forced GEMM kernel is not refused where it cannot run (gemm_plan's pipe_ok / wide_ok): the launch would get the kernel
        # it gets anyway.  The three kernels ask for different amounts of LDS, so the plan tells whether the forced one runs
        a.flags &= ~GEMM_FORCED
        assert lib.ssde_conv_lds_bytes(C.byref(a)) != rc, (fwd_id(c), form, "the forced GEMM kernel does not take this launch", rc)
    # the two routes that are taken by shape rather than by tile do not refuse what they do not want: the direct kernel runs it.
    # A row listed for them must be theirs (ssde_conv1x1_wants restated; the small-cout kernel's plan is not the direct one's)
    if c.route == "1x1" and not (c.cout >= 96 and c.n * c.h * c.w >= 128):
        raise L.SsdeError("conv(1x1 GEMM): not wanted, the direct kernel takes this launch")
    if c.route == "small":
        a.flags |= L.CONVF_NO_SMALL_COUT
        if lib.ssde_conv_lds_bytes(C.byref(a)) == rc:
            raise L.SsdeError("conv(small cout): not wanted, the direct kernel takes this launch")
    return rc


def check_forward(dev, c, form):
    """one launch of a row in one form: planned, launched into NaN, compared with fp64; GroupNorm partials where the tiling
    writes them, finalized and compared with the fp64 statistics of the fp64 reference output.  Returns the error.
    The form "accumulate-in-place" is the launch the backward lowering issues for every input gradient (TrainEngine._bwd_branch):
    dst preloaded with a base (the row's `resid` tensor), resid == dst, resid_post = 1, out_scale = 0.7 (neither 1 nor 1/sqrt(2):
    (base + conv) s, conv s + base and the fused forms all differ), no bias, no per-image addend, no partials; the reference is
    fp64 0.7 conv + base.  Every kernel reads the residual it is about to overwrite, and the split reductions hand partial sums
    over between workgroups through dst itself: the rows `direct ... 128+0-64-4x8 t3`, `f4 ... 128+0-64-8x12`,
    `f4r ... 128+128-64-8x12` and the f4p ks2 / ks4 rows, where the alias changes the plan (make_plan of conv_mfma.hip and
    ssde_conv_wino4r_launch drop the split for resid == dst), are the point of the form.  Both plan queries are made on
    arguments that carry the alias."""
    with _Env(row_env(c)):
        return _check_forward(dev, c, form)


def _check_forward(dev, c, form):
    ops, lib = _ops()
    assert fwd_plan(c, form) > 0                                # (raises with the message: a listed case must be accepted)
    a, dst, keep = fwd_args(c, form, dev)
    lds = lib.ssde_conv_lds_bytes(C.byref(a))
    assert lds > 0, (fwd_id(c), form, lib.ssde_last_error())
    if c.tile == L.TILE_WINOGRAD4P:
        need = int(lib.ssde_conv_ws_floats(C.byref(a)))
        assert need > 0, (fwd_id(c), lib.ssde_last_error())
        ws = torch.full((need,), float("nan")).to(dev)
        a.wino_ws, a.wino_ws_floats = ws.data_ptr(), need
    sl = lib.ssde_conv_gn_slices(C.byref(a)) if form != INPLACE else 0          # (the backward lowering asks for no partials)
    part = None
    if sl > 0:
        part = torch.full((c.n, sl, c.cout // 4, 3), float("nan")).to(dev)
        a.gn_part = part.data_ptr()
    L.check(lib.ssde_conv2d(C.byref(a), ops._stream()), "ssde_conv2d")
    ref = fwd_ref(c, form)
    got = dst.cpu()
    assert bool(torch.isfinite(got).all()), (fwd_id(c), form, "part of dst was not written")
    err = rel_err(got, ref)
    line = "conv %s %s vs fp64: %.3g" % (fwd_id(c), form, err)
    stats = None
    if part is not None:
        Go = c.cout // 4                                        # groups of one channel quad: every entry of the partials on its own
        f = L.GnFinalizeArgs()
        m2, r2 = torch.zeros(c.n, Go).to(dev), torch.zeros(c.n, Go).to(dev)
        f.part0, f.c0, f.slices0, f.n, f.groups, f.eps = part.data_ptr(), c.cout, sl, c.n, Go, EPS
        f.mean, f.rstd = m2.data_ptr(), r2.data_ptr()
        L.check(lib.ssde_gn_finalize(C.byref(f), ops._stream()), "ssde_gn_finalize")
        mr, rr = _gn64(ref, Go)
        stats = ((m2.cpu().double() - mr).abs().max().item() / max(1.0, mr.abs().max().item()), ((r2.cpu().double() - rr).abs() / rr).max().item())
        line += "; partials in %d slices: mean %.3g, rstd %.3g" % (sl, stats[0], stats[1])
    print(line)
    assert err < TOL_OP, (fwd_id(c), form, err)
    if stats is not None:
        assert stats[0] < TOL_MEAN and stats[1] < TOL_RSTD, (fwd_id(c), form, stats)
    # a second launch on the same arguments into fresh NaN: a split reduction left its hand-over slots ready, and every route
    # sums in a fixed order -- the same bits (but where f4 / f4r hand a reduction over between workgroups in arrival order)
    if form == INPLACE:
        dst.copy_(fwd_inputs(c)["resid"])                        # (from the restored base)
    else:
        dst.fill_(float("nan"))
    if part is not None:
        first_part = part.clone()
        part.fill_(float("nan"))
    L.check(lib.ssde_conv2d(C.byref(a), ops._stream()), "ssde_conv2d")
    again = dst.cpu()
    if c.route in ("f4", "f4r") and c.c0 + c.c1 >= 128 and not c.flags & L.CONVF_NO_KSPLIT:
        assert rel_err(again, ref) < TOL_OP, (fwd_id(c), form, "second launch", rel_err(again, ref))
    else:
        assert torch.equal(again, got), (fwd_id(c), form, "a second launch gives other bits")
        assert part is None or torch.equal(part, first_part), (fwd_id(c), form, "a second launch gives other partials")
    return err


def check_forward_case(dev, c):
    """a row plain, then fully fused with the residual before and after the scale, then as the in-place accumulation of an
    input gradient"""
    return max(check_forward(dev, c, form) for form in FORMS)


def check_refusal(c, word):
    """the plan query refuses the shape, names the route and the limit; nothing is launched"""
    try:
        fwd_plan(c)
    except L.SsdeError as e:
        msg = str(e)
        assert (ROUTE_IN_MESSAGE[c.route] in msg or "Winograd tile %d" % c.tile in msg) and word in msg, (fwd_id(c), msg)
        return msg
    raise AssertionError("%s: the plan accepts a shape outside the route's limits" % fwd_id(c))


def check_small_edges():
    """what conv_small.hip does not want is not refused but runs on the direct kernel: one channel more, a channel count that is
    no multiple of 8, a stride -- the plan of each is the direct kernel's (that of the same launch with SSDE_CONVF_NO_SMALL_COUT)"""
    assert fwd_plan(fwd("small", 1, 8, 0, 4, 6, 10)) > 0
    for c in (fwd("small", 1, 8, 0, 5, 6, 10), fwd("small", 1, 12, 0, 4, 6, 10), fwd("small", 1, 8, 0, 4, 6, 10, stride=2)):
        try:
            fwd_plan(c)
        except L.SsdeError as e:
            assert "direct kernel takes" in str(e), (fwd_id(c), str(e))
        else:
            raise AssertionError("%s: conv_small.hip's plan for a launch outside its limits" % fwd_id(c))


# ------------------------------------------------------------------------------------------------ weight gradient: the case table
Wg = namedtuple("Wg", "form runs n h w c0 c1 cout pro drop splits more stride pad pad_end g_ld g_off cin_store states")
WG_FLAGS = {"auto": 0, "direct": L.WGRADF_DIRECT, "f2": L.WGRADF_F2, "f4": L.WGRADF_F4_FORCE}
PRO_NAMES = {L.PRO_NONE: "none", L.PRO_GN: "gn", L.PRO_GN_SILU: "gnsilu", L.PRO_SILU: "silu"}
F2_SLAB, DIRECT_SLAB = 16 * 64 * 64, 9 * 64 * 64          # floats per (co, ci) tile of one split: wgrad_wino.hip kSlab, wgrad.hip


def wg(form, runs, n, h, w, c0, c1, cout, pro=L.PRO_NONE, drop=False, splits=0, more=0, stride=1, pad=1, pad_end=0, g_ld=None, g_off=0,
       cin_store=None, states=()):
    return Wg(form, runs, n, h, w, c0, c1, cout, pro, drop, splits, more, stride, pad, pad_end, cout if g_ld is None else g_ld, g_off,
              c0 + c1 if cin_store is None else cin_store, tuple(states))


def wg_id(c):
    s = "%s-runs-%s-n%d-%dx%d-%d+%d-%d-%s" % (c.form, c.runs, c.n, c.h, c.w, c.c0, c.c1, c.cout, PRO_NAMES[c.pro])
    if (c.stride, c.pad, c.pad_end) != (1, 1, 0):
        s += "-s%dp%de%d" % (c.stride, c.pad, c.pad_end)
    s += "-splits%d" % c.splits if c.splits else ""
    s += "-nostreamk" if c.more & L.WGRADF_NO_STREAMK else ""
    s += "-xvec1" if c.more & L.WGRADF_XVEC1 else ""
    s += "-launchorder" if c.more & L.WGRADF_NO_XCD_ORDER else ""
    s += "-g%d@%d" % (c.g_ld, c.g_off) if c.g_ld != c.cout else ""
    s += "-store%d" % c.cin_store if c.cin_store != c.c0 + c.c1 else ""
    return s + ("-drop" if c.drop else "")


def wg_out_size(c):
    return ((c.h + 2 * c.pad + c.pad_end - 3) // c.stride + 1, (c.w + 2 * c.pad + c.pad_end - 3) // c.stride + 1)


def _wgrad_rows():
    N, GN, GS, SI = L.PRO_NONE, L.PRO_GN, L.PRO_GN_SILU, L.PRO_SILU
    rows = []
    # ---- F(4x4,3x3), wgrad_wino4.hip (ssde_wgrad_wino4_wants: 3x3 / stride 1 / pad 1, maps % 4 and >= 8, channels % 32, every
    # input channel stored).  No tile grid: the GEMMs reduce over T = n * h/4 * w/4 tiles in stages of 16 -- T = 6, 18, 45, 60
    # leave a ragged last stage; an explicit split cuts T into ranges of whole stages (T = 45: 32 + 13 and 16 + 16 + 13)
    rows += [wg("f4", "f4", 1, 12, 8, 32, 0, 32), wg("f4", "f4", 3, 20, 12, 32, 32, 64, GS), wg("f4", "f4", 3, 20, 12, 32, 32, 64, GS, splits=2),
             wg("f4", "f4", 3, 20, 12, 32, 32, 64, GS, splits=3), wg("f4", "f4", 5, 8, 24, 64, 0, 96, SI, more=L.WGRADF_NO_STREAMK),
             wg("f4", "f4", 3, 20, 12, 32, 32, 64, GN, more=L.WGRADF_NO_STREAMK), wg("f4", "f4", 3, 12, 8, 32, 32, 32, N),
             wg("f4", "f4", 3, 12, 8, 32, 32, 32, GN), wg("f4", "f4", 3, 12, 8, 32, 32, 32, SI), wg("f4", "f4", 3, 12, 8, 64, 0, 32, GS, drop=True),
             wg("f4", "f4", 1, 8, 24, 32, 0, 32, g_ld=48, g_off=8),
             # the transforms with one channel per thread; the GEMM's workgroups in launch order
             wg("f4", "f4", 3, 20, 12, 32, 32, 64, GS, more=L.WGRADF_XVEC1), wg("f4", "f4", 3, 20, 12, 32, 32, 64, GS, more=L.WGRADF_NO_XCD_ORDER),
             # not legal there: F4_FORCE falls to F(2x2,3x3) on a 4x8 map, to the direct kernel with fewer channels stored
             wg("f4", "f2", 3, 4, 8, 64, 0, 64, GS), wg("f4", "direct", 1, 12, 8, 32, 0, 32, cin_store=30, states=[ROW, MANY_TILES])]
    # ---- F(2x2,3x3), wgrad_wino.hip (ssde_wgrad_wino_wants: 3x3 / stride 1 / pad 1, h % 4, w % 8, channels and the concat
    # boundary % 64, every input channel stored).  Chunks of 4x8 pixels tile such a map exactly; the splits cut n * h/4 * w/8 chunks
    rows += [wg("f2", "f2", 1, 4, 8, 64, 0, 64), wg("f2", "f2", 3, 12, 8, 64, 64, 64, GS), wg("f2", "f2", 3, 12, 8, 64, 64, 64, GS, splits=2),
             wg("f2", "f2", 3, 12, 8, 64, 64, 64, GS, splits=3), wg("f2", "f2", 5, 8, 24, 64, 0, 128, SI), wg("f2", "f2", 3, 4, 8, 64, 64, 64, N),
             wg("f2", "f2", 3, 4, 8, 64, 64, 64, GN), wg("f2", "f2", 3, 4, 8, 64, 64, 64, SI), wg("f2", "f2", 3, 12, 8, 64, 0, 64, GS, drop=True),
             wg("f2", "f2", 1, 8, 24, 64, 0, 64, g_ld=80, g_off=8),
             # not legal there: a width that is no multiple of 8
             wg("f2", "direct", 3, 20, 12, 64, 0, 64, GS, states=[COL, ROW, MANY_TILES])]
    # ---- the library's own choice: F(4x4,3x3) does not pay below 512 tiles, F(2x2,3x3) wherever it is legal, else the direct kernel
    rows += [wg("auto", "f2", 3, 8, 24, 64, 0, 64, GS), wg("auto", "f2", 1, 12, 8, 64, 0, 64, N, splits=3),
             wg("auto", "f2", 5, 4, 8, 64, 64, 128, SI, splits=2), wg("auto", "direct", 3, 20, 12, 32, 0, 32, GS, states=[COL, ROW, MANY_TILES]),
             wg("auto", "direct", 5, 4, 8, 8, 12, 40, GS, splits=2, states=[IMGS_TAIL])]
    # ---- the direct kernel, wgrad.hip: chunks of 64 / 128 output pixels (32 at stride 2), tiled like the forward kernel
    rows += [wg("direct", "direct", 3, 4, 8, 64, 0, 64, states=[IMGS_TAIL]),                                        # 4x8 px, 2 images, 3 = 2 + 1
             wg("direct", "direct", 1, 12, 8, 16, 16, 40, GS, states=[ROW, MANY_TILES]),                           # 8x8 px
             wg("direct", "direct", 5, 8, 24, 8, 0, 72, SI, splits=3, states=[COL, MANY_TILES]),                   # 8x16 px
             wg("direct", "direct", 3, 20, 12, 8, 12, 24, GN, splits=2, states=[COL, ROW, MANY_TILES]),            # 16x8 px
             wg("direct", "direct", 3, 20, 12, 8, 12, 24, N, states=[COL, ROW, MANY_TILES]),
             wg("direct", "direct", 3, 12, 8, 32, 8, 24, GS, drop=True, states=[ROW, MANY_TILES]),
             wg("direct", "direct", 1, 8, 24, 8, 0, 20, g_ld=48, g_off=8, states=[COL, MANY_TILES]),
             wg("direct", "direct", 3, 4, 8, 4, 0, 24, cin_store=3, states=[IMGS_TAIL]),
             # strides and paddings, odd maps
             wg("direct", "direct", 3, 7, 9, 8, 0, 40, stride=2, pad=0, states=[ROW, IMGS_TAIL, MANY_TILES]),                   # 3x4 out: 2x4 px, 4 images
             wg("direct", "direct", 3, 7, 9, 8, 0, 40, GS, stride=2, pad=0, pad_end=1, states=[ROW, IMGS_TAIL, MANY_TILES]),        # 3x4 out (odd map: the end padding is not read)
             wg("direct", "direct", 2, 12, 20, 16, 0, 24, SI, stride=2, pad=0, states=[COL, ROW, MANY_TILES]),                  # 5x9 out: 4x8 px
             wg("direct", "direct", 2, 12, 20, 8, 8, 24, GS, splits=3, stride=2, pad=0, pad_end=1, states=[COL, ROW, MANY_TILES]),   # 6x10 out
             wg("direct", "direct", 3, 7, 9, 8, 0, 40, GN, pad=0, states=[COL, ROW, IMGS_TAIL, MANY_TILES])]                    # 5x7 out: 4x4 px, 4 images
    return rows


WGRAD_CASES = _wgrad_rows()
assert len(set(WGRAD_CASES)) == len(WGRAD_CASES)


@functools.lru_cache(maxsize=None)
def wg_inputs(c):
    """the tensors of a row and its fp64 reference gradient (fp64 autograd through F.conv2d of the fp64 prologue), made once"""
    g = torch.Generator().manual_seed(_seed(c))
    ho, wo = wg_out_size(c)
    cin = c.c0 + c.c1
    src = _source(g, c.n, c.h, c.w, cin)
    src["keep"] = _keep((c.n, c.h, c.w, cin), SALT) if c.drop else None
    gy = 100.0 + 50.0 * torch.randn(c.n, ho, wo, c.g_ld, generator=g)    # the columns around the slice: large, so that a leak shows
    gy[..., c.g_off:c.g_off + c.cout] = torch.randn(c.n, ho, wo, c.cout, generator=g) + 0.25
    wt = torch.zeros(c.cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    t = _pro64(src["x"], c.pro, src["G"], src["gamma"], src["beta"], src["keep"]).permute(0, 3, 1, 2)
    if c.pad_end:
        t = F.pad(t, (0, c.pad_end, 0, c.pad_end))
    y = F.conv2d(t, wt, stride=c.stride, padding=c.pad)
    assert tuple(y.shape[2:]) == (ho, wo)
    y.backward(gy[..., c.g_off:c.g_off + c.cout].double().permute(0, 3, 1, 2))
    return dict(src=src, gy=gy, ref=wt.grad[:, :c.cin_store].contiguous())


def wg_shape_args(c):
    ho, wo = wg_out_size(c)
    return L.wgrad_shape_args(dict(c0=c.c0, c1=c.c1, pro_mode=c.pro, gn_groups=_groups(c.c0 + c.c1) if c.pro in (L.PRO_GN, L.PRO_GN_SILU) else 0),
                              WG_FLAGS[c.form] | c.more, g_ld=c.g_ld, g_off=c.g_off, n=c.n, h_in=c.h, w_in=c.w, h_out=ho, w_out=wo, c_out=c.cout,
                              ksize=3, stride=c.stride, pad=c.pad, pad_end=c.pad_end, cin_store=c.cin_store, transpose_out=0)


def wg_plan(c):
    """(route the library plans -- 'f4' / 'f2' / 'direct' --, scratch floats of its preferred split); raises SsdeError on a refusal.
    F(4x4,3x3) answers ssde_wgrad_wants_winograd4; the other two are told apart by the scratch their plans ask for: F(2x2,3x3)
    slabs of 16 x 64 x 64 floats per 64 x 64 tile of dw for at least one split, the direct kernel slabs of 9 x 64 x 64 and none
    for a single split."""
    _, lib = _ops()
    a = wg_shape_args(c)
    scratch = int(lib.ssde_wgrad_scratch_floats(C.byref(a)))
    if scratch < 0:
        raise L.SsdeError(lib.ssde_last_error().decode())
    ho, wo = wg_out_size(c)
    cin = c.c0 + c.c1
    if lib.ssde_wgrad_wants_winograd4(C.byref(a)):
        tiles = c.n * (ho // 4) * (wo // 4)
        fixed, split = 36 * tiles * (cin + c.cout), 36 * c.cout * cin
        assert scratch >= fixed + split and (scratch - fixed) % split == 0, (wg_id(c), scratch, fixed, split)
        return "f4", scratch
    ntiles = cdiv(c.cout, 64) * cdiv(c.cin_store, 64)
    # F(2x2,3x3), plan_params of wgrad_wino.hip: one round of at most 256 workgroups, at least 4 chunks each
    chunks = c.n * (wo // 8) * (ho // 4)
    s2 = max(1, min(256 // ntiles, chunks // 4 if chunks >= 4 else 1, chunks))
    s2 = cdiv(chunks, cdiv(chunks, s2)) if chunks else 1
    f2_floats = ntiles * F2_SLAB * s2
    # the direct kernel, chunked_plan_params of wgrad.hip: about 512 workgroups, at least 2 chunks each
    tw, th, imgs = wgrad_direct_tiling(ho, wo, c.stride)
    dchunks = cdiv(c.n, imgs) * cdiv(wo, tw) * cdiv(ho, th)
    sd = max(1, min(cdiv(512, ntiles), dchunks // 2 if dchunks >= 2 else 1))
    d_floats = ntiles * DIRECT_SLAB * sd if sd > 1 else 0
    legal_f2 = (c.stride, c.pad, c.pad_end) == (1, 1, 0) and c.h % 4 == 0 and c.w % 8 == 0 and c.cout % 64 == 0 and cin % 64 == 0 and \
        c.cin_store == cin and (c.c1 == 0 or c.c0 % 64 == 0)
    if legal_f2 and not a.flags & L.WGRADF_DIRECT:
        assert f2_floats != d_floats, (wg_id(c), "the scratch of this shape does not tell the two routes apart")
        if scratch == f2_floats:
            return "f2", scratch
    assert scratch == d_floats, (wg_id(c), scratch, f2_floats, d_floats)
    return "direct", scratch


def check_wgrad(dev, c):
    """one weight-gradient launch: the route asserted from the plan, launched onto zeros with scratch for the split it asks for,
    compared with fp64 autograd.  Returns the error."""
    ops, lib = _ops()
    route, need = wg_plan(c)
    assert route == c.runs, (wg_id(c), "the library plans", route)
    k = wg_inputs(c)
    a, keep = wg_shape_args(c), []
    _fill(ops, a.src, dev, k["src"], c.c0, c.c1, c.pro, c.drop, SALT, keep)
    gy = k["gy"].to(dev)
    dw = torch.zeros(c.cout, c.cin_store, 3, 3).to(dev)
    scale = 0.5
    ho, wo = wg_out_size(c)
    cin = c.c0 + c.c1
    if c.splits:                     # room for the explicit split on whichever route runs (a short scratch would cost splits silently)
        ntiles = cdiv(c.cout, 64) * cdiv(c.cin_store, 64)
        need = max(need, 36 * c.n * (ho // 4) * (wo // 4) * (cin + c.cout) + 36 * c.cout * cin * c.splits, ntiles * F2_SLAB * c.splits)
    scratch = torch.full((max(need, 1),), float("nan")).to(dev)
    a.g, a.splits, a.scale, a.dw, a.scratch, a.scratch_floats = gy.data_ptr(), c.splits, scale, dw.data_ptr(), scratch.data_ptr(), scratch.numel()
    L.check(lib.ssde_conv_wgrad(C.byref(a), ops._stream()), "ssde_conv_wgrad")
    err = rel_err(dw.cpu(), scale * k["ref"])
    print("wgrad %s vs fp64: %.3g" % (wg_id(c), err))
    assert err < TOL_OP, (wg_id(c), err)
    return err


# (forward route, n, c0, c1, cout, h, w, dropout): partial tile columns and rows, 2 to 8 images per workgroup, ragged batch tails
V_CASES = [("f4", 2, 32, 0, 32, 8, 12, False), ("f4", 3, 32, 32, 64, 20, 12, True), ("f4", 1, 32, 32, 96, 12, 20, False),
           ("f4r", 3, 32, 32, 64, 20, 12, True), ("f4r", 5, 64, 0, 32, 24, 8, False)]


def v_id(vc):
    return "%s-n%d-%d+%d-%d-%dx%d%s" % (vc[:7] + ("-drop" if vc[7] else "",))


def check_v_handover(dev, vc):
    """The transformed input a forward F(4x4,3x3) launch leaves behind (ssde_conv_args.wino_v: conv_wino4.hip's by-product of its
    first cout tile, wino4_xform.hip's output on the two-kernel route) is what the F(4x4,3x3) weight gradient of the layer
    multiplies with (ssde_wgrad_args.v_pre: its own transform pass is skipped).  On an irregular tiling, fused form, V
    prefilled with NaN: the forward output and the weight gradient computed from that V against fp64."""
    from score_sde_pytorch_amd.engine import wino4_v_floats
    ops, lib = _ops()
    route, n, c0, c1, cout, h, w, drop = vc
    c, form = fwd(route, n, c0, c1, cout, h, w, drop=drop), FORMS[1]
    assert _states(n, h, w, *wino_tiling(route, n, h, w)) & {COL, ROW}
    a, dst, keep = fwd_args(c, form, dev)
    v = torch.full((wino4_v_floats(n, h, w, c0 + c1),), float("nan")).to(dev)
    a.wino_v = v.data_ptr()
    assert lib.ssde_conv_lds_bytes(C.byref(a)) > 0, lib.ssde_last_error()
    L.check(lib.ssde_conv2d(C.byref(a), ops._stream()), "ssde_conv2d")
    err_y = rel_err(dst.cpu(), fwd_ref(c, form))
    assert bool(torch.isfinite(v).all()), (v_id(vc), "part of V was not written")
    s = fwd_inputs(c)["main"]
    g = torch.Generator().manual_seed(_seed(c) + 1)
    gy = torch.randn(n, h, w, cout, generator=g) + 0.25
    wt = torch.zeros(cout, c0 + c1, 3, 3, dtype=torch.float64, requires_grad=True)
    t = _pro64(s["x"], L.PRO_GN_SILU, s["G"], s["gamma"], s["beta"], s["keep"] if drop else None).permute(0, 3, 1, 2)
    F.conv2d(t, wt, padding=1).backward(gy.double().permute(0, 3, 1, 2))
    wa = L.wgrad_shape_args(dict(c0=c0, c1=c1, pro_mode=L.PRO_GN_SILU, gn_groups=s["G"]), L.WGRADF_F4_FORCE, g_ld=cout, g_off=0, n=n, h_in=h,
                            w_in=w, h_out=h, w_out=w, c_out=cout, ksize=3, stride=1, pad=1, pad_end=0, cin_store=c0 + c1, transpose_out=0)
    assert lib.ssde_wgrad_wants_winograd4(C.byref(wa)) == 1
    need = int(lib.ssde_wgrad_scratch_floats(C.byref(wa)))
    assert need > 0, lib.ssde_last_error()
    _fill(ops, wa.src, dev, s, c0, c1, L.PRO_GN_SILU, drop, SALT, keep)
    gyd, dw, scratch = gy.to(dev), torch.zeros(cout, c0 + c1, 3, 3).to(dev), torch.full((need,), float("nan")).to(dev)
    wa.g, wa.scale, wa.dw, wa.scratch, wa.scratch_floats, wa.v_pre = gyd.data_ptr(), 1.0, dw.data_ptr(), scratch.data_ptr(), need, v.data_ptr()
    L.check(lib.ssde_conv_wgrad(C.byref(wa), ops._stream()), "ssde_conv_wgrad")
    err_w = rel_err(dw.cpu(), wt.grad)
    print("V hand-over %s vs fp64: forward %.3g, weight gradient from the forward's V %.3g" % (v_id(vc), err_y, err_w))
    assert err_y < TOL_OP and err_w < TOL_OP, (v_id(vc), err_y, err_w)
    return max(err_y, err_w)


WG_REFUSALS = [(wg("direct", "direct", 1, 8, 8, 8, 0, 8, stride=3), "stride"), (wg("f4", "f4", 1, 8, 8, 32, 0, 32, cin_store=40), "cin_store"),
               (wg("f2", "f2", 1, 8, 8, 6, 0, 64), "multiples of 4"), (wg("direct", "direct", 1, 7, 9, 8, 0, 8, stride=2, pad=0, pad_end=2), "pad_end")]


def check_wgrad_refusal(c, word):
    try:
        wg_plan(c)
    except L.SsdeError as e:
        assert "wgrad" in str(e) and word in str(e), (wg_id(c), str(e))
        return str(e)
    raise AssertionError("%s: the plan accepts it" % wg_id(c))


# ------------------------------------------------------------------------------------------------ the seeded sweep (emulator)
SIDES = (4, 6, 7, 8, 9, 10, 12, 16, 20, 24)
SWEEP_FWD = ("f2", "f4", "f4r", "f4p", "small", "direct", "1x1")
SWEEP_WG = ("auto", "direct", "f2", "f4")
# the sides a route's kernel tiles: a draw takes a side from here, one draw in seven from all of SIDES (so that the limits of
# the plans are met from outside too, without most Winograd draws being refusals: two sides from SIDES are both multiples of 4 and
# at least 8 one time in four)
NATURAL = {"f2": (8, 10, 12, 16, 20, 24), "f4": (8, 12, 16, 20, 24), "f4r": (8, 12, 16, 20, 24), "f4p": (4, 8, 12, 16), "small": SIDES,
           "direct": SIDES, "1x1": (7, 8, 9, 10, 12, 16, 20, 24)}
SWEEP_DRAWS, SWEEP_FLOOR, SWEEP_REFUSED_MAX = 30, 20, 0.25


def _side(rng, natural):
    return rng.choice(SIDES if rng.random() < 1.0 / 7.0 else natural)


def draw_forward(rng, route):
    h, w = _side(rng, NATURAL[route]), _side(rng, NATURAL[route])
    n = rng.choice((1, 2, 3))
    ch = rng.choice((4, 8, 12, 16, 24, 32, 40)) if rng.random() < 0.12 else None           # now and then any small multiple of 4
    kw = {}
    if route == "f2":
        c0, c1 = rng.choice(((8, 0), (16, 0), (8, 8), (24, 8)))
    elif route in ("f4", "f4r"):
        c0, c1 = rng.choice(((8, 0), (16, 0), (8, 8), (24, 16)))
    elif route == "f4p":
        c0, c1 = rng.choice(((32, 0), (64, 0), (32, 32)))
        kw["flags"] = rng.choice((L.CONVF_NO_KSPLIT, L.CONVF_KSPLIT2, L.CONVF_KSPLIT4, 0))
    elif route == "small":
        c0, c1 = rng.choice(((8, 0), (16, 0), (32, 8), (128, 24)))
    elif route == "1x1":
        c0, c1 = rng.choice(((8, 0), (40, 0), (32, 16)))
        n = rng.choice((3, 4, 5))
    else:
        c0, c1 = rng.choice(((8, 0), (12, 0), (32, 8), (32, 32)))
        stride, pad, pad_end = rng.choice(((1, 1, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (2, 0, 1)))
        kw.update(tile=rng.choice(sorted(DIRECT_TILES)), stride=stride, pad=pad, pad_end=pad_end, flags=rng.choice((0, L.CONVF_BKC8, L.CONVF_NO_KSPLIT)))
        if rng.random() < 0.25:
            kw["aux"] = rng.choice(((8, 0), (32, 4)))
    if ch is not None:
        c0, c1 = ch, 0
    cout = rng.choice((1, 2, 3, 4)) if route == "small" else rng.choice((96, 100, 132)) if route == "1x1" else rng.choice((8, 40, 64, 72))
    return fwd(route, n, c0, c1, cout, h, w, drop=rng.random() < 0.2, **kw)


def draw_wgrad(rng, form):
    natural = {"auto": SIDES, "direct": SIDES, "f2": (4, 8, 12, 16, 24), "f4": (8, 12, 16, 20, 24)}[form]
    h, w = _side(rng, natural), _side(rng, (8, 16, 24) if form == "f2" else natural)
    n = rng.choice((1, 2, 3))
    if form == "f2":
        c0, c1, cout = rng.choice(((64, 0, 64), (64, 64, 64), (64, 0, 128)))
    elif form == "f4":
        c0, c1, cout = rng.choice(((32, 0, 32), (32, 32, 64), (64, 0, 96)))
    else:
        c0, c1, cout = rng.choice(((8, 0, 24), (8, 12, 40), (32, 0, 72), (64, 0, 64)))
    kw = {}
    if form in ("auto", "direct"):
        stride, pad, pad_end = rng.choice(((1, 1, 0), (1, 1, 0), (1, 0, 0), (2, 0, 0), (2, 0, 1)))
        kw.update(stride=stride, pad=pad, pad_end=pad_end)
    if form == "f4" and rng.random() < 0.3:
        kw["more"] = L.WGRADF_NO_STREAMK
    c = wg(form, "?", n, h, w, c0, c1, cout, rng.choice(sorted(PRO_NAMES)), drop=rng.random() < 0.2, splits=rng.choice((0, 0, 2, 3)), **kw)
    ho, wo = wg_out_size(c)
    return c if ho > 0 and wo > 0 else draw_wgrad(rng, form)


def check_sweep(dev, seed=20240917):
    """Cases drawn from a fixed seed over the axes of the two tables: map sides from SIDES, small channel counts, every forward
    route and every weight-gradient form, plain or fused.  Every case its plan accepts runs and is held to TOL_OP; refusals are
    counted.  At most a quarter of the draws may be refused and every route / form must have run SWEEP_FLOOR cases, so the sweep
    cannot pass by skipping.  The time is bounded by the number of draws (SWEEP_DRAWS per route and form, small shapes)."""
    rng = random.Random(seed)
    form_rng = random.Random(seed + 1)       # (the forms from a stream of their own: a form more or fewer leaves the drawn shapes alone)
    ran, refused, worst, by_form = {}, {}, 0.0, {}
    for i in range(SWEEP_DRAWS):
        for route in SWEEP_FWD:
            c, form = draw_forward(rng, route), form_rng.choice(FORMS)
            ho, wo = out_size(c)
            try:
                if ho < 1 or wo < 1:
                    raise L.SsdeError("no output")
                fwd_plan(c, form)
            except L.SsdeError:
                refused[route] = refused.get(route, 0) + 1
                continue
            worst = max(worst, check_forward(dev, c, form))
            ran[route] = ran.get(route, 0) + 1
            by_form[form] = by_form.get(form, 0) + 1
        for form in SWEEP_WG:
            c = draw_wgrad(rng, form)
            try:
                route, _ = wg_plan(c)
            except L.SsdeError:
                refused["wgrad-" + form] = refused.get("wgrad-" + form, 0) + 1
                continue
            worst = max(worst, check_wgrad(dev, c._replace(runs=route)))
            # (a forced form that falls back to another kernel runs and is checked, but does not count for the form)
            key = "wgrad-" + form if form in ("auto", route) else "wgrad-%s-fell-back" % form
            ran[key] = ran.get(key, 0) + 1
    drawn = SWEEP_DRAWS * (len(SWEEP_FWD) + len(SWEEP_WG))
    print("sweep: %d drawn, %d refused (%s), ran %s, forward launches by form %s, largest error %.3g"
          % (drawn, sum(refused.values()), refused, ran, by_form, worst))
    assert sum(refused.values()) <= SWEEP_REFUSED_MAX * drawn, (refused, drawn)
    assert set(by_form) == set(FORMS), by_form
    for key in SWEEP_FWD + tuple("wgrad-" + f for f in SWEEP_WG):
        assert ran.get(key, 0) >= SWEEP_FLOOR, (key, ran)
    return ran, refused
