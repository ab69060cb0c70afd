// upfirdn2d for NHWC fp32: zero-insert upsample, zero pad, 2-D FIR (true
// convolution, i.e. correlation with the flipped kernel), decimate.
// Reference semantics: upfirdn2d_native (op/upfirdn2d.py:159-200), which the CUDA
// kernel op/upfirdn2d_kernel.cu:107-207 reproduces; callers upsample_2d /
// downsample_2d / conv_downsample_2d (models/up_or_down_sampling.py:144-257) and
// the 2x2 box filters of naive_upsample_2d / naive_downsample_2d (:59-69).
// The optional GroupNorm(+SiLU) prologue implements "h = act(GroupNorm_0(x))"
// of an up/down ResnetBlockBigGANpp (layerspp.py:243-258) without writing h.
//
// HBM-bound: algorithmic traffic = (in + out) * 4 B.  Three kernels:
//  * upfirdn_tile_kernel<UP, DOWN> -- the three shapes the networks use with the 4x4 FIR (up 2 / pad (2,1),
//    down 2 / pad (1,1), pad (2,2)) and their gradients (the same shapes with up and down swapped): one workgroup owns
//    an output tile x 32 channels, stages the input tile it needs ONCE into LDS (zero padding resolved there, the
//    GroupNorm / SiLU prologue applied once per input element instead of once per tap: an input pixel feeds 4 outputs
//    when upsampling and 4..16 taps when downsampling), then every tap is an LDS read with compile-time parity logic.
//    A residual block resamples BOTH act(GroupNorm(x)) and x (layerspp.py:250-258): with `dst2` the raw tile is
//    filtered first, then transformed in place in LDS and filtered again -- x is read from HBM once for both outputs.
//  * upfirdn_wide_kernel<UP, DOWN> -- the same contract for any kh x kw up to 16 x 16 and for negative pads (which crop,
//    op/upfirdn2d.py:176-181): the taps live in LDS behind the staged tile, and with UP == 2 only the taps of the right
//    parity are walked.  Output tile, staged tile and LDS bytes are in the table above ssde_upfirdn2d.
//  * upfirdn_kernel<LDS_TAPS> -- the general form (any up / down / pads, channel counts that are not a multiple of 32
//    such as the 4-channel image pyramids): one lane = 4 channels of one output pixel.  Kernels that fit 4x4 travel in
//    the launch arguments; larger ones are read from ssde_upfirdn_args.taps once per workgroup into LDS.
#include "ssde_common.h"

namespace {

struct FirParams {
  ssde_src src;
  int n, h_in, w_in, c, h_out, w_out, up, down, pad0, pad1, kh, kw;
  float kf[16];   // flipped kernel (kernels that fit 4x4)
  const float* taps;   // [kh][kw] unflipped, device (larger kernels)
  float* dst;
  int accumulate;
};

// flipped taps into LDS: from the device array of a large kernel, or from the launch arguments
template <class P>
__device__ __forceinline__ void fir_taps_to_lds(const P& p, float* wl, int tid) {
  const int nt = p.kh * p.kw;
  for (int i = tid; i < nt; i += 256) wl[i] = p.taps ? p.taps[nt - 1 - i] : p.kf[i];
}

template <bool LDS_TAPS>
__global__ __launch_bounds__(256) void upfirdn_kernel(const FirParams p) {
  SSDE_LDS(wl);                   // LDS_TAPS: kh * kw flipped taps
  if (LDS_TAPS) {
    fir_taps_to_lds(p, wl, threadIdx.x);
    __syncthreads();
  }
  const int c4n = p.c >> 2;
  const size_t total = (size_t)p.n * p.h_out * p.w_out * c4n;
  const SsdePro pro = ssde_pro_decode(p.src);
  const bool use_gn = pro.gn;
  const int cpg = use_gn ? p.c / p.src.gn_groups : 1;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % c4n);
    size_t t = idx / c4n;
    const int ox = (int)(t % p.w_out); t /= p.w_out;
    const int oy = (int)(t % p.h_out);
    const int n = (int)(t / p.h_out);
    const int ch = c4 * 4;
    float mu = 0.f, rs = 1.f;
    float4 gam = make_float4(1.f, 1.f, 1.f, 1.f), bet = make_float4(0.f, 0.f, 0.f, 0.f);
    if (use_gn) {
      const int g = ch / cpg;
      mu = p.src.gn_mean[n * p.src.gn_groups + g];
      rs = p.src.gn_rstd[n * p.src.gn_groups + g];
      gam = *reinterpret_cast<const float4*>(p.src.gn_gamma + ch);
      bet = *reinterpret_cast<const float4*>(p.src.gn_beta + ch);
    }
    const float* xin = p.src.p0 + (size_t)n * p.h_in * p.w_in * p.c + ch;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ky = 0; ky < p.kh; ++ky) {
      const int uy = oy * p.down + ky - p.pad0;
      if (uy < 0 || uy % p.up != 0) continue;
      const int iy = uy / p.up;
      if (iy >= p.h_in) continue;
      for (int kx = 0; kx < p.kw; ++kx) {
        const int ux = ox * p.down + kx - p.pad0;
        if (ux < 0 || ux % p.up != 0) continue;
        const int ix = ux / p.up;
        if (ix >= p.w_in) continue;
        float4 v = *reinterpret_cast<const float4*>(xin + ((size_t)iy * p.w_in + ix) * p.c);
        v = ssde_pro_apply(v, mu, rs, gam, bet,
                           (uint32_t)(((size_t)n * p.h_in + iy) * p.w_in + ix) * (uint32_t)p.c + (uint32_t)ch, pro);
        const float w = LDS_TAPS ? wl[ky * p.kw + kx] : p.kf[ky * p.kw + kx];
        acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
      }
    }
    float4* o = reinterpret_cast<float4*>(p.dst + (((size_t)n * p.h_out + oy) * p.w_out + ox) * p.c + ch);
    if (p.accumulate) { const float4 old = *o; acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w; }
    *o = acc;
  }
}


// ---- LDS-staged tiles for the 4x4 FIR -----------------------------------------------------------------------------
constexpr int kFirCh = 32;        // channels per workgroup: 8 lanes x float4 = one 128-byte line per pixel
struct FirTileParams {
  ssde_src src;
  int n, h_in, w_in, c, h_out, w_out, pad0;
  int lth, ltw;                   // log2 of the output tile (th x tw outputs)
  int ih, iw;                     // staged input tile
  int tiles_x, tiles_y, cchunks;
  float kf[16];                   // flipped kernel
  float* dst; float* dst2;
  int accumulate;
};

// ---- the staged tile of both tiled kernels (P: FirTileParams or FirWideParams) ----
// stage the raw input tile [ih * iw][32 channels], zeros outside the image
template <class P>
__device__ __forceinline__ void fir_stage_tile(const P& p, float* tile, const float* xin, int iy0, int ix0, int slot, int c4) {
  const int npix = p.ih * p.iw;
  // kStageU loads of a thread are issued before the first of them is parked: with one load in flight per thread (a loop the
  // compiler cannot unroll: the tile size is a launch argument) the 4-12 round trips of a tile were paid one after the other
  // and the pass sat at 0.3-0.5 of the HBM peak on every shape but the largest (profiles/r6_fir_staging_unroll.txt)
  constexpr int kStageU = 4;
  for (int base = slot; base < npix; base += 32 * kStageU) {
    float4 v[kStageU];
#pragma unroll
    for (int u = 0; u < kStageU; ++u) {
      const int pix = base + 32 * u;
      const int ly = pix / p.iw, lx = pix - ly * p.iw;
      const int iy = iy0 + ly, ix = ix0 + lx;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pix < npix && iy >= 0 && iy < p.h_in && ix >= 0 && ix < p.w_in)
        v[u] = *reinterpret_cast<const float4*>(xin + ((size_t)iy * p.w_in + ix) * p.c);
    }
#pragma unroll
    for (int u = 0; u < kStageU; ++u) {
      const int pix = base + 32 * u;
      if (pix < npix) *reinterpret_cast<float4*>(tile + pix * kFirCh + c4 * 4) = v[u];
    }
  }
}

// the prologue in place: every thread transforms exactly the elements it staged; padding stays zero (upfirdn2d pads AFTER
// the activation: the reference filters act(GroupNorm(x)) as its own tensor)
template <class P>
__device__ __forceinline__ void fir_prologue_tile(const P& p, const SsdePro& pro, float* tile, int n, int ch, int iy0, int ix0,
                                                  int slot, int c4) {
  const int npix = p.ih * p.iw;
  float mu = 0.f, rs = 1.f;
  float4 gam = make_float4(1.f, 1.f, 1.f, 1.f), bet = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pro.gn) {
    const int g = ch / (p.c / p.src.gn_groups);
    mu = p.src.gn_mean[n * p.src.gn_groups + g];
    rs = p.src.gn_rstd[n * p.src.gn_groups + g];
    gam = *reinterpret_cast<const float4*>(p.src.gn_gamma + ch);
    bet = *reinterpret_cast<const float4*>(p.src.gn_beta + ch);
  }
  for (int pix = slot; pix < npix; pix += 32) {
    const int ly = pix / p.iw, lx = pix - ly * p.iw;
    const int iy = iy0 + ly, ix = ix0 + lx;
    if (iy >= 0 && iy < p.h_in && ix >= 0 && ix < p.w_in) {
      float4* e = reinterpret_cast<float4*>(tile + pix * kFirCh + c4 * 4);
      *e = ssde_pro_apply(*e, mu, rs, gam, bet,
                          (uint32_t)(((size_t)n * p.h_in + iy) * p.w_in + ix) * (uint32_t)p.c + (uint32_t)ch, pro);
    }
  }
}

template <int UP, int DOWN>
__global__ __launch_bounds__(256) void upfirdn_tile_kernel(const FirTileParams p) {
  SSDE_LDS(tile);                 // [ih * iw][32 channels]; then 16 weights re-ordered by tap parity
  const int tid = threadIdx.x, c4 = tid & 7, slot = tid >> 3;
  int b = blockIdx.x;
  const int cc = b % p.cchunks; b /= p.cchunks;
  const int tx = b % p.tiles_x; b /= p.tiles_x;
  const int ty = b % p.tiles_y;
  const int n = b / p.tiles_y;
  const int TH = 1 << p.lth, TW = 1 << p.ltw;
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int ch = cc * kFirCh + c4 * 4;
  // first staged input row / column: floor((o0 * DOWN - pad0) / UP)
  const int uy0 = oy0 * DOWN - p.pad0, ux0 = ox0 * DOWN - p.pad0;
  const int iy0 = UP == 2 ? (uy0 >> 1) : uy0, ix0 = UP == 2 ? (ux0 >> 1) : ux0;
  const int npix = p.ih * p.iw;
  float* wtab = tile + npix * kFirCh;      // [ky & 1][kx & 1][ky >> 1][kx >> 1] for UP == 2
  if (UP == 2 && tid < 16) {
    const int ky = ((tid >> 3) & 1) + 2 * ((tid >> 1) & 1), kx = ((tid >> 2) & 1) + 2 * (tid & 1);
    wtab[tid] = p.kf[ky * 4 + kx];
  }
  const float* xin = p.src.p0 + (size_t)n * p.h_in * p.w_in * p.c + ch;
  fir_stage_tile(p, tile, xin, iy0, ix0, slot, c4);
  __syncthreads();

  auto filter = [&](float* out) {
    for (int op = slot; op < TH * TW; op += 32) {
      const int oy = oy0 + (op >> p.ltw), ox = ox0 + (op & (TW - 1));
      if (oy >= p.h_out || ox >= p.w_out) continue;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (UP == 2) {
        // u = o * DOWN + k - pad0 must be even: k = k0, k0 + 2 with k0 = (pad0 - o * DOWN) & 1; input index u >> 1
        const int ky0 = (p.pad0 - oy * DOWN) & 1, kx0 = (p.pad0 - ox * DOWN) & 1;
        const int ly = ((oy * DOWN + ky0 - p.pad0) >> 1) - iy0, lx = ((ox * DOWN + kx0 - p.pad0) >> 1) - ix0;
        const float4 w = *reinterpret_cast<const float4*>(wtab + (ky0 * 2 + kx0) * 4);
        const float* t0 = tile + (ly * p.iw + lx) * kFirCh + c4 * 4;
        const float4 v00 = *reinterpret_cast<const float4*>(t0);
        const float4 v01 = *reinterpret_cast<const float4*>(t0 + kFirCh);
        const float4 v10 = *reinterpret_cast<const float4*>(t0 + p.iw * kFirCh);
        const float4 v11 = *reinterpret_cast<const float4*>(t0 + p.iw * kFirCh + kFirCh);
        acc.x = w.x * v00.x + w.y * v01.x + w.z * v10.x + w.w * v11.x;
        acc.y = w.x * v00.y + w.y * v01.y + w.z * v10.y + w.w * v11.y;
        acc.z = w.x * v00.z + w.y * v01.z + w.z * v10.z + w.w * v11.z;
        acc.w = w.x * v00.w + w.y * v01.w + w.z * v10.w + w.w * v11.w;
      } else {
        const int ly = oy * DOWN - p.pad0 - iy0, lx = ox * DOWN - p.pad0 - ix0;
        const float* t0 = tile + (ly * p.iw + lx) * kFirCh + c4 * 4;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky)
#pragma unroll
          for (int kx = 0; kx < 4; ++kx) {
            const float4 v = *reinterpret_cast<const float4*>(t0 + (ky * p.iw + kx) * kFirCh);
            const float w = p.kf[ky * 4 + kx];
            acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
          }
      }
      float4* o = reinterpret_cast<float4*>(out + (((size_t)n * p.h_out + oy) * p.w_out + ox) * p.c + ch);
      if (p.accumulate) { const float4 old = *o; acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w; }
      *o = acc;
    }
  };

  const SsdePro pro = ssde_pro_decode(p.src);
  const bool has_pro = pro.gn || pro.silu || pro.drop;
  if (p.dst2) {                    // the un-activated source, filtered with the same taps
    filter(p.dst2);
    __syncthreads();
  }
  if (has_pro) {
    fir_prologue_tile(p, pro, tile, n, ch, iy0, ix0, slot, c4);
    __syncthreads();
  }
  filter(p.dst);
}

// ---- LDS-staged tiles for any kh x kw up to 16 x 16, negative pads included --------------------------------------------
struct FirWideParams {
  ssde_src src;
  int n, h_in, w_in, c, h_out, w_out, pad0, kh, kw;
  int lth, ltw;                   // log2 of the output tile (th x tw outputs)
  int ih, iw;                     // staged input tile
  int tiles_x, tiles_y, cchunks;
  float kf[16];                   // flipped kernel (kernels that fit 4x4)
  const float* taps;              // [kh][kw] unflipped, device (larger kernels)
  float* dst; float* dst2;
  int accumulate;
};

template <int UP, int DOWN>
__global__ __launch_bounds__(256) void upfirdn_wide_kernel(const FirWideParams p) {
  SSDE_LDS(tile);                 // [ih * iw][32 channels]; then kh * kw flipped taps
  const int tid = threadIdx.x, c4 = tid & 7, slot = tid >> 3;
  int b = blockIdx.x;
  const int cc = b % p.cchunks; b /= p.cchunks;
  const int tx = b % p.tiles_x; b /= p.tiles_x;
  const int ty = b % p.tiles_y;
  const int n = b / p.tiles_y;
  const int TH = 1 << p.lth, TW = 1 << p.ltw;
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int ch = cc * kFirCh + c4 * 4;
  // first staged input row / column: floor((o0 * DOWN - pad0) / UP); negative with zero padding, positive where a negative
  // pad0 crops
  const int uy0 = oy0 * DOWN - p.pad0, ux0 = ox0 * DOWN - p.pad0;
  const int iy0 = UP == 2 ? (uy0 >> 1) : uy0, ix0 = UP == 2 ? (ux0 >> 1) : ux0;
  const float* wl = tile + p.ih * p.iw * kFirCh;
  fir_taps_to_lds(p, tile + p.ih * p.iw * kFirCh, tid);
  const float* xin = p.src.p0 + (size_t)n * p.h_in * p.w_in * p.c + ch;
  fir_stage_tile(p, tile, xin, iy0, ix0, slot, c4);
  __syncthreads();

  auto filter = [&](float* out) {
    for (int op = slot; op < TH * TW; op += 32) {
      const int oy = oy0 + (op >> p.ltw), ox = ox0 + (op & (TW - 1));
      if (oy >= p.h_out || ox >= p.w_out) continue;
      // u = o * DOWN + k - pad0 must be a multiple of UP: k = k0, k0 + UP, ... with k0 = (pad0 - o * DOWN) & 1 for UP == 2;
      // tap k0 + UP * j reads staged row ly + j
      const int ky0 = UP == 2 ? (p.pad0 - oy * DOWN) & 1 : 0, kx0 = UP == 2 ? (p.pad0 - ox * DOWN) & 1 : 0;
      const int uy = oy * DOWN + ky0 - p.pad0, ux = ox * DOWN + kx0 - p.pad0;
      const int ly = (UP == 2 ? (uy >> 1) : uy) - iy0, lx = (UP == 2 ? (ux >> 1) : ux) - ix0;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int ky = ky0, j = 0; ky < p.kh; ky += UP, ++j) {
        const float* t0 = tile + ((ly + j) * p.iw + lx) * kFirCh + c4 * 4;
        const float* w0 = wl + ky * p.kw;
        for (int kx = kx0; kx < p.kw; kx += UP, t0 += kFirCh) {
          const float4 v = *reinterpret_cast<const float4*>(t0);
          const float w = w0[kx];
          acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
        }
      }
      float4* o = reinterpret_cast<float4*>(out + (((size_t)n * p.h_out + oy) * p.w_out + ox) * p.c + ch);
      if (p.accumulate) { const float4 old = *o; acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w; }
      *o = acc;
    }
  };

  const SsdePro pro = ssde_pro_decode(p.src);
  const bool has_pro = pro.gn || pro.silu || pro.drop;
  if (p.dst2) {                    // the un-activated source, filtered with the same taps
    filter(p.dst2);
    __syncthreads();
  }
  if (has_pro) {
    fir_prologue_tile(p, pro, tile, n, ch, iy0, ix0, slot, c4);
    __syncthreads();
  }
  filter(p.dst);
}

int pow2_ceil(int v) { int q = 1; while (q < v) q *= 2; return q; }

}  // namespace

// Tiles of upfirdn_wide_kernel: 16x16 outputs when upsampling, 8x8 otherwise (smaller powers of two on smaller maps); the
// staged tile is L + 1 rows for UP == 1 and (L + 1) / 2 + 1 for UP == 2, L = (tile - 1) * DOWN + taps - 1; 128 B per pixel.
//   up down taps   outputs  staged   LDS bytes (tile + taps)
//   2  1    6x6    16x16    11x11     15 632
//   1  2    6x6     8x8     20x20     51 344
//   1  1    6x6     8x8     13x13     21 776
//   2  1   16x16   16x16    16x16     33 792
//   1  2   16x16    8x8     30x30    116 224      (above 64 KiB: the dynamic-LDS attribute is raised once)
//   1  1   16x16    8x8     23x23     68 736
// Which launches take it by default -- those where it was timed against the one-lane-per-output kernel and won (same
// launches, alternated in one process, windows of 5 ms: tools/fir_bench.py wide, profiles/fir_wide_ab.txt; time
// of the tiles / time of one lane per output, batch 256 at 4x4 .. 32x32 and batch 16 at 128x128 / 256x256, plain and
// GroupNorm + SiLU + dst2):
//   3 taps 0.29 - 0.87    4x3 taps 0.26 - 0.83    the 4x4 FIR with pads (-1, -1) 0.23 - 0.93    5 taps 0.19 - 0.60
//   6 taps 0.16 - 0.53    8 taps 0.13 - 0.53      12 taps 0.11 - 0.90
//   16 taps 0.11 - 0.47 upsampling;  0.61 - 0.78 otherwise on maps from 32x32 up and on 16x16 down 2;  1.09 on 16x16 stride 1,
//           1.31 / 1.57 on 8x8 down 2 (an 8x8 output tile stages 23x23 .. 30x30 pixels and three quarters of the lanes idle
//           on a 4x4 output)
// So: every kernel of at least 3 taps on both axes, except the ones past 12x12 without upsampling on maps of fewer than
// 1024 pixels.  Extrapolated, not timed: 7, 9 .. 11 taps (between timed neighbours that all win), 13 .. 15 taps (they follow
// the 16-tap rule) and rectangular kernels other than 4x3.  Kernels with fewer than 3 taps on an axis -- the 2x2 boxes, the
// 1x1 zero insertion, one-dimensional kernels -- were not timed and keep the one-lane-per-output kernel they always had.
// SSDE_FIRF_TILED takes the tiles wherever they are legal, SSDE_FIRF_GENERAL never.
extern "C" int ssde_upfirdn2d(const ssde_upfirdn_args* a, void* stream) {
  SSDE_REQUIRE(a && a->src.p0 && a->dst, "upfirdn2d: null args");
  SSDE_REQUIRE(a->src.p1 == nullptr && a->src.c1 == 0, "upfirdn2d: concatenated source not supported");
  if (int rc = ssde_src_act_check(a->src, "upfirdn2d", "")) return rc;
  SSDE_REQUIRE(a->c > 0 && a->c % 4 == 0 && a->src.c0 == a->c, "upfirdn2d: channels must be a multiple of 4 and match src.c0");
  SSDE_REQUIRE(a->kh >= 1 && a->kh <= SSDE_FIR_MAX_TAPS && a->kw >= 1 && a->kw <= SSDE_FIR_MAX_TAPS,
               "upfirdn2d: kernel %dx%d, at most %dx%d taps", a->kh, a->kw, SSDE_FIR_MAX_TAPS, SSDE_FIR_MAX_TAPS);
  const bool inline_taps = a->kh <= 4 && a->kw <= 4;
  SSDE_REQUIRE(inline_taps || a->taps, "upfirdn2d: a kernel larger than 4x4 needs the taps pointer");
  SSDE_REQUIRE(a->up >= 1 && a->down >= 1, "upfirdn2d: bad up/down");
  SSDE_REQUIRE(a->n > 0 && a->h_in > 0 && a->w_in > 0, "upfirdn2d: empty input");
  // output size exactly as upfirdn2d_native computes it (op/upfirdn2d.py:196-197); negative pads crop (:176-181)
  const int span_h = a->h_in * a->up + a->pad0 + a->pad1 - a->kh, span_w = a->w_in * a->up + a->pad0 + a->pad1 - a->kw;
  SSDE_REQUIRE(span_h >= 0 && span_w >= 0, "upfirdn2d: output size is not positive (input %dx%d, up %d, pads %d %d, kernel %dx%d)",
               a->h_in, a->w_in, a->up, a->pad0, a->pad1, a->kh, a->kw);
  const int eh = span_h / a->down + 1, ew = span_w / a->down + 1;
  SSDE_REQUIRE(eh == a->h_out && ew == a->w_out, "upfirdn2d: output must be %dx%d (got %dx%d)", eh, ew, a->h_out, a->w_out);
  if (a->src.pro_mode == SSDE_PRO_GN || a->src.pro_mode == SSDE_PRO_GN_SILU) {
    SSDE_REQUIRE(a->src.gn_groups > 0 && a->c % a->src.gn_groups == 0 && (a->c / a->src.gn_groups) % 4 == 0,
                 "upfirdn2d: GroupNorm channels-per-group must be a multiple of 4");
    SSDE_REQUIRE(a->src.gn_mean && a->src.gn_rstd && a->src.gn_gamma && a->src.gn_beta, "upfirdn2d: GroupNorm pointers missing");
  }
  float kf[16] = {0.f};
  if (inline_taps)
    for (int y = 0; y < a->kh; ++y)
      for (int x = 0; x < a->kw; ++x) kf[y * a->kw + x] = a->k[(a->kh - 1 - y) * a->kw + (a->kw - 1 - x)];
  const float* taps = inline_taps ? nullptr : a->taps;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool general = (a->flags & SSDE_FIRF_GENERAL) != 0;
  const bool tile_shape = a->c % kFirCh == 0 && a->up <= 2 && a->down <= 2 && !(a->up == 2 && a->down == 2);
  const bool tiled = !general && tile_shape && a->kh == 4 && a->kw == 4 && a->pad0 >= 0 && a->pad1 >= 0;
  if (tiled) {
    FirTileParams p;
    p.src = a->src;
    p.n = a->n; p.h_in = a->h_in; p.w_in = a->w_in; p.c = a->c; p.h_out = a->h_out; p.w_out = a->w_out; p.pad0 = a->pad0;
    const int want = a->up == 2 ? 16 : 8;             // 16x16 outputs from an 11x11 input tile, or 8x8 from 19x19 / 12x12
    const int th = pow2_ceil(a->h_out < want ? a->h_out : want), tw = pow2_ceil(a->w_out < want ? a->w_out : want);
    p.lth = ssde_ilog2(th); p.ltw = ssde_ilog2(tw);
    p.ih = ((th - 1) * a->down + 3) / a->up + 2;
    p.iw = ((tw - 1) * a->down + 3) / a->up + 2;
    p.tiles_x = ssde_cdiv(a->w_out, tw); p.tiles_y = ssde_cdiv(a->h_out, th); p.cchunks = a->c / kFirCh;
    for (int i = 0; i < 16; ++i) p.kf[i] = kf[i];
    p.dst = a->dst; p.dst2 = a->dst2; p.accumulate = a->accumulate;
    const int lds = (p.ih * p.iw * kFirCh + 16) * 4;
    const dim3 grid((unsigned)((size_t)a->n * p.tiles_y * p.tiles_x * p.cchunks));
    if (a->up == 2) hipLaunchKernelGGL((upfirdn_tile_kernel<2, 1>), grid, dim3(256), lds, st, p);
    else if (a->down == 2) hipLaunchKernelGGL((upfirdn_tile_kernel<1, 2>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((upfirdn_tile_kernel<1, 1>), grid, dim3(256), lds, st, p);
    SSDE_LAUNCH_CHECK();
    return SSDE_OK;
  }
  const bool wide_wins = a->kh >= 3 && a->kw >= 3 && (a->up == 2 || a->kh * a->kw <= 144 || a->h_in * a->w_in >= 1024);
  const bool wide = !general && tile_shape && (wide_wins || (a->flags & SSDE_FIRF_TILED));
  if (wide) {
    FirWideParams p;
    p.src = a->src;
    p.n = a->n; p.h_in = a->h_in; p.w_in = a->w_in; p.c = a->c; p.h_out = a->h_out; p.w_out = a->w_out; p.pad0 = a->pad0;
    p.kh = a->kh; p.kw = a->kw;
    const int want = a->up == 2 ? 16 : 8;
    const int th = pow2_ceil(a->h_out < want ? a->h_out : want), tw = pow2_ceil(a->w_out < want ? a->w_out : want);
    p.lth = ssde_ilog2(th); p.ltw = ssde_ilog2(tw);
    const int lh = (th - 1) * a->down + a->kh - 1, lw = (tw - 1) * a->down + a->kw - 1;
    p.ih = a->up == 2 ? (lh + 1) / 2 + 1 : lh + 1;
    p.iw = a->up == 2 ? (lw + 1) / 2 + 1 : lw + 1;
    p.tiles_x = ssde_cdiv(a->w_out, tw); p.tiles_y = ssde_cdiv(a->h_out, th); p.cchunks = a->c / kFirCh;
    for (int i = 0; i < 16; ++i) p.kf[i] = kf[i];
    p.taps = taps;
    p.dst = a->dst; p.dst2 = a->dst2; p.accumulate = a->accumulate;
    const int lds = (p.ih * p.iw * kFirCh + a->kh * a->kw) * 4;
    SSDE_REQUIRE(lds <= 160 * 1024, "upfirdn2d: %d bytes of LDS", lds);
    using Wide = ssde_lds_kernels<upfirdn_wide_kernel<2, 1>, upfirdn_wide_kernel<1, 2>, upfirdn_wide_kernel<1, 1>>;
    const dim3 grid((unsigned)((size_t)a->n * p.tiles_y * p.tiles_x * p.cchunks));
    if (a->up == 2) return ssde_launch_lds<upfirdn_wide_kernel<2, 1>, Wide>("upfirdn2d", grid, dim3(256), lds, st, p);
    if (a->down == 2) return ssde_launch_lds<upfirdn_wide_kernel<1, 2>, Wide>("upfirdn2d", grid, dim3(256), lds, st, p);
    return ssde_launch_lds<upfirdn_wide_kernel<1, 1>, Wide>("upfirdn2d", grid, dim3(256), lds, st, p);
  }
  FirParams p;
  p.src = a->src;
  p.n = a->n; p.h_in = a->h_in; p.w_in = a->w_in; p.c = a->c; p.h_out = a->h_out; p.w_out = a->w_out;
  p.up = a->up; p.down = a->down; p.pad0 = a->pad0; p.pad1 = a->pad1; p.kh = a->kh; p.kw = a->kw;
  for (int i = 0; i < 16; ++i) p.kf[i] = kf[i];
  p.taps = taps;
  p.accumulate = a->accumulate;
  const size_t total = (size_t)a->n * a->h_out * a->w_out * (a->c / 4);
  size_t blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  const dim3 grid((unsigned)blocks);
  const int lds = taps ? a->kh * a->kw * 4 : 0;
  auto launch = [&](const FirParams& q) {
    if (taps) hipLaunchKernelGGL(upfirdn_kernel<true>, grid, dim3(256), lds, st, q);
    else hipLaunchKernelGGL(upfirdn_kernel<false>, grid, dim3(256), 0, st, q);
  };
  if (a->dst2) {                  // general form: the raw source is a second pass
    FirParams q = p;
    q.src.pro_mode = SSDE_PRO_NONE; q.src.drop_thresh = 0; q.dst = a->dst2;
    launch(q);
    SSDE_LAUNCH_CHECK();
  }
  p.dst = a->dst;
  launch(p);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}
