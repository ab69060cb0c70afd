// 3x3 / stride 1 / pad 1 convolution by Winograd F(4x4, 3x3), unfused and batched over the 36 transform positions
// (SSDE_TILE_WINOGRAD4P, ABI 11):
//
//   wino4_xform_vq_kernel (wino4_xform.hip)   V[pos][Cin/4][t][4] = B^T pro(x) B            into the launch's workspace
//   wino4p_gemm_kernel (this file)            M[ks][pos][t][co] = sum_ci V_pos[t][ci] U_pos[ci][co]   36 independent GEMMs
//   wino4p_out_kernel (this file)             Y = A^T (sum_ks M) A + the usual epilogue (ssde_store_tile)
//
// For the 4x4 maps.  A 4x4 map is ONE F(4x4,3x3) tile per image, so a batch of 256 has only 256 tiles: the forms that take
// their parallelism from tiles (conv_wino4r.hip: 32 tiles x 64 couts per workgroup) have 8-32 workgroups there, and splitting
// their reduction eight ways lost to the hand-over.  This form takes its parallelism from the 36 transform
// positions instead: every position is a plain [T x Cin] x [Cin x Cout] GEMM, all of them independent.  V and M round-trip
// through memory, which on large maps is what sinks the unfused form; at 4x4 they are 19 MB and 9 MB per
// 512 -> 256 layer at batch 256 and stay in the last-level cache.
//
// The GEMM: one wave = a 64 (tiles) x 64 (couts) block of one position and one share of the reduction, 2 x 2 blocks of
// v_mfma_f32_32x32x2_f32 (four independent accumulators: the matrix pipe's rate from one wave per SIMD).  Both operands are
// K-major in channel quads exactly as they lie in memory -- V as the transform pass writes it, U as SSDE_PACK_WINO4P lays it
// out ([36][Cin/4][cout_pad][4]) -- so lane (li = lane & 31, lh = lane >> 5) loads channels 2 lh, 2 lh + 1 of its row / column
// with one 8-byte load (a 512-byte run per 32 lanes) straight into the MFMA operand registers: no LDS, no barrier.  Chunks of
// four channel quads are double-buffered in registers, so a chunk's loads have the 32 MFMAs (2048 cycles) of the previous chunk
// to land.  The shares of a split reduction write separate slabs; nothing is handed over between workgroups.
// The output pass: one wave = one tile x 64 couts.  It sums the slabs of the tile in a fixed order (deterministic, no
// atomics), applies A^T M A, parks the 4x4 outputs in LDS and ends in ssde_store_tile (bias, chan_add, residual, out_scale,
// GroupNorm partials: one slice per tile, i.e. per image on the 4x4 maps).
#include "wino4_common.h"
#include <type_traits>

namespace {

constexpr int kGemmWaves = 4;                 // waves of a GEMM workgroup (independent blocks: no LDS, no barrier)
constexpr int kBM = 64, kBN = 64;             // tiles x couts of one wave
constexpr int kKC = 4;                        // channel quads per register chunk (two chunks in flight)
constexpr int kOutLdt = kBN + 4;              // pitch of the output pass's parked tile

struct Wino4pGemmParams {
  const float* v;          // [36][Q][T][4]
  const float* u;          // [36][Q][Np][4]  (SSDE_PACK_WINO4P)
  float* m;                // [ks][36][T][Np]
  int T, Q, Np, m_tiles, n_tiles, ks, qper;
};

__global__ __launch_bounds__(64 * kGemmWaves) void wino4p_gemm_kernel(const Wino4pGemmParams p) {
  const int lane = threadIdx.x & 63;
  int r = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kGemmWaves + (int)(threadIdx.x >> 6));
  // couts fastest: the waves of a workgroup share their V rows
  const int nt = r % p.n_tiles; r /= p.n_tiles;
  const int mt = r % p.m_tiles; r /= p.m_tiles;
  const int pos = r % 36, ks = r / 36;
  if (ks >= p.ks) return;
  const int li = lane & 31, lh = lane >> 5;
  const int t0 = mt * kBM, c0 = nt * kBN;
  // rows beyond the batch read the last tile's run (a valid address; their products are never stored)
  const int ta = min(t0 + li, p.T - 1), tb = min(t0 + 32 + li, p.T - 1);
  const size_t q0 = (size_t)ks * p.qper;
  const float* va = p.v + (((size_t)pos * p.Q + q0) * p.T + ta) * 4 + 2 * lh;
  const float* vb = p.v + (((size_t)pos * p.Q + q0) * p.T + tb) * 4 + 2 * lh;
  const float* ua = p.u + (((size_t)pos * p.Q + q0) * p.Np + c0 + li) * 4 + 2 * lh;
  const float* ub = ua + 32 * 4;
  const size_t vs = (size_t)p.T * 4, us = (size_t)p.Np * 4;     // one channel quad further

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  ssde_f32x2 A[2][kKC][2], B[2][kKC][2];
  auto load = [&](auto SetC, int qi) __attribute__((always_inline)) {
    constexpr int S = decltype(SetC)::value;
#pragma unroll
    for (int k = 0; k < kKC; ++k) {
      const size_t q = (size_t)(qi + k);
      A[S][k][0] = *reinterpret_cast<const ssde_f32x2*>(va + q * vs);
      A[S][k][1] = *reinterpret_cast<const ssde_f32x2*>(vb + q * vs);
      B[S][k][0] = *reinterpret_cast<const ssde_f32x2*>(ua + q * us);
      B[S][k][1] = *reinterpret_cast<const ssde_f32x2*>(ub + q * us);
    }
  };
  // the first MFMA of a quad takes channels {0, 2} (lh = 0, 1), the second {1, 3}: the same pairing on both operands.  The four
  // accumulators in turn, so that no MFMA waits for the one before it
  auto compute = [&](auto SetC) __attribute__((always_inline)) {
    constexpr int S = decltype(SetC)::value;
#pragma unroll
    for (int k = 0; k < kKC; ++k) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[S][k][i].x, B[S][k][j].x, acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[S][k][i].y, B[S][k][j].y, acc[i][j], 0, 0, 0);
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  // qper is a multiple of 2 kKC (the launcher's channel rule).  The load of the chunk after next is unconditional -- on the last
  // trip it re-reads the last chunk -- so that the compiler's wait counts are the same on every trip
  // (sched_barrier: left to itself hipcc sinks every load to just in front of its first MFMA, and each chunk waits out a
  //  whole memory latency)
  load(S0{}, 0);
  for (int qi = 0; qi < p.qper; qi += 2 * kKC) {
    load(S1{}, qi + kKC);
    __builtin_amdgcn_sched_barrier(0);
    compute(S0{});
    __builtin_amdgcn_sched_barrier(0);
    load(S0{}, min(qi + 2 * kKC, p.qper - kKC));
    __builtin_amdgcn_sched_barrier(0);
    compute(S1{});
    __builtin_amdgcn_sched_barrier(0);
  }

  // plain stores into this share's slab: lane (li, lh) holds, of block (i, j), cout c0 + 32 j + li of the rows
  // t0 + 32 i + 8 (e >> 2) + 4 lh + (e & 3)
  float* mo = p.m + ((size_t)ks * 36 + pos) * p.T * p.Np;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int t = t0 + 32 * i + 8 * (e >> 2) + 4 * lh + (e & 3);
      if (t < p.T) {
#pragma unroll
        for (int j = 0; j < 2; ++j) mo[(size_t)t * p.Np + c0 + 32 * j + li] = acc[i][j][e];
      }
    }
}

struct Wino4pOutParams {
  const float* m;          // [ks][36][T][Np]
  int T, Np, ks;
  int H, W, tiles_w, per_img;
  SsdeEpi e;
};

// one wave = one tile x 64 couts (lane = cout): the fixed-order slab sum, A^T M A, then ssde_store_tile
__global__ __launch_bounds__(64) void wino4p_out_kernel(const Wino4pOutParams p) {
  SSDE_LDS(park);                                // [16 pixels][kOutLdt]
  const int lane = threadIdx.x;
  const int t = blockIdx.x, n0 = blockIdx.y * kBN;
  const size_t plane = (size_t)p.T * p.Np, slab = 36 * plane;
  const float* mp = p.m + (size_t)t * p.Np + n0 + lane;
  float mm[36];
#pragma unroll
  for (int pos = 0; pos < 36; ++pos) mm[pos] = mp[pos * plane];
  for (int k = 1; k < p.ks; ++k) {               // ((s0 + s1) + s2) + s3
#pragma unroll
    for (int pos = 0; pos < 36; ++pos) mm[pos] += mp[k * slab + pos * plane];
  }
  // Y = A^T M A with M[a][b] = mm[6 a + b] (a: row of the 6x6 tile); over the rows of every column first (wino4_common.h)
  float y[4][4];
#pragma unroll
  for (int dy = 0; dy < 4; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) y[dy][dx] = 0.f;
#pragma unroll
  for (int px = 0; px < 6; ++px) {
    const float m[6] = {mm[px], mm[6 + px], mm[12 + px], mm[18 + px], mm[24 + px], mm[30 + px]};
    wino4_out_column(px, m, y);
  }
#pragma unroll
  for (int dy = 0; dy < 4; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) park[(dy * 4 + dx) * kOutLdt + lane] = y[dy][dx];
  SSDE_LDS_BARRIER();
  const int img = t / p.per_img, tr = t - img * p.per_img;
  const int ty = tr / p.tiles_w, tx = tr - ty * p.tiles_w;
  auto pixfn = [&](int row, size_t& pix, int& im) {
    im = img;
    pix = ((size_t)img * p.H + ty * 4 + (row >> 2)) * p.W + tx * 4 + (row & 3);
    return true;
  };
  ssde_store_tile<16, kBN, 64, 4, 0>(park, kOutLdt, n0, p.e, pixfn, p.e.gn_part ? t : -1);
}

struct W4pShape {
  int T, Q, Np, ks;
  int64_t v_floats;
  int64_t slab_floats;     // one share's products
};

bool w4p_legal_split(int Q, int ks) { return Q % (2 * kKC * ks) == 0; }

// the shares of the reduction: SSDE_CONVF_NO_KSPLIT = one, SSDE_CONVF_KSPLIT2 / KSPLIT4 = two / four where the channel count
// allows (else the next fewer); otherwise the most shares that keep the launch within ONE wave per SIMD with at least 32 channel
// quads per share.  Measured (tools/w4p_bench.py, GroupNorm + SiLU prologue, ms for 1 / 2 / 4 shares):
//   batch 256 (576 waves unsplit):  256->256 0.039 / 0.060 / 0.067   512->256 0.055 / 0.091 / 0.096   768->256 0.072 / 0.120 / 0.124
//   batch 128 (288 waves):          256->256 0.038 / 0.035 / 0.053   512->256 0.053 / 0.042 / 0.068   768->256 0.070 / 0.051 / 0.084
//   batch 16 (144 waves):           256->256 0.033 / 0.031 / 0.036   512->256 0.050 / 0.040 / 0.042   768->256 0.067 / 0.049 / 0.047
// (a second wave on a SIMD shares its matrix pipe, and every share adds a slab to write and to read back)
int w4p_splits(int waves1, int Q, unsigned flags) {
  if (flags & SSDE_CONVF_NO_KSPLIT) return 1;
  int ks = 1;
  if (flags & (SSDE_CONVF_KSPLIT2 | SSDE_CONVF_KSPLIT4)) {
    ks = (flags & SSDE_CONVF_KSPLIT4) ? 4 : 2;
  } else {
    const int simds = 4 * ssde_num_cus();
    ks = 4;
    while (ks > 1 && (waves1 * ks > simds || Q / ks < 8 * kKC)) ks /= 2;
  }
  while (ks > 1 && !w4p_legal_split(Q, ks)) ks /= 2;
  return ks;
}

// the shape of a launch and the plan the queries report, without touching a device
int w4p_shape(const ssde_conv_args* a, W4pShape* s, ssde_conv_plan* pl) {
  constexpr const char* kRoute = "conv(winograd 4x4, position-batched)";
  if (int rc = wino4_check_shape(a, kRoute, 0)) return rc;        // (maps below 8x8 are this route's)
  const ssde_src& src = a->main;
  if (int rc = ssde_src_check(src, kRoute, "", 4, SSDE_SRC_NEEDS_C0)) return rc;   // (the prologue: wino4_xform.hip)
  const int ctot = src.c0 + src.c1;
  SSDE_REQUIRE(ctot % (8 * kKC) == 0, "conv(winograd 4x4, position-batched): input channels must be a multiple of %d (got %d)", 8 * kKC, ctot);
  SSDE_REQUIRE(a->c_out > 0 && a->c_out % 4 == 0, "conv(winograd 4x4, position-batched): output channels must be a multiple of 4");
  SSDE_REQUIRE((unsigned long long)a->n * a->h_in * a->w_in * (unsigned)ctot < (1ull << 32),
               "conv(winograd 4x4, position-batched): tensor too large");
  s->T = a->n * (a->h_out / 4) * (a->w_out / 4);
  s->Q = ctot / 4;
  s->Np = ssde_cdiv(a->c_out, kBN) * kBN;
  s->ks = w4p_splits(36 * ssde_cdiv(s->T, kBM) * (s->Np / kBN), s->Q, a->flags);
  s->v_floats = (int64_t)36 * s->T * ctot;
  s->slab_floats = (int64_t)36 * s->T * s->Np;
  pl->lds_bytes = 16 * kOutLdt * 4;
  pl->gn_slices = (a->h_out / 4) * (a->w_out / 4);          // one slice per tile (c_out % 4 == 0 on this route)
  pl->ws_floats = s->v_floats + s->ks * s->slab_floats;
  return SSDE_OK;
}

}  // namespace

// The route of a->tile == SSDE_TILE_WINOGRAD4P.  Its workspace (ssde_conv_args.wino_ws) holds V, then the slabs of the shares.
int ssde_conv_wino4p_plan(const ssde_conv_args* a, ssde_conv_plan* pl) {
  W4pShape s;
  return w4p_shape(a, &s, pl);
}

// Everything is validated before the first launch is enqueued.
int ssde_conv_wino4p_launch(const ssde_conv_args* a, hipStream_t st) {
  W4pShape s;
  ssde_conv_plan pl;
  if (int rc = w4p_shape(a, &s, &pl)) return rc;
  // a workspace sized for fewer shares (a plan exported on a device with fewer CUs) takes fewer shares
  while (s.ks > 1 && a->wino_ws_floats < s.v_floats + s.ks * s.slab_floats) s.ks /= 2;
  SSDE_REQUIRE(a->wino_ws && a->wino_ws_floats >= s.v_floats + s.ks * s.slab_floats,
               "conv(winograd 4x4, position-batched): workspace (ssde_conv_args.wino_ws) missing or smaller than %lld floats",
               (long long)(s.v_floats + s.slab_floats));
  float* v = a->wino_ws;
  float* m = a->wino_ws + s.v_floats;
  ssde_conv_args x = *a;                         // the transform pass writes V into the workspace (wino_v is not this route's)
  x.wino_v = v;
  if (int rc = ssde_wino4_xform_vq_launch(&x, st)) return rc;
  const Wino4pGemmParams g{v, a->w_main, m, s.T, s.Q, s.Np, ssde_cdiv(s.T, kBM), s.Np / kBN, s.ks, s.Q / s.ks};
  const int waves = 36 * g.m_tiles * g.n_tiles * s.ks;
  hipLaunchKernelGGL(wino4p_gemm_kernel, dim3(ssde_cdiv(waves, kGemmWaves)), dim3(64 * kGemmWaves), 0, st, g);
  SSDE_LAUNCH_CHECK();
  Wino4pOutParams o;
  o.m = m; o.T = s.T; o.Np = s.Np; o.ks = s.ks;
  o.H = a->h_out; o.W = a->w_out; o.tiles_w = a->w_out / 4; o.per_img = pl.gn_slices;
  o.e = SsdeEpi{a->bias, a->chan_add, a->chan_add_ld, a->resid, a->resid_post, a->out_scale, a->dst, a->c_out, a->gn_part};
  hipLaunchKernelGGL(wino4p_out_kernel, dim3(s.T, s.Np / kBN), dim3(64), pl.lds_bytes, st, o);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}
