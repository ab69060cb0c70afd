// Single-head spatial self-attention core of AttnBlockpp (models/layerspp.py:82-86):
//   w = softmax_j( sum_c q[i,c] k[j,c] * C^-1/2 ),  h[i,c] = sum_j w[i,j] v[j,c]
// with L = H*W tokens and d = C channels, and its backward (what autograd derives for those
// three lines).  fp32 operands on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
// L <= 256 (the 16x16 attention and the 4x4 bottleneck of every shipped config) runs
// on the single-tile kernels described first; 256 < L <= SSDE_ATTN_L_MAX (attn_resolutions of 32
// and more, larger bottlenecks, non-square maps) on the streaming kernels further down.
//
// Forward, one workgroup = 64 query rows of one image:
//   1. S = Q K^T  (4 waves x 64 keys each), Q/K channel chunks staged in LDS
//   2. row softmax on the 64 x L score tile held in LDS (never written to HBM,
//      the reference materialises [B, L, L])
//   3. O = P V   (4 waves x 64 channels each), V chunks staged in LDS as stored
//      (token-major); the k-strided B fragment is read with 4 ds_read_b32.
// Backward re-uses the same two GEMM phases (P is recomputed, never stored):
//   kernel A (per 64 query rows):  P, D_i = dO_i . O_i;  dP = dO V^T;  dS = P o (dP - D);  dQ = scale dS K
//   kernel B (per 64 key rows):    P^T from the saved row max / row sum;  dV = P^T dO;
//                                  dP^T = V dO^T;  dS^T = P^T o (dP^T - D);  dK = scale dS^T Q
// The fp32 kernels of both sets are cut from one copy of each tile step: gemm_nt (A B^T into the accumulators), pv_pass (the P.V
// loop of one 256-channel pass; gemm_pv = zero, pv_pass, store per pass), the accumulator <-> tile mapping (acc_row / acc_col) under
// the epilogues acc_to_tile, acc_to_probs, probs_to_ds, scale_rows and store_acc, online_softmax (softmax_rows is its single
// window, normalised), row_dot (D) and load_stats (m, l, D into LDS).  attn_x6_kernel alone keeps copies of its own: its loads are
// issued from asm and its ISA is pinned (tools/isa_inflight_check.py).
// qkv layout [N, L, 3C]: the fused NIN_0..2 projection output (q | k | v).
#include "ssde_common.h"
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kQB = 64;          // rows per workgroup
constexpr int kLMax = 256;       // tokens of a score tile: all the single-tile kernels take
constexpr int kKB = kLMax;       // keys (dK / dV: queries) per window of the streaming kernels: the same tile, and one St layout for both kernel sets
constexpr int kLDC = 36;         // channel-chunk row stride (32 + 4)
constexpr int kLDP = 260;        // score / V row stride (256 + 4)
constexpr int kTileFloats = kQB * kLDP;                 // the 64 x L tile
constexpr int kStageFloats = (kQB + kLMax) * kLDC;      // Q/K chunk staging (phase 1); >= 32 * kLDP (phase 3)
constexpr int kFwdVch = 8;                              // V tokens per chunk of the forward kernel
constexpr int kAttnLdsFloats = kQB * kLDP + kFwdVch * kLDP;  // forward: Q/K staging aliases the tile in phase 1; 75 KB: two workgroups per CU
constexpr int kBwdLdsFloats = kTileFloats + kStageFloats + 3 * kLMax;   // backward: tile | staging | St[3][256]: m, l, D per row or column

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// The accumulators of a wave's 64 x 64 block (four 32 x 32 results of v_mfma_f32_32x32x2_f32): register r of acc[a][b] holds, in
// lane li + 32 lh, row acc_row(a, r, lh) of the block and column acc_col(kb, b, li) of the tile or output, kb being the block's first
// column there.
__device__ __forceinline__ int acc_row(int a, int r, int lh) { return a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh; }
__device__ __forceinline__ int acc_col(int kb, int b, int li) { return kb + b * 32 + li; }

// acc (wave: rows 0..63 x columns kb..kb+63, kb = wave*64) = A[64 x C] * B[Lk x C]^T.
// A: 64 rows from pointer A (row stride lda), rows >= a_valid read as zero; B likewise with b_valid rows.
__device__ __forceinline__ void gemm_nt(const float* __restrict__ A, int a_valid, size_t lda,
                                        const float* __restrict__ B, int b_valid, size_t ldb, int C, int Lk,
                                        float* Qs, float* Ks, f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int kb = wave * 64;
  zero_acc(acc);
  // The 32-channel chunk c0+32 is fetched into registers while the MFMAs of chunk c0 run (as fixed-count, branch-free
  // loads: rows past the valid range read a clamped address and are zeroed); it is parked in LDS behind the barrier.
  const int f = tid & 7, r0 = tid >> 3;                   // item (row r0 + 32 it, channel quad f)
  float4 ra[2], rb[8];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = r0 + it * 32;
      const float4 v = *reinterpret_cast<const float4*>(A + (size_t)max(min(row, a_valid - 1), 0) * lda + c0 + f * 4);
      ra[it] = row < a_valid ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int row = r0 + it * 32;
      const float4 v = *reinterpret_cast<const float4*>(B + (size_t)max(min(row, b_valid - 1), 0) * ldb + c0 + f * 4);
      rb[it] = row < b_valid ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  load_chunk(0);
  for (int c0 = 0; c0 < C; c0 += 32) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) *reinterpret_cast<float4*>(Qs + (r0 + it * 32) * kLDC + f * 4) = ra[it];
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (r0 + it * 32 < Lk) *reinterpret_cast<float4*>(Ks + (r0 + it * 32) * kLDC + f * 4) = rb[it];
    __syncthreads();
    if (c0 + 32 < C) load_chunk(c0 + 32);
    if (kb < Lk) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        float4 af[2], bf[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) af[a] = *reinterpret_cast<const float4*>(Qs + (a * 32 + li) * kLDC + kk * 8 + lh * 4);
#pragma unroll
        for (int b = 0; b < 2; ++b) bf[b] = *reinterpret_cast<const float4*>(Ks + (kb + b * 32 + li) * kLDC + kk * 8 + lh * 4);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].x, bf[b].x, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].y, bf[b].y, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].z, bf[b].z, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].w, bf[b].w, acc[a][b], 0, 0, 0);
          }
      }
    }
  }
}

// acc += Ps[64 x Lp] * Bm[rows x (cp .. cp + Cw)]   (Bm token-major rows, row stride ldb, rows >= b_valid zero): the P.V loop of every
// fp32 kernel, for one 256-channel pass of which the wave takes 64 channels.  VCH = tokens of V staged per chunk (a multiple of 8):
// 32 in the backward kernels; 8 in the forward kernel, whose LDS footprint (64 x 260 score tile + the chunk) then lets two
// workgroups share a CU; 16 in the streaming forward.
template <int VCH>
__device__ __forceinline__ void pv_pass(const float* Ps, int Lp, const float* __restrict__ Bm, int b_valid, size_t ldb, int cp, int Cw,
                                        float* Vs, f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int cb = wave * 64;
  constexpr int NIT = VCH / 4;
  const int f4n = Cw >> 2;
  int vrow[NIT], vf[NIT];
  {
    int row = tid / f4n, ff = tid - row * f4n;
    const int dr = 256 / f4n, df = 256 - dr * f4n;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      vrow[it] = row; vf[it] = ff;
      row += dr; ff += df;
      if (ff >= f4n) { ff -= f4n; ++row; }
    }
  }
  float4 rv[NIT];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int tok = k0 + vrow[it];
      const float4 v = *reinterpret_cast<const float4*>(Bm + (size_t)max(min(tok, b_valid - 1), 0) * ldb + cp + vf[it] * 4);
      rv[it] = (vrow[it] < VCH && tok < b_valid) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  load_chunk(0);
  for (int k0 = 0; k0 < Lp; k0 += VCH) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (vrow[it] < VCH) *reinterpret_cast<float4*>(Vs + vrow[it] * kLDP + vf[it] * 4) = rv[it];
    __syncthreads();
    if (k0 + VCH < Lp) load_chunk(k0 + VCH);
    if (cb < Cw) {
#pragma unroll
      for (int kk = 0; kk < VCH / 8; ++kk) {
        float4 af[2];
        float bf[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a) af[a] = *reinterpret_cast<const float4*>(Ps + (a * 32 + li) * kLDP + k0 + kk * 8 + lh * 4);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int j = 0; j < 4; ++j) bf[b][j] = Vs[(kk * 8 + lh * 4 + j) * kLDP + cb + b * 32 + li];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].x, bf[b][0], acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].y, bf[b][1], acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].z, bf[b][2], acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a].w, bf[b][3], acc[a][b], 0, 0, 0);
          }
      }
    }
  }
}

// acc[a][b][r] *= Rs[row of (a, r)]   (Rs: one float per row of the 64-row block, in LDS)
__device__ __forceinline__ void scale_rows(f32x16 (&acc)[2][2], const float* Rs) {
  const int lh = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float s = Rs[acc_row(a, r, lh)];
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b][r] *= s;
    }
}

// out[row][cp + wave's 64 channels] = acc * mul for rows < out_valid, channels < C
__device__ __forceinline__ void store_acc(const f32x16 (&acc)[2][2], float* __restrict__ out, size_t ldo, int out_valid, int cp, int C,
                                          float mul) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = acc_col(cp + wave * 64, b, li);
      if (col >= C) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = acc_row(a, r, lh);
        if (row < out_valid) out[(size_t)row * ldo + col] = acc[a][b][r] * mul;
      }
    }
}

// out[64 x C] = out_scale * Ps[64 x Lp] * Bm[L x C], one 256-channel pass after the other
template <int VCH = 32>
__device__ __forceinline__ void gemm_pv(const float* Ps, int Lp, const float* __restrict__ Bm, int b_valid, size_t ldb, int C,
                                        float* Vs, float* __restrict__ out, size_t ldo, int out_valid, float out_scale) {
  f32x16 acc[2][2];
  for (int cp = 0; cp < C; cp += 256) {
    zero_acc(acc);
    pv_pass<VCH>(Ps, Lp, Bm, b_valid, ldb, cp, min(256, C - cp), Vs, acc);
    store_acc(acc, out, ldo, out_valid, cp, C, out_scale);
  }
}

// accumulators (wave's 64 x 64 block of the 64 x Lk tile) -> LDS tile, times `mul`
__device__ __forceinline__ void acc_to_tile(const f32x16 (&acc)[2][2], float* Ps, int Lk, float mul) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5, kb = wave * 64;
  if (kb < Lk) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(a, r, lh), col = acc_col(kb, b, li);
          Ps[row * kLDP + col] = acc[a][b][r] * mul;
        }
  }
}

// One window of the online softmax over the first Lb columns of the tile (4 lanes per row):
// m_new = max(m, row max), alpha = exp(m - m_new), l = l * alpha + sum_j exp(s_j - m_new).  kWriteP: the tile becomes
// exp(s - m_new) with columns Lb .. roundup(Lb, 32) - 1 zeroed.  Returns alpha (the same value in the 4 lanes of a row).
template <bool kWriteP>
__device__ __forceinline__ float online_softmax(float* Ps, int Lb, float& m_run, float& l_run) {
  const int tid = threadIdx.x;
  const int row = tid >> 2, sub = tid & 3;
  float* prow = Ps + row * kLDP;
  float m = -INFINITY;
  for (int j = sub; j < Lb; j += 4) m = fmaxf(m, prow[j]);
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  m = fmaxf(m, m_run);
  const float alpha = __expf(m_run - m);                    // first window: exp(-inf) = 0 against l = 0 and O = 0
  float sum = 0.f;
  for (int j = sub; j < Lb; j += 4) {
    const float e = __expf(prow[j] - m);
    if (kWriteP) prow[j] = e;
    sum += e;
  }
  sum += __shfl_xor(sum, 1, 64);
  sum += __shfl_xor(sum, 2, 64);
  if (kWriteP) {
    const int Lp = (Lb + 31) & ~31;
    for (int j = Lb + sub; j < Lp; j += 4) prow[j] = 0.f;
  }
  l_run = l_run * alpha + sum;
  m_run = m;
  return alpha;
}

// softmax over the first L columns of each of the 64 rows, columns L..Lp-1 zeroed: the only window of an online softmax (alpha =
// exp(-inf) = 0 against l = 0), normalised in place.  m, l: the row max and the row sum of exp (the same in the 4 lanes of a row).
__device__ __forceinline__ void softmax_rows(float* Ps, int L, float& m, float& l) {
  m = -INFINITY; l = 0.f;
  online_softmax<true>(Ps, L, m, l);
  float* prow = Ps + (threadIdx.x >> 2) * kLDP;
  const float inv = 1.0f / l;
  for (int j = threadIdx.x & 3; j < L; j += 4) prow[j] *= inv;
}

__global__ __launch_bounds__(256) void attn_kernel(const float* __restrict__ qkv, float* __restrict__ dst,
                                                   int N, int L, int C, float scale) {
  SSDE_LDS(smem);
  float* Qs = smem;                       // [64][36]
  float* Ks = smem + kQB * kLDC;          // [256][36]
  float* Ps = smem;                       // [64][260]   (after step 1)
  float* Vs = smem + kQB * kLDP;          // [kFwdVch][260]
  const int n = blockIdx.y, q0 = blockIdx.x * kQB;
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * L * C3;
  const int Lk = (L + 63) & ~63;          // keys rounded to a wave block
  const int Lp = (L + 31) & ~31;

  f32x16 acc[2][2];
  gemm_nt(base + (size_t)q0 * C3, L - q0, C3, base + C, L, C3, C, Lk, Qs, Ks, acc);
  __syncthreads();
  acc_to_tile(acc, Ps, Lk, scale);
  __syncthreads();
  float m, l;
  softmax_rows(Ps, L, m, l);
  gemm_pv<kFwdVch>(Ps, Lp, base + 2 * C, L, C3, C, Vs, dst + ((size_t)n * L + q0) * C, C, L - q0, 1.0f);
}

// ---- forward on the BF16 matrix pipe (SSDE_ATTNF_BF16X6): both contractions as exact-fp32 products of a 3-way bf16 split ------
// The fp32-MFMA kernel above spends 2 x 32 k matrix cycles per wave on the two contractions of a 64-row block and sits at 0.48 of
// that pipe's peak (0.217 ms per launch at 16x16, batch 256: five launches per U-Net evaluation).  v_mfma_f32_32x32x16_bf16 does
// the same contraction in 6/16 of the time (ssde_common.h: SSDE_MFMA_BF16X6, the 1x1 GEMMs' split -- every partial product exact
// in the fp32 accumulator, what is dropped is below the rounding of the product itself), so the kernel is re-cut around what then
// bounds it -- staging and LDS traffic:
//   * one workgroup of EIGHT waves per CU owns 64 query rows of one image and (almost) all of the CU's LDS;
//   * Q is split ONCE into three bf16 planes for all channels (98 KB at C = 256); K arrives in 16-channel stages, V in
//     16-token stages, split by the thread that loaded them, two stages in LDS and two more in flight in registers
//     (loads return in order; the barriers wait for LDS only);
//   * phase 1, S = Q K^T: wave w owns keys 32 w .. 32 w + 31 (two 32 x 32 blocks); phase 3, O = P V: channels 32 w .. 32 w + 31;
//   * phase 2: scaled scores -> fp32 tile (over the dead Q planes) -> every thread takes 32 consecutive keys of one row into
//     registers -> max / exp / sum over the 8 threads of a row by shuffles (the arithmetic of softmax_rows) -> P written as three
//     bf16 planes in the A-fragment layout;
//   * V is staged TRANSPOSED ([channel][16 tokens] bf16, the B fragment wants 8 consecutive tokens of a channel per lane): a
//     thread holds two tokens x four channels, packs token pairs into dwords and writes channel (j + (quad >> 1)) & 3 in its j-th
//     store, which spreads the 64 lanes of a store over the 64 banks;
//   * the four workgroups of an image run on ONE XCD (they read the same K and V: L2 hits).
// L == 256 and C % 64 == 0, C <= 256 only (the 16x16 attention of every shipped config); anything else stays on attn_kernel.
namespace x6 {
constexpr int kT = 512, kRows = 64, kL = 256;
constexpr int kKStage = 3 * kL * 32;                      // bytes of one K stage: [3 pieces][256 keys][16 channels] bf16
constexpr int kPPlane = kL * kRows * 2;                   // bytes of one P piece: [16 token steps][64 rows][16 tokens] bf16
constexpr int kMain = 3 * kPPlane;                        // Q planes (<= this for C <= 256) | fp32 score tile | P planes
constexpr int kLds = kMain + 2 * kKStage;                 // (a V stage is 3 * C * 32 <= kKStage bytes)
static_assert(kRows * kLDP * 4 <= kMain, "score tile");

// x -> its three bf16 pieces as the upper halves of three dwords (ssde_split3's arithmetic)
__device__ __forceinline__ void split_hi(float x, uint32_t& a, uint32_t& b, uint32_t& c) {
  a = __builtin_bit_cast(uint32_t, x);
  const float r = x - __builtin_bit_cast(float, a & 0xffff0000u);
  b = __builtin_bit_cast(uint32_t, r);
  c = __builtin_bit_cast(uint32_t, r - __builtin_bit_cast(float, b & 0xffff0000u));
}
}  // namespace x6

// kNst = C / 16, the number of K stages, is a template parameter: the producers' code is then straight-line from the first request to
// the last wait (no loop-carried copies of a register whose load is in flight; tools/isa_inflight_check.py walks the emitted ISA)
template <int kNst>
__global__ __launch_bounds__(x6::kT) void attn_x6_kernel(const float* __restrict__ qkv, float* __restrict__ dst, int N, float scale) {
  using namespace x6;
  constexpr int C = 16 * kNst;
  SSDE_LDS(smem);
  char* lds = reinterpret_cast<char*>(smem);
  char* stage0 = lds + kMain;
  char* stage1 = stage0 + kKStage;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  // workgroup -> (image, 64-row block): the four blocks of an image are consecutive workgroups of ONE XCD
  const int xcd = blockIdx.x & 7, k_in = blockIdx.x >> 3;
  const int n = (k_in >> 2) * 8 + xcd, q0 = (k_in & 3) * kRows;
  if (n >= N) return;
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * kL * C3;
  const int qplane = C * kRows * 2;                        // bytes of one Q piece: [C / 16][64 rows][16 channels] bf16
  constexpr int nst = kNst;                                 // K stages (a multiple of 4: C % 64 == 0)

  // ---- roles.  Waves 0-3 are CONSUMERS: each owns a 64 x 64 block of the products (64 query rows x 64 keys in phase 1, x 64
  // channels in phase 3: four 32 x 32 accumulators) and does nothing but read fragments and issue MFMAs.  Waves 4-7 are PRODUCERS:
  // they stream K and V (requests, counted waits, the 3-way split, the parking in LDS).  A SIMD holds one wave of each kind, so the
  // split runs beside the MFMAs by itself, and the fragments of a stage are read by four waves instead of eight (48 KB per
  // stage instead of 72: in the first form -- eight waves with 64 x 32 blocks, each also staging -- the LDS reads behind every barrier,
  // then the MFMAs, then the split took turns: 0.163 ms per launch, profiles/r6_attention_x6_versions.txt).
  const bool consumer = wave < 4;                          // (uniform)
  f32x16 acc[2][2];
  auto zero = [&]() {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  };
  // The operands of a stage's MFMAs: A = rows (a * 32 + li) of the planes at `ap` (piece pitch a_pitch), B = rows (64 wave + b * 32
  // + li) of the stage at `bp` (piece pitch b_pitch); a lane reads 16 bytes = 8 consecutive k of its row
  struct Frags { ssde_u32x4 A[2][3], B[2][3]; };
  auto read_frags = [&](Frags& f, const char* ap, int a_pitch, const char* bp, int b_pitch) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int a = 0; a < 2; ++a) f.A[a][q] = *reinterpret_cast<const ssde_u32x4*>(ap + q * a_pitch + (a * 32 + li) * 32 + lh * 16);
#pragma unroll
      for (int b = 0; b < 2; ++b) f.B[b][q] = *reinterpret_cast<const ssde_u32x4*>(bp + q * b_pitch + (wave * 64 + b * 32 + li) * 32 + lh * 16);
    }
  };
  // smallest terms first.  Six terms (SSDE_MFMA_BF16X6) drop a1 b2 + a2 b1 + a2 b2 <= 2^-23 |a b| per product; the scores take
  // EIGHT (all but a2 b2 <= 2^-32 |a b|): with pieces taken by truncation the dropped terms are a one-sided error, and the scores
  // of a peaked query row (|q| ~ 10) carry it into the exponent.  P V, with P in [0, 1], keeps six.
  auto mfmas = [&](auto Terms, const Frags& f) __attribute__((always_inline)) {
    constexpr int kTerms = decltype(Terms)::value;
    constexpr int TI[8] = {1, 2, 0, 2, 1, 0, 1, 0}, TJ[8] = {2, 1, 2, 0, 1, 1, 0, 0};
#pragma unroll
    for (int t = 8 - kTerms; t < 8; ++t)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ssde_bf16x8, f.A[a][TI[t]]),
                                                              __builtin_bit_cast(ssde_bf16x8, f.B[b][TJ[t]]), acc[a][b], 0, 0, 0);
  };
  using Six = std::integral_constant<int, 6>;
  using Eight = std::integral_constant<int, 8>;

  // ---- the streamed operands (producers): K in nst stages of 16 channels, then V in 16 stages of 16 tokens, ONE stream through a
  // register ring of four elements.  Element u + 4 is requested at the top of stage u -- the first V stages during the last K
  // stages, so they land under the softmax -- and has three stages to land.  The loads are asm statements hipcc does not track,
  // four per element and thread, counted by the kernel itself: "element u + 1 has landed" is vmcnt(12) (elements u + 2 .. u + 4 are
  // younger), 8 / 4 / 0 over the last V stages.  Every requested element is consumed (no load lands in a register hipcc considers
  // free) and the whole stream lives inside the producers' arm of the role branch (no copy of a register in flight at a join).
  // History: loads hipcc tracked ran one stage ahead in effect -- it waits vmcnt(0) in front of every store once a guard sits
  // near them: 50 us per workgroup.
  const int ptid = tid & 255;                               // thread of the producer half
  const float* kbase = base + C;
  const float* vbase = base + 2 * C;
  // K: a producer thread stages (key row (ptid >> 2) + 64 i, channel quad ptid & 3), i = 0 .. 3, of the stage's 256 x 4
  const int krow = ptid >> 2, kf = ptid & 3;
  const uint32_t koff = (uint32_t)((krow * C3 + kf * 4) * 4), kstep = (uint32_t)(64 * C3 * 4);
  // V: tokens 2 tp, 2 tp + 1 of the channel quads fq0 and fq0 + 32
  const int tp = ptid & 7, fq0 = ptid >> 3;
  const bool v_on0 = fq0 * 4 < C, v_on1 = (fq0 + 32) * 4 < C;
  const uint32_t voff = (uint32_t)((2 * tp * C3 + (v_on0 ? fq0 * 4 : 0)) * 4), vtok = (uint32_t)(C3 * 4), vquad = v_on1 ? 512u : 0u;
  const int vpitch = C * 32;                                // bytes of one piece of a V stage: [C channels][16 tokens] bf16
  auto request = [&](int u, ssde_f32x4 (&Rs)[4]) __attribute__((always_inline)) {      // stream element u (uniform)
    const bool is_k = u < nst;
    const float* sb = is_k ? kbase + u * 16 : vbase + (size_t)(u - nst) * 16 * C3;       // (scalar)
    const uint32_t o0 = is_k ? koff : voff;
    const uint32_t o1 = o0 + (is_k ? kstep : vtok);                    // K: row + 64       V: token 2 tp + 1
    const uint32_t o2 = is_k ? o0 + 2 * kstep : o0 + vquad;            // K: row + 128      V: quad fq0 + 32, token 2 tp
    const uint32_t o3 = is_k ? o0 + 3 * kstep : o2 + vtok;             // K: row + 192      V: quad fq0 + 32, token 2 tp + 1
    SSDE_GLOAD16_I_SAFE(Rs[0], o0, sb, 0);
    SSDE_GLOAD16_I_SAFE(Rs[1], o1, sb, 0);
    SSDE_GLOAD16_I_SAFE(Rs[2], o2, sb, 0);
    SSDE_GLOAD16_I_SAFE(Rs[3], o3, sb, 0);
  };
#ifdef SSDE_EMULATED
#define SSDE_X6_WAIT(n, Rs) ((void)0)
#else
#define SSDE_X6_WAIT(n, Rs) asm volatile("s_waitcnt vmcnt(%4)" : "+v"((Rs)[0]), "+v"((Rs)[1]), "+v"((Rs)[2]), "+v"((Rs)[3]) : "n"(n) : "memory")
#endif
  // a K element split and parked: [3 pieces][256 keys][16 channels] bf16
  auto park_k = [&](const ssde_f32x4 (&Rs)[4], char* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint2 p0, p1, p2;
      ssde_split3(make_float4(Rs[i].x, Rs[i].y, Rs[i].z, Rs[i].w), p0, p1, p2);
      char* d = buf + (krow + 64 * i) * 32 + kf * 8;
      *reinterpret_cast<uint2*>(d) = p0;
      *reinterpret_cast<uint2*>(d + kL * 32) = p1;
      *reinterpret_cast<uint2*>(d + 2 * kL * 32) = p2;
    }
  };
  // a V element, TRANSPOSED: [3 pieces][C channels][16 tokens] bf16, a dword = (token 2 tp) | (token 2 tp + 1) << 16.  The j-th
  // store of a thread writes channel (j + rot) & 3 of its quad, rot = (fq >> 1) & 3: the 64 lanes of one store hit 64 different
  // banks.  The rotation of the four words is two rounds of selects (v_cndmask), no branches
  const int rot = (fq0 >> 1) & 3;                           // (the same for fq0 + 32)
  const bool rot1 = (rot & 1) != 0, rot2 = (rot & 2) != 0;
  auto park_v = [&](const ssde_f32x4 (&Rs)[4], char* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {                           // quad fq0 + 32 h
      const float f0[4] = {Rs[2 * h].x, Rs[2 * h].y, Rs[2 * h].z, Rs[2 * h].w};
      const float f1[4] = {Rs[2 * h + 1].x, Rs[2 * h + 1].y, Rs[2 * h + 1].z, Rs[2 * h + 1].w};
      uint32_t w[3][4], y[3][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t a0, b0, c0, a1, b1, c1;
        split_hi(f0[i], a0, b0, c0);
        split_hi(f1[i], a1, b1, c1);
        w[0][i] = ssde_pack_hi16(a0, a1); w[1][i] = ssde_pack_hi16(b0, b1); w[2][i] = ssde_pack_hi16(c0, c1);
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        uint32_t x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = rot1 ? w[q][(i + 1) & 3] : w[q][i];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[q][i] = rot2 ? x[(i + 2) & 3] : x[i];
      }
      if (h == 0 ? v_on0 : v_on1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          char* d = buf + ((fq0 + 32 * h) * 4 + ((j + rot) & 3)) * 32 + tp * 4;
#pragma unroll
          for (int q = 0; q < 3; ++q) *reinterpret_cast<uint32_t*>(d + q * vpitch) = y[q][j];
        }
      }
    }
  };

  // ---- phase 1: S = Q K^T ----
  ssde_f32x4 R[4][4];                                       // (producers)
  zero();
  if (!consumer) { request(0, R[0]); request(1, R[1]); request(2, R[2]); request(3, R[3]); }       // before Q: they land under its split
  {
    // Q: every channel of the 64 rows, split once by all eight waves (up to 8 float4 of a thread requested together)
    const int cq4 = C >> 2, total = kRows * cq4;            // channel quads per row
    for (int item0 = tid; item0 < total; item0 += 8 * kT) {
      float4 qv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int item = min(item0 + u * kT, total - 1);
        const int row = item / cq4, cq = item - row * cq4;
        qv[u] = *reinterpret_cast<const float4*>(base + (size_t)(q0 + row) * C3 + cq * 4);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int item = item0 + u * kT;
        if (item < total) {
          const int row = item / cq4, cq = item - row * cq4;
          uint2 p0, p1, p2;
          ssde_split3(qv[u], p0, p1, p2);
          char* d = lds + (cq >> 2) * (kRows * 32) + row * 32 + (cq & 3) * 8;
          *reinterpret_cast<uint2*>(d) = p0;
          *reinterpret_cast<uint2*>(d + qplane) = p1;
          *reinterpret_cast<uint2*>(d + 2 * qplane) = p2;
        }
      }
    }
  }
  if (consumer) {
    SSDE_LDS_BARRIER();                                    // (the Q planes and K stage 0 are complete)
    for (int u = 0; u < nst; ++u) {
      Frags f;
      read_frags(f, lds + u * (kRows * 32), qplane, (u & 1) ? stage1 : stage0, kL * 32);
      mfmas(Eight{}, f);
      SSDE_LDS_BARRIER();
    }
  } else {
    // (the Q loads above are younger than the four requests and have been consumed: loads return in order, so the ring has landed)
    SSDE_X6_WAIT(12, R[0]);
    park_k(R[0], stage0);
    SSDE_LDS_BARRIER();
#pragma unroll
    for (int u = 0; u < nst; ++u) {                        // (straight-line: every index is a compile-time constant)
      const int j = u & 3;
      request(u + 4, R[j]);                                 // R[j] held element u: parked in LDS during stage u - 1
      SSDE_X6_WAIT(12, R[(j + 1) & 3]);                     // element u + 1 (at u = nst - 1: V stage 0, parked in phase 3)
      if (u + 1 < nst) park_k(R[(j + 1) & 3], (j & 1) ? stage0 : stage1);
      SSDE_LDS_BARRIER();
    }
    // V stages 1 .. 3 are still in flight: waited for HERE, before the softmax -- its 32 scores per thread could make hipcc move
    // the ring, and a register must not be copied while its load is in flight (they were requested 1-3 stages ago)
    SSDE_X6_WAIT(8, R[1]); SSDE_X6_WAIT(4, R[2]); SSDE_X6_WAIT(0, R[3]);
  }

  // ---- phase 2: softmax of the 64 x 256 scores; P as three bf16 planes (all eight waves) ----
  {
    float* tile = smem;                                    // [64][kLDP] over the Q planes (every wave is behind the last barrier)
    if (consumer) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            tile[row * kLDP + wave * 64 + b * 32 + li] = acc[a][b][r] * scale;
          }
    }
    SSDE_LDS_BARRIER();
    const int row = tid >> 3, sub = tid & 7;               // keys 32 sub .. 32 sub + 31 of the row
    float x[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(tile + row * kLDP + sub * 32 + i * 4);
      x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
    }
    SSDE_LDS_BARRIER();                                    // the tile is in registers: the P planes may overwrite it
    float m = x[0];
#pragma unroll
    for (int i = 1; i < 32; ++i) m = fmaxf(m, x[i]);
    m = fmaxf(m, __shfl_xor(m, 1, 64));
    m = fmaxf(m, __shfl_xor(m, 2, 64));
    m = fmaxf(m, __shfl_xor(m, 4, 64));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) { x[i] = __expf(x[i] - m); sum += x[i]; }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int u = 0; u < 4; ++u) {                          // 16-byte units: token step 2 sub + (u >> 1), half u & 1
      uint2 a0, a1, a2, b0, b1, b2;
      ssde_split3(make_float4(x[8 * u] * inv, x[8 * u + 1] * inv, x[8 * u + 2] * inv, x[8 * u + 3] * inv), a0, a1, a2);
      ssde_split3(make_float4(x[8 * u + 4] * inv, x[8 * u + 5] * inv, x[8 * u + 6] * inv, x[8 * u + 7] * inv), b0, b1, b2);
      char* d = lds + (2 * sub + (u >> 1)) * (kRows * 32) + row * 32 + (u & 1) * 16;
      *reinterpret_cast<uint4*>(d) = make_uint4(a0.x, a0.y, b0.x, b0.y);
      *reinterpret_cast<uint4*>(d + kPPlane) = make_uint4(a1.x, a1.y, b1.x, b1.y);
      *reinterpret_cast<uint4*>(d + 2 * kPPlane) = make_uint4(a2.x, a2.y, b2.x, b2.y);
    }
  }

  // ---- phase 3: O = P V over 16 stages of 16 tokens ----
  if (consumer) {
    const bool w_on = wave * 64 < C;                        // (C < 256: the upper consumers only keep the barriers)
    zero();
    SSDE_LDS_BARRIER();                                    // (the P planes and V stage 0 are complete)
    for (int v = 0; v < 16; ++v) {
      if (w_on) {
        Frags f;
        read_frags(f, lds + v * (kRows * 32), kPPlane, (v & 1) ? stage1 : stage0, vpitch);
        mfmas(Six{}, f);
      }
      SSDE_LDS_BARRIER();
    }
    if (w_on) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float* out = dst + ((size_t)n * kL + q0) * C + wave * 64 + b * 32 + li;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            out[(size_t)row * C] = acc[a][b][r];
          }
      }
    }
  } else {
    park_v(R[0], stage0);                                  // (V stages 0 .. 3 have landed: end of phase 1)
    SSDE_LDS_BARRIER();
#pragma unroll
    for (int v = 0; v < 16; ++v) {                         // (straight-line: every index below is a compile-time constant)
      const int j = v & 3;
      if (v + 4 < 16) request(nst + v + 4, R[j]);
      if (v + 1 < 16) {
        // element v + 1: stages 1 .. 3 landed before the softmax; from 4 on, the stages requested behind it are younger
        // (v = 3: stages 5 .. 7 and nothing older in flight; the last ones: 8 / 4 / 0)
        if (v + 1 >= 4) {
          if (v + 4 < 16) SSDE_X6_WAIT(12, R[(j + 1) & 3]);
          else if (v + 3 < 16) SSDE_X6_WAIT(8, R[(j + 1) & 3]);
          else if (v + 2 < 16) SSDE_X6_WAIT(4, R[(j + 1) & 3]);
          else SSDE_X6_WAIT(0, R[(j + 1) & 3]);
        }
        park_v(R[(j + 1) & 3], (j & 1) ? stage0 : stage1);
      }
      SSDE_LDS_BARRIER();
    }
  }
#undef SSDE_X6_WAIT
}

// ---- what the backward kernels of both sets share -----------------------------------------------------------------------------
// St[3][kKB] in LDS holds m, l and D = sum_c dO * O of the tile's query rows: indexed by the tile's ROW where a workgroup owns
// 64 queries (dQ: the first 64 of each), by its COLUMN where it owns 64 keys and the queries are the window (dK / dV).

// sum_c o[row][c] * d_o[row][c] of row tid >> 2 of the 64-row block that starts at row `first` of o / d_o [N * L][C] (4 lanes per
// row, each returns the sum); 0 for rows >= valid
__device__ __forceinline__ float row_dot(const float* __restrict__ o, const float* __restrict__ d_o, size_t first, int C, int valid) {
  const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
  float d = 0.f;
  if (row < valid) {
    const float* po = o + (first + row) * C;
    const float* pd = d_o + (first + row) * C;
    for (int c = sub * 4; c < C; c += 16) {
      const float4 a = *reinterpret_cast<const float4*>(po + c);
      const float4 b = *reinterpret_cast<const float4*>(pd + c);
      d += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
    }
  }
  d += __shfl_xor(d, 1, 64);
  d += __shfl_xor(d, 2, 64);
  return d;
}

// Thread tid fills entry tid of St from row first + tid of stats[N * L][4]; entries >= count get (0, 1, 0), which keeps
// exp(s - m) / l finite where it is computed and then dropped.  (The caller decides which threads call.)
__device__ __forceinline__ void load_stats(float* St, const float* __restrict__ stats, size_t first, int count) {
  const int j = threadIdx.x;
  float m = 0.f, l = 1.f, d = 0.f;
  if (j < count) { const float* st = stats + (first + j) * 4; m = st[0]; l = st[1]; d = st[2]; }
  St[j] = m; St[kKB + j] = l; St[2 * kKB + j] = d;
}

// tile[row][col] = exp(scale * acc - m) / l over the wave's 64 columns; zero for rows >= rows_valid and columns >= cols_valid.
// kRowStats: m, l belong to the tile's ROWS (dQ), else to its COLUMNS (dK / dV)
template <bool kRowStats>
__device__ __forceinline__ void acc_to_probs(const f32x16 (&acc)[2][2], float* Ps, const float* St, int Lk, int rows_valid, int cols_valid,
                                             float scale) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5, kb = wave * 64;
  if (kb < Lk) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(a, r, lh), col = acc_col(kb, b, li);
          const int s = kRowStats ? row : col;
          float pv = 0.f;
          if (row < rows_valid && col < cols_valid) pv = __expf(acc[a][b][r] * scale - St[s]) / St[kKB + s];
          Ps[row * kLDP + col] = pv;
        }
  }
}

// tile[row][col] *= acc - D over the wave's 64 columns (columns < Lp)
template <bool kRowStats>
__device__ __forceinline__ void probs_to_ds(const f32x16 (&acc)[2][2], float* Ps, const float* St, int Lk, int Lp) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5, kb = wave * 64;
  if (kb < Lk) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(a, r, lh), col = acc_col(kb, b, li);
          if (col < Lp) Ps[row * kLDP + col] *= (acc[a][b][r] - St[2 * kKB + (kRowStats ? row : col)]);
        }
  }
}

// ---- backward A: dQ (and the per-row softmax statistics + D for kernel B) ----
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                         const float* __restrict__ d_o, float* __restrict__ dqkv,
                                                         float* __restrict__ stats, int N, int L, int C, float scale) {
  SSDE_LDS(smem);
  float* Ps = smem;                       // [64][260]
  float* Qs = smem + kTileFloats;         // staging
  float* Ks = Qs + kQB * kLDC;
  float* Vs = Qs;
  float* St = smem + kTileFloats + kStageFloats;   // [3][256]: only D of the block's 64 rows (P comes from the softmax below)
  const int n = blockIdx.y, q0 = blockIdx.x * kQB, tid = threadIdx.x;
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * L * C3;
  const int Lk = (L + 63) & ~63, Lp = (L + 31) & ~31;
  const int valid = L - q0;

  f32x16 acc[2][2];
  gemm_nt(base + (size_t)q0 * C3, valid, C3, base + C, L, C3, C, Lk, Qs, Ks, acc);
  __syncthreads();
  acc_to_tile(acc, Ps, Lk, scale);
  __syncthreads();
  float m, l;
  softmax_rows(Ps, L, m, l);
  const float d = row_dot(o, d_o, (size_t)n * L + q0, C, valid);
  if ((tid & 3) == 0) {
    const int row = tid >> 2;
    St[2 * kKB + row] = d;
    if (row < valid) {
      float* st = stats + ((size_t)n * L + q0 + row) * 4;
      st[0] = m; st[1] = l; st[2] = d; st[3] = 0.f;
    }
  }
  // dP = dO V^T
  gemm_nt(d_o + ((size_t)n * L + q0) * C, valid, C, base + 2 * C, L, C3, C, Lk, Qs, Ks, acc);
  __syncthreads();
  probs_to_ds<true>(acc, Ps, St, Lk, Lp);   // dS = P o (dP - D), in place over P
  // dQ = scale * dS K
  gemm_pv(Ps, Lp, base + C, L, C3, C, Vs, dqkv + ((size_t)n * L + q0) * C3, C3, valid, scale);
}

// ---- backward B: dK, dV for 64 key rows ----
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                          float* __restrict__ dqkv, const float* __restrict__ stats,
                                                          int N, int L, int C, float scale) {
  SSDE_LDS(smem);
  float* Ps = smem;                       // [64 keys][260 queries]
  float* Qs = smem + kTileFloats;
  float* Ks = Qs + kQB * kLDC;
  float* Vs = Qs;
  float* St = smem + kTileFloats + kStageFloats;   // [3][256]: m, l, D per query
  const int n = blockIdx.y, k0 = blockIdx.x * kQB;
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * L * C3;
  const int Lk = (L + 63) & ~63, Lp = (L + 31) & ~31;
  const int valid = L - k0;
  load_stats(St, stats, (size_t)n * L, L);

  f32x16 acc[2][2];
  // S^T = K_tile Q^T
  gemm_nt(base + (size_t)k0 * C3 + C, valid, C3, base, L, C3, C, Lk, Qs, Ks, acc);
  __syncthreads();
  // P^T[key, query] = exp(scale * s - m_q) / l_q ; rows (keys) >= valid and columns (queries) >= L are zero
  acc_to_probs<false>(acc, Ps, St, Lk, valid, L, scale);
  __syncthreads();
  // dV = P^T dO
  gemm_pv(Ps, Lp, d_o + (size_t)n * L * C, L, C, C, Vs, dqkv + ((size_t)n * L + k0) * C3 + 2 * C, C3, valid, 1.0f);
  // dP^T = V_tile dO^T
  gemm_nt(base + (size_t)k0 * C3 + 2 * C, valid, C3, d_o + (size_t)n * L * C, L, C, C, Lk, Qs, Ks, acc);
  __syncthreads();
  probs_to_ds<false>(acc, Ps, St, Lk, Lp);   // dS^T = P^T o (dP^T - D)
  // dK = scale * dS^T Q
  gemm_pv(Ps, Lp, base, L, C3, C, Vs, dqkv + ((size_t)n * L + k0) * C3 + C, C3, valid, scale);
}

// ---- more than 256 tokens: streaming kernels (ABI 13, added without a layout change) ---------------------------------------------------------------------------
// The kernels above hold a whole 64 x L score tile in LDS, which is what stops them at L = 256.  The kernels below are built from
// the same pieces (gemm_nt, pv_pass, the tile epilogues, the online softmax), but the tile is a WINDOW of at most 256 keys
// (forward, dQ) or 256 queries (dK / dV) that walks the other axis in a fixed order, and the output stays in the accumulator
// registers across the windows (4 waves x 64 channels: 64 accumulator VGPRs per 256 channels).  Nothing of size L^2 reaches HBM,
// there are no atomics, and two runs agree to the bit.
//   forward   attn_stream_kernel<NCP>: per key block S = Q K_blk^T -> tile; online softmax (running row max m and row sum l,
//             P_blk = exp(S - m_new) left unnormalised); O *= exp(m_old - m_new); O += P_blk V_blk; at the end O /= l, once.
//             NCP = channel passes of 256 (1: C <= 256, 2: C <= 512) = accumulator sets held by a wave.
//   backward  attn_stream_stats_kernel: m, l by the same online pass (no P V) and D = sum_c dO O, into stats[N, L, 4];
//             attn_stream_bwd_q_kernel<NCP>: per key block P = exp(S - m) / l, dP = dO V_blk^T, dS = P o (dP - D), dQ += dS K_blk;
//             attn_stream_bwd_kv_kernel: per query block P^T, dV += P^T dO_blk, dS^T, dK += dS^T Q_blk for one 256-channel pass of
//             the outputs (blockIdx.z: at C = 512 the two passes of a key block each recompute S^T and dP^T rather than hold
//             256 accumulator registers of dK and dV beside the 64 of the running product).
// Rows / keys past L: gemm_nt and pv_pass clamp their addresses and zero what they fetched, the softmax reads the valid columns
// only and zeroes the tile up to the next multiple of 32, and no row >= L is stored.
constexpr int kStreamCMax = 512;                            // two 256-channel passes held in registers (the widest attention of a shipped config)
constexpr int kStreamVch = 16;                              // V tokens per chunk of the streaming forward (one workgroup per CU: 290 registers)
constexpr int kStreamLdsFloats = kQB * kLDP + kStreamVch * kLDP + kQB;   // forward / statistics: tile | V chunk | one float per row (83 KB)

template <int NCP>
__global__ __launch_bounds__(256) void attn_stream_kernel(const float* __restrict__ qkv, float* __restrict__ dst,
                                                          int N, int L, int C, float scale) {
  SSDE_LDS(smem);
  float* Qs = smem;                       // [64][36]    (inside the tile: dead once S sits in the accumulators)
  float* Ks = smem + kQB * kLDC;          // [256][36]
  float* Ps = smem;                       // [64][260]
  float* Vs = smem + kQB * kLDP;          // [kStreamVch][260]
  float* Rs = Vs + kStreamVch * kLDP;     // [64] per-row factor
  const int n = blockIdx.y, q0 = blockIdx.x * kQB, tid = threadIdx.x;
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * L * C3;
  const int valid = L - q0;

  f32x16 o[NCP][2][2];
#pragma unroll
  for (int p = 0; p < NCP; ++p) zero_acc(o[p]);
  float m_run = -INFINITY, l_run = 0.f;   // of row tid >> 2 (held by its 4 lanes)
  for (int kb0 = 0; kb0 < L; kb0 += kKB) {
    const int Lb = min(kKB, L - kb0);
    const int Lk = (Lb + 63) & ~63, Lp = (Lb + 31) & ~31;
    f32x16 acc[2][2];
    gemm_nt(base + (size_t)q0 * C3, valid, C3, base + (size_t)kb0 * C3 + C, Lb, C3, C, Lk, Qs, Ks, acc);
    __syncthreads();
    acc_to_tile(acc, Ps, Lk, scale);
    __syncthreads();
    const float alpha = online_softmax<true>(Ps, Lb, m_run, l_run);
    if ((tid & 3) == 0) Rs[tid >> 2] = alpha;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NCP; ++p) {
      if (p * 256 < C) {
        scale_rows(o[p], Rs);
        pv_pass<kStreamVch>(Ps, Lp, base + (size_t)kb0 * C3 + 2 * C, Lb, C3, p * 256, min(256, C - p * 256), Vs, o[p]);
      }
    }
    // (the next window's gemm_nt opens with a barrier before it writes the staging inside the tile; Rs is next written
    // behind three more)
  }
  __syncthreads();
  if ((tid & 3) == 0) Rs[tid >> 2] = 1.0f / l_run;
  __syncthreads();
#pragma unroll
  for (int p = 0; p < NCP; ++p) {
    if (p * 256 < C) {
      scale_rows(o[p], Rs);
      store_acc(o[p], dst + ((size_t)n * L + q0) * C, C, valid, p * 256, C, 1.0f);
    }
  }
}

// ---- streaming backward 1: row max, row sum and D per query row ----
__global__ __launch_bounds__(256) void attn_stream_stats_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                const float* __restrict__ d_o, float* __restrict__ stats,
                                                                int N, int L, int C, float scale) {
  SSDE_LDS(smem);
  float* Qs = smem;
  float* Ks = smem + kQB * kLDC;
  float* Ps = smem;
  const int n = blockIdx.y, q0 = blockIdx.x * kQB, tid = threadIdx.x;
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * L * C3;
  const int valid = L - q0;
  float m_run = -INFINITY, l_run = 0.f;
  for (int kb0 = 0; kb0 < L; kb0 += kKB) {
    const int Lb = min(kKB, L - kb0);
    const int Lk = (Lb + 63) & ~63;
    f32x16 acc[2][2];
    gemm_nt(base + (size_t)q0 * C3, valid, C3, base + (size_t)kb0 * C3 + C, Lb, C3, C, Lk, Qs, Ks, acc);
    __syncthreads();
    acc_to_tile(acc, Ps, Lk, scale);
    __syncthreads();
    online_softmax<false>(Ps, Lb, m_run, l_run);
  }
  const float d = row_dot(o, d_o, (size_t)n * L + q0, C, valid);
  const int row = tid >> 2;
  if ((tid & 3) == 0 && row < valid) {
    float* st = stats + ((size_t)n * L + q0 + row) * 4;
    st[0] = m_run; st[1] = l_run; st[2] = d; st[3] = 0.f;
  }
}

// ---- streaming backward 2: dQ for 64 query rows ----
template <int NCP>
__global__ __launch_bounds__(256) void attn_stream_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                                float* __restrict__ dqkv, const float* __restrict__ stats,
                                                                int N, int L, int C, float scale) {
  SSDE_LDS(smem);
  float* Ps = smem;                       // [64 queries][260 keys]
  float* Qs = smem + kTileFloats;         // staging
  float* Ks = Qs + kQB * kLDC;
  float* Vs = Qs;
  float* St = smem + kTileFloats + kStageFloats;   // [3][256]: m, l, D of the block's 64 rows (the first 64 of each)
  const int n = blockIdx.y, q0 = blockIdx.x * kQB, tid = threadIdx.x;
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * L * C3;
  const int valid = L - q0;
  if (tid < kQB) load_stats(St, stats, (size_t)n * L + q0, valid);
  f32x16 dq[NCP][2][2];
#pragma unroll
  for (int p = 0; p < NCP; ++p) zero_acc(dq[p]);
  for (int kb0 = 0; kb0 < L; kb0 += kKB) {
    const int Lb = min(kKB, L - kb0);
    const int Lk = (Lb + 63) & ~63, Lp = (Lb + 31) & ~31;
    f32x16 acc[2][2];
    gemm_nt(base + (size_t)q0 * C3, valid, C3, base + (size_t)kb0 * C3 + C, Lb, C3, C, Lk, Qs, Ks, acc);
    __syncthreads();                      // (also: the previous window's dS has been read, St is written)
    acc_to_probs<true>(acc, Ps, St, Lk, valid, Lb, scale);
    // dP = dO V_blk^T
    gemm_nt(d_o + ((size_t)n * L + q0) * C, valid, C, base + (size_t)kb0 * C3 + 2 * C, Lb, C3, C, Lk, Qs, Ks, acc);
    __syncthreads();
    probs_to_ds<true>(acc, Ps, St, Lk, Lp);
    // dQ += dS K_blk   (scale applied once, at the store)
#pragma unroll
    for (int p = 0; p < NCP; ++p)
      if (p * 256 < C) pv_pass<32>(Ps, Lp, base + (size_t)kb0 * C3 + C, Lb, C3, p * 256, min(256, C - p * 256), Vs, dq[p]);
  }
#pragma unroll
  for (int p = 0; p < NCP; ++p)
    if (p * 256 < C) store_acc(dq[p], dqkv + ((size_t)n * L + q0) * C3, C3, valid, p * 256, C, scale);
}

// ---- streaming backward 3: dK, dV for 64 key rows and one 256-channel pass of the outputs ----
__global__ __launch_bounds__(256) void attn_stream_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                                 float* __restrict__ dqkv, const float* __restrict__ stats,
                                                                 int N, int L, int C, float scale) {
  SSDE_LDS(smem);
  float* Ps = smem;                       // [64 keys][260 queries]
  float* Qs = smem + kTileFloats;
  float* Ks = Qs + kQB * kLDC;
  float* Vs = Qs;
  float* St = smem + kTileFloats + kStageFloats;   // [3][256]: m, l, D of the window's queries
  const int n = blockIdx.y, k0 = blockIdx.x * kQB;
  const int cp = blockIdx.z * 256, Cw = min(256, C - cp);
  const int C3 = 3 * C;
  const float* base = qkv + (size_t)n * L * C3;
  const float* dob = d_o + (size_t)n * L * C;
  const int valid = L - k0;
  f32x16 dv[2][2], dk[2][2];
  zero_acc(dv);
  zero_acc(dk);
  for (int qb0 = 0; qb0 < L; qb0 += kKB) {
    const int Lb = min(kKB, L - qb0);
    const int Lk = (Lb + 63) & ~63, Lp = (Lb + 31) & ~31;
    __syncthreads();                      // the previous window's readers of St and of the tile are done
    load_stats(St, stats, (size_t)n * L + qb0, Lb);
    f32x16 acc[2][2];
    // S^T = K_tile Q_blk^T
    gemm_nt(base + (size_t)k0 * C3 + C, valid, C3, base + (size_t)qb0 * C3, Lb, C3, C, Lk, Qs, Ks, acc);
    __syncthreads();
    acc_to_probs<false>(acc, Ps, St, Lk, valid, Lb, scale);
    // dV += P^T dO_blk
    pv_pass<32>(Ps, Lp, dob + (size_t)qb0 * C, Lb, C, cp, Cw, Vs, dv);
    // dP^T = V_tile dO_blk^T
    gemm_nt(base + (size_t)k0 * C3 + 2 * C, valid, C3, dob + (size_t)qb0 * C, Lb, C, C, Lk, Qs, Ks, acc);
    __syncthreads();
    probs_to_ds<false>(acc, Ps, St, Lk, Lp);
    // dK += dS^T Q_blk
    pv_pass<32>(Ps, Lp, base + (size_t)qb0 * C3, Lb, C3, cp, Cw, Vs, dk);
  }
  float* out = dqkv + ((size_t)n * L + k0) * C3;
  store_acc(dv, out + 2 * C, C3, valid, cp, C, 1.0f);
  store_acc(dk, out + C, C3, valid, cp, C, scale);
}

// what both entry points ask of a launch's sizes
int check_shape(const char* what, int n, int l, int c) {
  SSDE_REQUIRE(n > 0 && l > 0 && l <= SSDE_ATTN_L_MAX, "%s: token count %d outside 1..%d", what, l, SSDE_ATTN_L_MAX);
  SSDE_REQUIRE(c > 0 && c % 32 == 0, "%s: channels must be a multiple of 32 (got %d)", what, c);
  return SSDE_OK;
}

}  // namespace

// The route of a forward launch (the plan query ssde_attention_route): no device access
static int attn_route(const ssde_attn_args* a) {
  SSDE_REQUIRE(a, "attention: null args");
  if (int rc = check_shape("attention", a->n, a->l, a->c)) return rc;
  if (a->l > kLMax || (a->flags & SSDE_ATTNF_STREAM)) {
    SSDE_REQUIRE(a->c <= kStreamCMax, "attention: the streaming kernels (more than %d tokens, or SSDE_ATTNF_STREAM) take at most %d channels (got %d)",
                 kLMax, kStreamCMax, a->c);
    return SSDE_ATTN_ROUTE_STREAM;
  }
  if ((a->flags & SSDE_ATTNF_BF16X6) && a->l == x6::kL && a->c <= 256 && a->c % 64 == 0) return SSDE_ATTN_ROUTE_X6;
  return SSDE_ATTN_ROUTE_F32;
}

extern "C" int ssde_attention_route(const ssde_attn_args* a) { return attn_route(a); }

extern "C" int ssde_attention(const ssde_attn_args* a, void* stream) {
  SSDE_REQUIRE(a && a->qkv && a->dst, "attention: null args");
  const int route = attn_route(a);
  if (route < 0) return route;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(ssde_cdiv(a->l, kQB), a->n);
  if (route == SSDE_ATTN_ROUTE_STREAM) {
    if (a->c <= 256) return ssde_launch_lds<attn_stream_kernel<1>>("attention", grid, 256, kStreamLdsFloats * 4, st, a->qkv, a->dst, a->n, a->l, a->c, a->scale);
    return ssde_launch_lds<attn_stream_kernel<2>>("attention", grid, 256, kStreamLdsFloats * 4, st, a->qkv, a->dst, a->n, a->l, a->c, a->scale);
  }
  if (route == SSDE_ATTN_ROUTE_X6) {
    const dim3 grid_x6(ssde_cdiv(a->n, 8) * 8 * 4);
    switch (a->c) {
      case 64: return ssde_launch_lds<attn_x6_kernel<4>>("attention", grid_x6, x6::kT, x6::kLds, st, a->qkv, a->dst, a->n, a->scale);
      case 128: return ssde_launch_lds<attn_x6_kernel<8>>("attention", grid_x6, x6::kT, x6::kLds, st, a->qkv, a->dst, a->n, a->scale);
      case 192: return ssde_launch_lds<attn_x6_kernel<12>>("attention", grid_x6, x6::kT, x6::kLds, st, a->qkv, a->dst, a->n, a->scale);
      default: return ssde_launch_lds<attn_x6_kernel<16>>("attention", grid_x6, x6::kT, x6::kLds, st, a->qkv, a->dst, a->n, a->scale);
    }
  }
  return ssde_launch_lds<attn_kernel>("attention", grid, 256, kAttnLdsFloats * 4, st, a->qkv, a->dst, a->n, a->l, a->c, a->scale);
}

extern "C" int ssde_attention_bwd(const ssde_attn_bwd_args* a, void* stream) {
  SSDE_REQUIRE(a && a->qkv && a->o && a->d_o && a->dqkv && a->stats, "attention_bwd: null args");
  if (int rc = check_shape("attention_bwd", a->n, a->l, a->c)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(ssde_cdiv(a->l, kQB), a->n);
  const int lds = kBwdLdsFloats * 4;
  if (a->l > kLMax) {   // (no flag field: the backward routes by the token count alone)
    SSDE_REQUIRE(a->c <= kStreamCMax, "attention_bwd: the streaming kernels (more than %d tokens) take at most %d channels (got %d)", kLMax,
                 kStreamCMax, a->c);
    if (int rc = ssde_launch_lds<attn_stream_stats_kernel>("attention_bwd", grid, 256, kStreamLdsFloats * 4, st, a->qkv, a->o, a->d_o, a->stats, a->n, a->l,
                            a->c, a->scale))
      return rc;
    if (int rc = a->c <= 256 ? ssde_launch_lds<attn_stream_bwd_q_kernel<1>>("attention_bwd", grid, 256, lds, st, a->qkv, a->d_o, a->dqkv, a->stats, a->n, a->l, a->c, a->scale)
                             : ssde_launch_lds<attn_stream_bwd_q_kernel<2>>("attention_bwd", grid, 256, lds, st, a->qkv, a->d_o, a->dqkv, a->stats, a->n, a->l, a->c, a->scale))
      return rc;
    return ssde_launch_lds<attn_stream_bwd_kv_kernel>("attention_bwd", dim3(grid.x, grid.y, ssde_cdiv(a->c, 256)), 256, lds, st, a->qkv, a->d_o, a->dqkv,
                      a->stats, a->n, a->l, a->c, a->scale);
  }
  if (int rc = ssde_launch_lds<attn_bwd_q_kernel>("attention_bwd", grid, 256, lds, st, a->qkv, a->o, a->d_o, a->dqkv, a->stats, a->n, a->l, a->c, a->scale)) return rc;
  return ssde_launch_lds<attn_bwd_kv_kernel>("attention_bwd", grid, 256, lds, st, a->qkv, a->d_o, a->dqkv, a->stats, a->n, a->l, a->c, a->scale);
}
