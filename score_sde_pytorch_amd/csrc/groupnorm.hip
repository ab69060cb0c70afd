// GroupNorm statistics (mean, rstd per (sample, group)) for NHWC fp32 tensors.
// Reference: nn.GroupNorm(num_groups=min(C//4, 32), eps=1e-6) as used at
// models/layerspp.py:67,219,231 and models/ncsnpp.py:194-227.  Only the reduction
// lives here; normalise + affine (+ SiLU) is fused into the consumer's LDS staging
// (conv_mfma.hip, resample.hip), so the normalised tensor never touches HBM -- except for group widths that are no multiple
// of 4, which no consumer's prologue accepts: those run through ssde_gn_apply / ssde_gn_apply_bwd at the end of this file.
//
// HBM-bound: every element is read exactly once with 16-byte lane loads; a wave
// covers 256 consecutive channels of a pixel run.  Sums are accumulated relative
// to a per-group pivot (the group's first element) so E[(x-K)^2] - E[x-K]^2 does
// not cancel catastrophically; lanes are combined with wave64 shuffles.
#include "ssde_common.h"

namespace {

constexpr int kGnThreads = 1024;

struct GnParams {
  const float* p0; const float* p1; int c0, c1;
  int n, hw, groups, slices; float eps;
  float* mean; float* rstd; float* scratch;
};

// grid = (slices, n).  Thread (pl, cl): channel float4 `cl`, pixels pl, pl+PL, ...
__global__ __launch_bounds__(kGnThreads) void gn_stats_kernel(const GnParams p) {
  SSDE_LDS(smem);
  float* s_sum = smem;
  float* s_sq = smem + kGnThreads;
  const int n = blockIdx.y, slice = blockIdx.x;
  const int C = p.c0 + p.c1;
  const int CL = C >> 2;                 // float4 lanes per pixel
  const int PL = kGnThreads / CL;        // pixel lanes
  const int tid = threadIdx.x;
  const int cpg = C / p.groups;
  const int px_per_slice = (p.hw + p.slices - 1) / p.slices;
  const int px0 = slice * px_per_slice;
  const int px1 = min(p.hw, px0 + px_per_slice);

  float sum = 0.f, sq = 0.f;
  if (tid < CL * PL) {
    const int cl = tid % CL, pl = tid / CL;
    const int ch = cl * 4;
    const float* base; int Cs, cc;
    if (ch < p.c0) { base = p.p0; Cs = p.c0; cc = ch; } else { base = p.p1; Cs = p.c1; cc = ch - p.c0; }
    // pivot: first element (pixel 0) of this lane's group
    const int g = ch / cpg;
    const int gch = g * cpg;
    const float pivot = (gch < p.c0) ? p.p0[(size_t)n * p.hw * p.c0 + gch]
                                     : p.p1[(size_t)n * p.hw * p.c1 + (gch - p.c0)];
    const float* src = base + (size_t)n * p.hw * Cs + cc;
    int px = px0 + pl;
    // 4 independent loads in flight per lane
    for (; px + 3 * PL < px1; px += 4 * PL) {
      const float4 a = *reinterpret_cast<const float4*>(src + (size_t)px * Cs);
      const float4 b = *reinterpret_cast<const float4*>(src + (size_t)(px + PL) * Cs);
      const float4 c = *reinterpret_cast<const float4*>(src + (size_t)(px + 2 * PL) * Cs);
      const float4 d = *reinterpret_cast<const float4*>(src + (size_t)(px + 3 * PL) * Cs);
      const float4 v[4] = {a, b, c, d};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x0 = v[k].x - pivot, x1 = v[k].y - pivot, x2 = v[k].z - pivot, x3 = v[k].w - pivot;
        sum += (x0 + x1) + (x2 + x3);
        sq += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
      }
    }
    for (; px < px1; px += PL) {
      const float4 a = *reinterpret_cast<const float4*>(src + (size_t)px * Cs);
      const float x0 = a.x - pivot, x1 = a.y - pivot, x2 = a.z - pivot, x3 = a.w - pivot;
      sum += (x0 + x1) + (x2 + x3);
      sq += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
    }
  }
  s_sum[tid] = sum;
  s_sq[tid] = sq;
  __syncthreads();
  // one thread per group gathers its (cpg/4) x PL lanes in a fixed order (deterministic)
  if (tid < p.groups) {
    const int g = tid;
    const int l0 = g * (cpg >> 2), l1 = l0 + (cpg >> 2);
    float S = 0.f, Q = 0.f;
    for (int pl = 0; pl < PL; ++pl)
      for (int cl = l0; cl < l1; ++cl) { S += s_sum[pl * CL + cl]; Q += s_sq[pl * CL + cl]; }
    if (p.slices == 1) {
      const int gch = g * cpg;
      const float pivot = (gch < p.c0) ? p.p0[(size_t)n * p.hw * p.c0 + gch]
                                       : p.p1[(size_t)n * p.hw * p.c1 + (gch - p.c0)];
      const float cnt = (float)cpg * (float)p.hw;
      const float m = S / cnt;
      float var = Q / cnt - m * m;
      var = var < 0.f ? 0.f : var;
      p.mean[n * p.groups + g] = pivot + m;
      p.rstd[n * p.groups + g] = 1.0f / sqrtf(var + p.eps);
    } else {
      float* o = p.scratch + (((size_t)n * p.slices + slice) * p.groups + g) * 2;
      o[0] = S; o[1] = Q;
    }
  }
}

// slices > 1: combine the per-slice partial sums (same pivot in every slice).
__global__ void gn_finalize_kernel(const GnParams p) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.n * p.groups) return;
  const int n = idx / p.groups, g = idx % p.groups;
  const int C = p.c0 + p.c1, cpg = C / p.groups;
  float S = 0.f, Q = 0.f;
  for (int s = 0; s < p.slices; ++s) {
    const float* o = p.scratch + (((size_t)n * p.slices + s) * p.groups + g) * 2;
    S += o[0]; Q += o[1];
  }
  const int gch = g * cpg;
  const float pivot = (gch < p.c0) ? p.p0[(size_t)n * p.hw * p.c0 + gch]
                                   : p.p1[(size_t)n * p.hw * p.c1 + (gch - p.c0)];
  const float cnt = (float)cpg * (float)p.hw;
  const float m = S / cnt;
  float var = Q / cnt - m * m;
  var = var < 0.f ? 0.f : var;
  p.mean[idx] = pivot + m;
  p.rstd[idx] = 1.0f / sqrtf(var + p.eps);
}

// Statistics from the producers' partials (ssde_store_tile): a team of 16 lanes per (image, group), ssde_gn_merge16
// (ssde_common.h) -- 16 (image, group) pairs per workgroup.  (Until round 6: one wave per pair, most of its lanes idle behind 16
// to 64 entries and two more shuffle rounds in the chain.)
struct GnFinParams {
  const float* part0; const float* part1;
  int c0, c1, s0, s1, n, groups; float eps;
  float* mean; float* rstd;
};
__global__ __launch_bounds__(256) void gn_part_finalize_kernel(const GnFinParams p) {
  const int idx = blockIdx.x * 16 + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
  const int tot = p.n * p.groups;
  const int pair = idx < tot ? idx : tot - 1;          // (whole waves run the shuffles: a pair beyond the end repeats the last one)
  const int n = pair / p.groups, g = pair - n * p.groups;
  float cnt, m, M2;
  ssde_gn_merge16(p.part0, p.part1, p.c0, p.c1, p.s0, p.s1, p.groups, n, g, l16, cnt, m, M2);
  if (l16 == 0 && idx < tot) {
    p.mean[idx] = m;
    p.rstd[idx] = ssde_gn_rstd(cnt, M2, p.eps);
  }
}

// The same merge for groups with MANY entries (SSDE_GN_TEAM_MAX_ENTRIES: the 128x128 / 256x256 levels of FFHQ-256, 1024-4096
// slices per image): one workgroup per (image, group).  Thread t merges the entries t, t + 256, ... in order -- four loads in
// flight at a time --, then the 256 thread results are merged pairwise through LDS, lower index first: a fixed order, so the
// result is deterministic (it is NOT the order of a 16-lane team: such a group is always merged here, by nobody else).
// With teams of 16 these launches were 64-256 dependent loads per lane: 109 launches of an FFHQ-256 evaluation took 3.2 ms
// (round 5's wave per group: 1.4 ms).
__global__ __launch_bounds__(256) void gn_part_finalize_big_kernel(const GnFinParams p) {
  SSDE_LDS(red);                                   // [256][3]
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int n = pair / p.groups, g = pair - n * p.groups;
  SsdeGnTeam t;
  ssde_gn_team_init(t, p.part0, p.part1, p.c0, p.c1, p.s0, p.s1, p.groups, n, g);
  float cnt = 0.f, m = 0.f, M2 = 0.f;
  for (int k0 = tid; k0 < t.etot; k0 += 4 * 256) {
    float v[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 256 * i;
      const float* e = t.entry(k < t.etot ? k : 0);
      v[i][0] = e[0]; v[i][1] = e[1]; v[i][2] = e[2];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k0 + 256 * i < t.etot) ssde_stat_merge(cnt, m, M2, v[i][2], v[i][0], v[i][1]);
  }
  red[tid * 3] = cnt; red[tid * 3 + 1] = m; red[tid * 3 + 2] = M2;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    if ((tid & (2 * o - 1)) == 0) {
      ssde_stat_merge(cnt, m, M2, red[(tid + o) * 3], red[(tid + o) * 3 + 1], red[(tid + o) * 3 + 2]);
      red[tid * 3] = cnt; red[tid * 3 + 1] = m; red[tid * 3 + 2] = M2;
    }
    __syncthreads();
  }
  if (tid == 0) {
    p.mean[pair] = m;
    p.rstd[pair] = ssde_gn_rstd(cnt, M2, p.eps);
  }
}


// ---- any group width (ABI 13) -------------------------------------------------------------------------------------------
// nn.GroupNorm(min(C // 4, 32), C) (layerspp.py:219,231) on the 192 = 128 + 64 channels of a 1024-px decoder level: 32 groups
// of 6.  A lane's four channels then belong to up to two groups (A: the group of its first channel, B: the next one; widths
// >= 4), and a group may straddle p0 / p1.  Same grid, same lane map, same pivoted sums and the same fixed gather order as
// gn_stats_kernel: on a multiple of 4 every lane's B sums are zero and the result has the quad kernel's bits.
__global__ __launch_bounds__(kGnThreads) void gn_stats_any_kernel(const GnParams p) {
  SSDE_LDS(smem);                          // [4][kGnThreads]: sum A, sq A, sum B, sq B
  float* s_sum = smem;
  float* s_sq = smem + kGnThreads;
  float* s_sumb = smem + 2 * kGnThreads;
  float* s_sqb = smem + 3 * kGnThreads;
  const int n = blockIdx.y, slice = blockIdx.x;
  const int C = p.c0 + p.c1;
  const int CL = C >> 2;
  const int PL = kGnThreads / CL;
  const int tid = threadIdx.x;
  const int cpg = C / p.groups;
  const int px_per_slice = (p.hw + p.slices - 1) / p.slices;
  const int px0 = slice * px_per_slice;
  const int px1 = min(p.hw, px0 + px_per_slice);
  auto pivot_of = [&](int g) {
    const int gch = g * cpg;
    return (gch < p.c0) ? p.p0[(size_t)n * p.hw * p.c0 + gch] : p.p1[(size_t)n * p.hw * p.c1 + (gch - p.c0)];
  };

  float sum = 0.f, sq = 0.f, sumb = 0.f, sqb = 0.f;
  if (tid < CL * PL) {
    const int cl = tid % CL, pl = tid / CL;
    const int ch = cl * 4;
    const float* base; int Cs, cc;
    if (ch < p.c0) { base = p.p0; Cs = p.c0; cc = ch; } else { base = p.p1; Cs = p.c1; cc = ch - p.c0; }
    const int ga = ch / cpg, gb = (ch + 3) / cpg;
    const int split = (ga + 1) * cpg - ch;           // channels ch .. ch + split - 1 are group A's (>= 4: all of them)
    const float pivot = pivot_of(ga), pivotb = pivot_of(gb);
    const bool a1 = split > 1, a2 = split > 2, a3 = split > 3;
    const float* src = base + (size_t)n * p.hw * Cs + cc;
    auto add = [&](const float4& v) {
      const float x0 = v.x - pivot, x1 = a1 ? v.y - pivot : 0.f, x2 = a2 ? v.z - pivot : 0.f, x3 = a3 ? v.w - pivot : 0.f;
      sum += (x0 + x1) + (x2 + x3);
      sq += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
      const float y1 = a1 ? 0.f : v.y - pivotb, y2 = a2 ? 0.f : v.z - pivotb, y3 = a3 ? 0.f : v.w - pivotb;
      sumb += y1 + (y2 + y3);
      sqb += y1 * y1 + (y2 * y2 + y3 * y3);
    };
    int px = px0 + pl;
    for (; px + 3 * PL < px1; px += 4 * PL) {
      const float4 a = *reinterpret_cast<const float4*>(src + (size_t)px * Cs);
      const float4 b = *reinterpret_cast<const float4*>(src + (size_t)(px + PL) * Cs);
      const float4 c = *reinterpret_cast<const float4*>(src + (size_t)(px + 2 * PL) * Cs);
      const float4 d = *reinterpret_cast<const float4*>(src + (size_t)(px + 3 * PL) * Cs);
      add(a); add(b); add(c); add(d);
    }
    for (; px < px1; px += PL) add(*reinterpret_cast<const float4*>(src + (size_t)px * Cs));
  }
  s_sum[tid] = sum; s_sq[tid] = sq; s_sumb[tid] = sumb; s_sqb[tid] = sqb;
  __syncthreads();
  // one thread per group gathers the lanes that hold its channels in a fixed order: pixel lanes outside, channel lanes inside
  if (tid < p.groups) {
    const int g = tid;
    const int l0 = (g * cpg) >> 2, l1 = ((g + 1) * cpg + 3) >> 2;
    float S = 0.f, Q = 0.f;
    for (int pl = 0; pl < PL; ++pl)
      for (int cl = l0; cl < l1; ++cl) {
        const bool is_a = 4 * cl >= g * cpg;         // the lane's first channel is this group's: its A sums; else its B sums
        S += is_a ? s_sum[pl * CL + cl] : s_sumb[pl * CL + cl];
        Q += is_a ? s_sq[pl * CL + cl] : s_sqb[pl * CL + cl];
      }
    if (p.slices == 1) {
      const float pivot = pivot_of(g);
      const float cnt = (float)cpg * (float)p.hw;
      const float m = S / cnt;
      float var = Q / cnt - m * m;
      var = var < 0.f ? 0.f : var;
      p.mean[n * p.groups + g] = pivot + m;
      p.rstd[n * p.groups + g] = 1.0f / sqrtf(var + p.eps);
    } else {
      float* o = p.scratch + (((size_t)n * p.slices + slice) * p.groups + g) * 2;
      o[0] = S; o[1] = Q;
    }
  }
}

// ---- GroupNorm as a launch of its own: dst = drop(act(gamma (x - mean) rstd + beta)) ------------------------------------
// The consumers' prologue (ssde_pro_apply) materialised, for the group widths they refuse and for the activations they do not
// know (ssde_src.act: the kernels below are instantiated per SSDE_ACT_*, the SiLU instance is the code of ABI 13's first form;
// SSDE_PRO_SILU is the activation alone, with neither statistics nor affine).  grid = (pixel runs, n), thread
// (pl, cl) as in the statistics kernels: a thread keeps ONE channel quad for all its pixels, so the statistics of its four
// channels' groups -- read from a per-workgroup LDS table, one division per channel and workgroup -- gamma and beta live in
// registers, and the loop is a 16-byte load, the arithmetic and a 16-byte store: one read and one write of the tensor.
struct GnApplyParams {
  ssde_src s; int n, hw, px_per_wg; float* dst;
  const float* dy; float* sums; float* g0; float* g1; int acc0, acc1;       // backward apply only
  float* scratch; int slices;                                                    // backward reduce only
};
struct GnQuad { float4 mu, rs, gam, bet; const float* src; int Cs; };

// table [2][C] (mean, rstd of every channel's group in image n), then this thread's quad
__device__ __forceinline__ void gn_quad_table(const GnApplyParams& p, float* tab, int n, int C) {
  if (p.s.pro_mode != SSDE_PRO_GN && p.s.pro_mode != SSDE_PRO_GN_SILU) return;   // a plain copy of the concatenation, or the activation alone: no statistics
  const int cpg = C / p.s.gn_groups;
  for (int c = threadIdx.x; c < C; c += kGnThreads) {
    const int g = c / cpg;
    tab[c] = p.s.gn_mean[n * p.s.gn_groups + g];
    tab[C + c] = p.s.gn_rstd[n * p.s.gn_groups + g];
  }
}
__device__ __forceinline__ GnQuad gn_quad_load(const GnApplyParams& p, const float* tab, int n, int C, int ch) {
  GnQuad q;
  q.mu = q.rs = q.gam = q.bet = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.s.pro_mode == SSDE_PRO_GN || p.s.pro_mode == SSDE_PRO_GN_SILU) {
    q.mu = *reinterpret_cast<const float4*>(tab + ch);
    q.rs = *reinterpret_cast<const float4*>(tab + C + ch);
    q.gam = *reinterpret_cast<const float4*>(p.s.gn_gamma + ch);
    q.bet = *reinterpret_cast<const float4*>(p.s.gn_beta + ch);
  }
  if (ch < p.s.c0) { q.Cs = p.s.c0; q.src = p.s.p0 + (size_t)n * p.hw * p.s.c0 + ch; }
  else { q.Cs = p.s.c1; q.src = p.s.p1 + (size_t)n * p.hw * p.s.c1 + (ch - p.s.c0); }
  return q;
}

template <int ACT>
__global__ __launch_bounds__(kGnThreads) void gn_apply_kernel(const GnApplyParams p) {
  SSDE_LDS(tab);
  const int n = blockIdx.y, tid = threadIdx.x;
  const int C = p.s.c0 + p.s.c1, CL = C >> 2, PL = kGnThreads / CL;
  gn_quad_table(p, tab, n, C);
  __syncthreads();
  if (tid >= CL * PL) return;
  const int cl = tid % CL, pl = tid / CL, ch = cl * 4;
  const GnQuad q = gn_quad_load(p, tab, n, C, ch);
  const SsdePro pro = ssde_pro_decode(p.s);
  const int px0 = blockIdx.x * p.px_per_wg, px1 = min(p.hw, px0 + p.px_per_wg);
  float* dst = p.dst + (size_t)n * p.hw * C + ch;
  auto one = [&](float4 v, int px) {
    if (pro.gn) {
      v.x = (v.x - q.mu.x) * q.rs.x * q.gam.x + q.bet.x;
      v.y = (v.y - q.mu.y) * q.rs.y * q.gam.y + q.bet.y;
      v.z = (v.z - q.mu.z) * q.rs.z * q.gam.z + q.bet.z;
      v.w = (v.w - q.mu.w) * q.rs.w * q.gam.w + q.bet.w;
    }
    if (pro.silu) { v.x = ssde_act<ACT>(v.x); v.y = ssde_act<ACT>(v.y); v.z = ssde_act<ACT>(v.z); v.w = ssde_act<ACT>(v.w); }
    if (__builtin_expect(pro.drop, 0)) {
      const uint32_t e0 = ((uint32_t)n * (uint32_t)p.hw + (uint32_t)px) * (uint32_t)C + (uint32_t)ch;
      v.x *= ssde_keep(e0, pro); v.y *= ssde_keep(e0 + 1u, pro); v.z *= ssde_keep(e0 + 2u, pro); v.w *= ssde_keep(e0 + 3u, pro);
    }
    *reinterpret_cast<float4*>(dst + (size_t)px * C) = v;
  };
  int px = px0 + pl;
  for (; px + 3 * PL < px1; px += 4 * PL) {          // 4 independent loads in flight per lane
    const float4 a = *reinterpret_cast<const float4*>(q.src + (size_t)px * q.Cs);
    const float4 b = *reinterpret_cast<const float4*>(q.src + (size_t)(px + PL) * q.Cs);
    const float4 c = *reinterpret_cast<const float4*>(q.src + (size_t)(px + 2 * PL) * q.Cs);
    const float4 d = *reinterpret_cast<const float4*>(q.src + (size_t)(px + 3 * PL) * q.Cs);
    one(a, px); one(b, px + PL); one(c, px + 2 * PL); one(d, px + 3 * PL);
  }
  for (; px < px1; px += PL) one(*reinterpret_cast<const float4*>(q.src + (size_t)px * q.Cs), px);
}

// ---- its adjoint ------------------------------------------------------------------------------------------------------
// du = dy * mask * act'(u) and xhat of one quad of one pixel (act' and the mask recomputed, as in backward.hip); without a
// GroupNorm (SSDE_PRO_SILU) u is x itself and xhat is not used
template <int ACT>
__device__ __forceinline__ void gn_quad_du(const GnApplyParams& p, const GnQuad& q, const SsdePro& pro, const float4& x, const float4& dy,
                                           int n, int px, int C, int ch, float (&xh)[4], float (&du)[4]) {
  const float xv[4] = {x.x, x.y, x.z, x.w}, dv[4] = {dy.x, dy.y, dy.z, dy.w};
  const float mu[4] = {q.mu.x, q.mu.y, q.mu.z, q.mu.w}, rs[4] = {q.rs.x, q.rs.y, q.rs.z, q.rs.w};
  const float gm[4] = {q.gam.x, q.gam.y, q.gam.z, q.gam.w}, bt[4] = {q.bet.x, q.bet.y, q.bet.z, q.bet.w};
  const uint32_t e0 = ((uint32_t)n * (uint32_t)p.hw + (uint32_t)px) * (uint32_t)C + (uint32_t)ch;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    xh[k] = (xv[k] - mu[k]) * rs[k];
    float d = dv[k];
    if (pro.silu) d *= ssde_act_grad<ACT>(pro.gn ? xh[k] * gm[k] + bt[k] : xv[k]);
    if (__builtin_expect(pro.drop, 0)) d *= ssde_keep(e0 + (uint32_t)k, pro);
    du[k] = d;
  }
}

// launch 1: per (image, pixel slice, channel) the sums of du and du * xhat -> scratch [n][slices][C][2]; grid = (slices, n)
template <int ACT>
__global__ __launch_bounds__(kGnThreads) void gn_apply_bwd_reduce_kernel(const GnApplyParams p) {
  SSDE_LDS(smem);                                    // [8][kGnThreads] lane sums, then the table [2][C]
  const int n = blockIdx.y, slice = blockIdx.x, tid = threadIdx.x;
  const int C = p.s.c0 + p.s.c1, CL = C >> 2, PL = kGnThreads / CL;
  float* tab = smem + 8 * kGnThreads;
  gn_quad_table(p, tab, n, C);
  __syncthreads();
  float db[4] = {0.f, 0.f, 0.f, 0.f}, dg[4] = {0.f, 0.f, 0.f, 0.f};
  if (tid < CL * PL) {
    const int cl = tid % CL, pl = tid / CL, ch = cl * 4;
    const GnQuad q = gn_quad_load(p, tab, n, C, ch);
    const SsdePro pro = ssde_pro_decode(p.s);
    const int pps = (p.hw + p.slices - 1) / p.slices;
    const int px0 = slice * pps, px1 = min(p.hw, px0 + pps);
    const float* dy = p.dy + (size_t)n * p.hw * C + ch;
    for (int px = px0 + pl; px < px1; px += PL) {
      const float4 x = *reinterpret_cast<const float4*>(q.src + (size_t)px * q.Cs);
      const float4 d = *reinterpret_cast<const float4*>(dy + (size_t)px * C);
      float xh[4], du[4];
      gn_quad_du<ACT>(p, q, pro, x, d, n, px, C, ch, xh, du);
#pragma unroll
      for (int k = 0; k < 4; ++k) { db[k] += du[k]; dg[k] += du[k] * xh[k]; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { smem[k * kGnThreads + tid] = db[k]; smem[(4 + k) * kGnThreads + tid] = dg[k]; }
  __syncthreads();
  // one thread per channel adds its pixel lanes in order (deterministic)
  for (int c = tid; c < C; c += kGnThreads) {
    const int cl = c >> 2, k = c & 3;
    float B = 0.f, G = 0.f;
    for (int pl = 0; pl < PL; ++pl) { B += smem[k * kGnThreads + pl * CL + cl]; G += smem[(4 + k) * kGnThreads + pl * CL + cl]; }
    float* o = p.scratch + (((size_t)n * p.slices + slice) * C + c) * 2;
    o[0] = B; o[1] = G;
  }
}

// launch 2: one workgroup per result.  Blocks [0, n G): (image, group) -> sums = mean_g(dxh), mean_g(dxh * xhat) with
// dxh = du * gamma, over the group's channels and the slices; blocks [n G, n G + C): channel -> dbeta, dgamma over images
// and slices.  Thread t adds the entries t, t + 256, ... in order, then a pairwise tree through LDS, lower index first.
__global__ __launch_bounds__(256) void gn_apply_bwd_finish_kernel(const GnApplyParams p) {
  SSDE_LDS(red);                                     // [256][2]
  const int tid = threadIdx.x, G = p.s.gn_groups, C = p.s.c0 + p.s.c1, cpg = C / G;
  const int item = blockIdx.x;
  float a = 0.f, b = 0.f;
  if (item < p.n * G) {
    const int n = item / G, g = item - n * G;
    for (int e = tid; e < p.slices * cpg; e += 256) {
      const int sl = e / cpg, c = g * cpg + (e - sl * cpg);
      const float* o = p.scratch + (((size_t)n * p.slices + sl) * C + c) * 2;
      const float gm = p.s.gn_gamma[c];
      a += o[0] * gm; b += o[1] * gm;
    }
  } else {
    const int c = item - p.n * G;
    for (int e = tid; e < p.n * p.slices; e += 256) {
      const float* o = p.scratch + ((size_t)e * C + c) * 2;
      a += o[0]; b += o[1];
    }
  }
  red[tid * 2] = a; red[tid * 2 + 1] = b;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    if ((tid & (2 * o - 1)) == 0) {
      a += red[(tid + o) * 2]; b += red[(tid + o) * 2 + 1];
      red[tid * 2] = a; red[tid * 2 + 1] = b;
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (item < p.n * G) {
      const float cnt = (float)cpg * (float)p.hw;
      float* o = p.sums + (size_t)item * 2;
      o[0] = a / cnt; o[1] = b / cnt;
    } else {
      // (dbeta / dgamma ride in g0 / g1 of this launch's parameter copy)
      p.g0[item - p.n * G] = a; p.g1[item - p.n * G] = b;
    }
  }
}

// launch 3: dx = rstd * (dxh - mean_g(dxh) - xhat * mean_g(dxh * xhat)) into the gradients of p0 / p1; grid = (pixel runs, n).
// SSDE_PRO_SILU (no GroupNorm): dx = du, the only launch of the adjoint
template <int ACT>
__global__ __launch_bounds__(kGnThreads) void gn_apply_bwd_apply_kernel(const GnApplyParams p) {
  SSDE_LDS(tab);                                     // [2][C] mean, rstd, then [2][C] the group sums of every channel
  const int n = blockIdx.y, tid = threadIdx.x;
  const bool has_gn = p.s.pro_mode == SSDE_PRO_GN || p.s.pro_mode == SSDE_PRO_GN_SILU;
  const int C = p.s.c0 + p.s.c1, CL = C >> 2, PL = kGnThreads / CL, cpg = has_gn ? C / p.s.gn_groups : C;
  gn_quad_table(p, tab, n, C);
  for (int c = tid; c < C; c += kGnThreads) {
    const int g = c / cpg;
    tab[2 * C + c] = has_gn ? p.sums[((size_t)n * p.s.gn_groups + g) * 2] : 0.f;
    tab[3 * C + c] = has_gn ? p.sums[((size_t)n * p.s.gn_groups + g) * 2 + 1] : 0.f;
  }
  __syncthreads();
  if (tid >= CL * PL) return;
  const int cl = tid % CL, pl = tid / CL, ch = cl * 4;
  const GnQuad q = gn_quad_load(p, tab, n, C, ch);
  const float4 sa4 = *reinterpret_cast<const float4*>(tab + 2 * C + ch), sb4 = *reinterpret_cast<const float4*>(tab + 3 * C + ch);
  const float sa[4] = {sa4.x, sa4.y, sa4.z, sa4.w}, sb[4] = {sb4.x, sb4.y, sb4.z, sb4.w};
  const float gm[4] = {q.gam.x, q.gam.y, q.gam.z, q.gam.w}, rs[4] = {q.rs.x, q.rs.y, q.rs.z, q.rs.w};
  const SsdePro pro = ssde_pro_decode(p.s);
  const int px0 = blockIdx.x * p.px_per_wg, px1 = min(p.hw, px0 + p.px_per_wg);
  const float* dy = p.dy + (size_t)n * p.hw * C + ch;
  float* g; int acc;
  if (ch < p.s.c0) { g = p.g0 ? p.g0 + (size_t)n * p.hw * p.s.c0 + ch : nullptr; acc = p.acc0; }
  else { g = p.g1 ? p.g1 + (size_t)n * p.hw * p.s.c1 + (ch - p.s.c0) : nullptr; acc = p.acc1; }
  if (!g) return;
  for (int px = px0 + pl; px < px1; px += PL) {
    const float4 x = *reinterpret_cast<const float4*>(q.src + (size_t)px * q.Cs);
    const float4 d = *reinterpret_cast<const float4*>(dy + (size_t)px * C);
    float xh[4], du[4], r[4];
    gn_quad_du<ACT>(p, q, pro, x, d, n, px, C, ch, xh, du);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = pro.gn ? rs[k] * (du[k] * gm[k] - sa[k] - xh[k] * sb[k]) : du[k];
    float4* o = reinterpret_cast<float4*>(g + (size_t)px * q.Cs);
    float4 v = make_float4(r[0], r[1], r[2], r[3]);
    if (acc) { const float4 t = *o; v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
    *o = v;
  }
}

}  // namespace

extern "C" int ssde_gn_finalize(const ssde_gn_finalize_args* a, void* stream) {
  SSDE_REQUIRE(a && a->part0 && a->mean && a->rstd, "gn_finalize: null args");
  const int C = a->c0 + a->c1;
  SSDE_REQUIRE(a->c0 > 0 && a->c0 % 4 == 0 && a->c1 % 4 == 0 && (a->c1 == 0 || a->part1), "gn_finalize: bad channel counts");
  SSDE_REQUIRE(a->groups > 0 && C % a->groups == 0 && (C / a->groups) % 4 == 0, "gn_finalize: channels-per-group must be a multiple of 4");
  SSDE_REQUIRE(a->n > 0 && a->slices0 > 0 && (a->c1 == 0 || a->slices1 > 0), "gn_finalize: bad shape");
  GnFinParams p{a->part0, a->part1, a->c0, a->c1, a->slices0, a->slices1, a->n, a->groups, a->eps, a->mean, a->rstd};
  if (ssde_gn_group_is_big(a->c0, a->c1, a->slices0, a->slices1, a->groups))
    hipLaunchKernelGGL(gn_part_finalize_big_kernel, dim3(a->n * a->groups), dim3(256), 256 * 3 * sizeof(float), static_cast<hipStream_t>(stream), p);
  else
    hipLaunchKernelGGL(gn_part_finalize_kernel, dim3(ssde_cdiv(a->n * a->groups, 16)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_groupnorm_stats(const ssde_gn_stats_args* a, void* stream) {
  SSDE_REQUIRE(a && a->p0 && a->mean && a->rstd, "gn_stats: null args");
  const int C = a->c0 + a->c1;
  SSDE_REQUIRE(a->c0 % 4 == 0 && a->c1 % 4 == 0 && C > 0 && C <= 4 * kGnThreads, "gn_stats: bad channel count %d", C);
  SSDE_REQUIRE(a->c1 == 0 || a->p1, "gn_stats: second tensor missing");
  SSDE_REQUIRE(a->groups > 0 && a->groups <= kGnThreads && C % a->groups == 0 && C / a->groups >= 4,
               "gn_stats: channels-per-group must be a whole number >= 4 (C=%d G=%d)", C, a->groups);
  const bool any = (C / a->groups) % 4 != 0 || (a->flags & SSDE_GNSTATF_ANY_WIDTH);
  SSDE_REQUIRE(a->n > 0 && a->hw > 0, "gn_stats: bad shape");
  int slices = a->slices > 0 ? a->slices : 1;
  SSDE_REQUIRE(slices == 1 || a->scratch, "gn_stats: scratch needed for slices > 1");
  GnParams p{a->p0, a->p1, a->c0, a->c1, a->n, a->hw, a->groups, slices, a->eps, a->mean, a->rstd, a->scratch};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (any) hipLaunchKernelGGL(gn_stats_any_kernel, dim3(slices, a->n), dim3(kGnThreads), 4 * kGnThreads * sizeof(float), st, p);
  else hipLaunchKernelGGL(gn_stats_kernel, dim3(slices, a->n), dim3(kGnThreads), 2 * kGnThreads * sizeof(float), st, p);
  SSDE_LAUNCH_CHECK();
  if (slices > 1) {
    const int tot = a->n * a->groups;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(ssde_cdiv(tot, 256)), dim3(256), 0, st, p);
    SSDE_LAUNCH_CHECK();
  }
  return SSDE_OK;
}

static int gn_apply_check(const ssde_src& s, int n, int hw, bool copy_ok, const char* what) {
  const int C = s.c0 + s.c1;
  const bool gn = s.pro_mode == SSDE_PRO_GN || s.pro_mode == SSDE_PRO_GN_SILU;
  SSDE_REQUIRE(gn || s.pro_mode == SSDE_PRO_SILU || (copy_ok && s.pro_mode == SSDE_PRO_NONE), "%s: prologue mode %d is not handled", what, s.pro_mode);
  SSDE_REQUIRE(s.act >= SSDE_ACT_SILU && s.act <= SSDE_ACT_LRELU, "%s: activation %d (src.act) is none of SSDE_ACT_*", what, s.act);
  SSDE_REQUIRE(s.p0 && (!gn || (s.gn_mean && s.gn_rstd && s.gn_gamma && s.gn_beta)), "%s: null args", what);
  SSDE_REQUIRE(s.c0 > 0 && s.c0 % 4 == 0 && s.c1 >= 0 && s.c1 % 4 == 0 && C <= 4 * kGnThreads, "%s: bad channel counts %d + %d", what, s.c0, s.c1);
  SSDE_REQUIRE(s.c1 == 0 || s.p1, "%s: second tensor missing", what);
  SSDE_REQUIRE(!gn || (s.gn_groups > 0 && C % s.gn_groups == 0), "%s: %d channels in %d groups", what, C, s.gn_groups);
  SSDE_REQUIRE(s.drop_thresh == 0u || s.drop_seed, "%s: dropout without a seed word", what);
  SSDE_REQUIRE(n > 0 && n <= 65535 && hw > 0, "%s: bad shape", what);
  return SSDE_OK;
}
// pixels per workgroup of the two apply kernels: four per lane, at most 65535 runs
static int gn_apply_px_per_wg(int C, int hw) {
  const int PL = kGnThreads / (C >> 2);
  int px = 4 * PL;
  while (ssde_cdiv(hw, px) > 65535) px *= 2;
  return px;
}
// the instantiation of a kernel template for src.act (checked by gn_apply_check: one of SSDE_ACT_*)
#define GN_LAUNCH_ACT(kernel, act, ...)                                                          \
  switch (act) {                                                                                 \
    case SSDE_ACT_ELU: hipLaunchKernelGGL(kernel<SSDE_ACT_ELU>, __VA_ARGS__); break;             \
    case SSDE_ACT_RELU: hipLaunchKernelGGL(kernel<SSDE_ACT_RELU>, __VA_ARGS__); break;           \
    case SSDE_ACT_LRELU: hipLaunchKernelGGL(kernel<SSDE_ACT_LRELU>, __VA_ARGS__); break;         \
    default: hipLaunchKernelGGL(kernel<SSDE_ACT_SILU>, __VA_ARGS__); break;                      \
  }

extern "C" int ssde_gn_apply(const ssde_gn_apply_args* a, void* stream) {
  SSDE_REQUIRE(a && a->dst, "gn_apply: null args");
  if (int rc = gn_apply_check(a->src, a->n, a->hw, true, "gn_apply")) return rc;
  const int C = a->src.c0 + a->src.c1;
  GnApplyParams p{};
  p.s = a->src; p.n = a->n; p.hw = a->hw; p.dst = a->dst;
  p.px_per_wg = gn_apply_px_per_wg(C, a->hw);
  GN_LAUNCH_ACT(gn_apply_kernel, a->src.act, dim3(ssde_cdiv(a->hw, p.px_per_wg), a->n), dim3(kGnThreads), 2 * C * sizeof(float),
                static_cast<hipStream_t>(stream), p);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_gn_apply_bwd(const ssde_gn_apply_bwd_args* a, void* stream) {
  SSDE_REQUIRE(a && a->dy, "gn_apply_bwd: null args");
  if (int rc = gn_apply_check(a->src, a->n, a->hw, false, "gn_apply_bwd")) return rc;
  const bool act_only = a->src.pro_mode == SSDE_PRO_SILU;
  SSDE_REQUIRE(act_only || (a->sums && a->scratch), "gn_apply_bwd: null args");
  SSDE_REQUIRE(!act_only || (!a->dgamma && !a->dbeta && (a->g0 || a->g1)), "gn_apply_bwd: SSDE_PRO_SILU has no dgamma / dbeta and needs g0 or g1");
  SSDE_REQUIRE((a->dgamma == nullptr) == (a->dbeta == nullptr), "gn_apply_bwd: dgamma and dbeta go together");
  SSDE_REQUIRE(act_only || (a->slices >= 1 && a->slices <= 65535), "gn_apply_bwd: bad slice count %d", a->slices);
  SSDE_REQUIRE(a->g1 == nullptr || a->src.c1 > 0, "gn_apply_bwd: g1 without a second tensor");
  const int C = a->src.c0 + a->src.c1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  GnApplyParams p{};
  p.s = a->src; p.n = a->n; p.hw = a->hw; p.dy = a->dy; p.sums = a->sums; p.scratch = a->scratch; p.slices = a->slices;
  if (!act_only) {
    GN_LAUNCH_ACT(gn_apply_bwd_reduce_kernel, a->src.act, dim3(a->slices, a->n), dim3(kGnThreads), (8 * kGnThreads + 2 * C) * sizeof(float), st, p);
    SSDE_LAUNCH_CHECK();
    GnApplyParams f = p;
    f.g0 = a->dbeta; f.g1 = a->dgamma;
    hipLaunchKernelGGL(gn_apply_bwd_finish_kernel, dim3(a->n * a->src.gn_groups + (a->dgamma ? C : 0)), dim3(256), 256 * 2 * sizeof(float), st, f);
    SSDE_LAUNCH_CHECK();
  }
  if (a->g0 || a->g1) {
    p.g0 = a->g0; p.g1 = a->g1; p.acc0 = a->acc0; p.acc1 = a->acc1;
    p.px_per_wg = gn_apply_px_per_wg(C, a->hw);
    GN_LAUNCH_ACT(gn_apply_bwd_apply_kernel, a->src.act, dim3(ssde_cdiv(a->hw, p.px_per_wg), a->n), dim3(kGnThreads), 4 * C * sizeof(float), st, p);
    SSDE_LAUNCH_CHECK();
  }
  return SSDE_OK;
}
