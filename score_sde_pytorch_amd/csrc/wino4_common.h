// What the F(4x4,3x3) kernels share (conv_wino4.hip, conv_wino4r.hip, conv_wino4p.hip, wino4_xform.hip, wgrad_wino4.hip), once
// each: the transform matrices as code, the map from a workgroup's tiles to pixels, the workgroup epilogue of the two kernels
// that own 32 tiles x 64 couts x 36 positions, and the host steps of their launchers.  DESIGN.md 25.
#pragma once
#include "ssde_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- the matrices ---------------------------------------------------------------------------------------------------
// 1-D input transform (one column / row of B^T d), B^T rows [4,0,-5,0,1,0] [0,-4,-4,1,1,0] [0,4,-4,-1,1,0] [0,-2,-1,2,1,0]
// [0,2,-1,-2,1,0] [0,4,0,-5,0,1]; T = float, or a packed pair ssde_f32x2 (v_pk_*)
template <class T>
__device__ __forceinline__ void bt6(const T (&d)[6], T (&o)[6]) {
  const T t1 = d[4] - 4.f * d[2], t2 = d[3] - 4.f * d[1], t3 = d[4] - d[2], t4 = d[3] - d[1];
  o[0] = 4.f * d[0] - 5.f * d[2] + d[4];
  o[1] = t1 + t2;
  o[2] = t1 - t2;
  o[3] = t3 + 2.f * t4;
  o[4] = t3 - 2.f * t4;
  o[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}
// float2 = two channels, each through the scalar form
template <>
__device__ __forceinline__ void bt6<float2>(const float2 (&d)[6], float2 (&o)[6]) {
  float dx[6], dy[6], ox[6], oy[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) { dx[a] = d[a].x; dy[a] = d[a].y; }
  bt6(dx, ox);
  bt6(dy, oy);
#pragma unroll
  for (int a = 0; a < 6; ++a) o[a] = make_float2(ox[a], oy[a]);
}

// The same matrix for the transform pass (wino4_xform_vq_kernel), in its own arithmetic form.
// The fused multiply-adds are written out and the compiler adds none (as ssde_stat_merge, ssde_common.h): left to -ffp-contract,
// two instantiations of the kernel that differ in their stores alone were contracted differently (1 ulp in 4 % of V on the
// device), and V must be the same bits whichever instantiation a launch takes.
__device__ __forceinline__ void bt6q(const float4 (&d)[6], float4 (&o)[6]) {
#pragma clang fp contract(off)
#define SSDE_BT6_LANE(c)                                                                                             \
  {                                                                                                                  \
    const float t1 = __builtin_fmaf(-4.f, d[2].c, d[4].c), t2 = __builtin_fmaf(-4.f, d[1].c, d[3].c);                 \
    const float t3 = d[4].c - d[2].c, t4 = d[3].c - d[1].c;                                                           \
    o[0].c = __builtin_fmaf(4.f, d[0].c, __builtin_fmaf(-5.f, d[2].c, d[4].c));                                       \
    o[1].c = t1 + t2; o[2].c = t1 - t2; o[3].c = __builtin_fmaf(2.f, t4, t3); o[4].c = __builtin_fmaf(-2.f, t4, t3);  \
    o[5].c = __builtin_fmaf(4.f, d[1].c, __builtin_fmaf(-5.f, d[3].c, d[5].c));                                       \
  }
  SSDE_BT6_LANE(x) SSDE_BT6_LANE(y) SSDE_BT6_LANE(z) SSDE_BT6_LANE(w)
#undef SSDE_BT6_LANE
}

// 1-D transform of the output gradient (weight gradient: Z = A dY A^T), A rows [1,0,0,0] [1,1,1,1] [1,-1,1,-1] [1,2,4,8]
// [1,-2,4,-8] [0,0,0,1]
__device__ __forceinline__ void at6(const float (&d)[4], float (&o)[6]) {
  const float s = d[0] + d[2], t = d[1] + d[3], u = d[0] + 4.f * d[2], v = 2.f * d[1] + 8.f * d[3];
  o[0] = d[0];
  o[1] = s + t;
  o[2] = s - t;
  o[3] = u + v;
  o[4] = u - v;
  o[5] = d[3];
}

// Output transform Y = A^T M A, one column px of the 6x6 products at a time: t = A^T m (A^T rows [1,1,1,1,1,0] [0,1,-1,2,-2,0]
// [0,1,1,4,4,0] [0,1,-1,8,-8,1]), then y[dy][dx] += A[px][dx] t[dy].  T = float (one cout) or float2 (a cout pair)
__device__ __forceinline__ void wino4_at_col(const float (&m)[6], float (&t)[4]) {
  const float s1 = m[1] + m[2], d1 = m[1] - m[2], s2 = m[3] + m[4], d2 = m[3] - m[4];
  t[0] = m[0] + s1 + s2; t[1] = d1 + 2.f * d2; t[2] = s1 + 4.f * s2; t[3] = d1 + 8.f * d2 + m[5];
}
__device__ __forceinline__ void wino4_at_col(const float2 (&m)[6], float2 (&t)[4]) {
  float mx[6], my[6], tx[4], ty[4];
#pragma unroll
  for (int a = 0; a < 6; ++a) { mx[a] = m[a].x; my[a] = m[a].y; }
  wino4_at_col(mx, tx);
  wino4_at_col(my, ty);
#pragma unroll
  for (int a = 0; a < 4; ++a) t[a] = make_float2(tx[a], ty[a]);
}
__device__ __forceinline__ void wino4_axpy(float& y, float k, float t) { y += k * t; }
__device__ __forceinline__ void wino4_axpy(float2& y, float k, const float2& t) { y.x += k * t.x; y.y += k * t.y; }
template <class T>
__device__ __forceinline__ void wino4_out_column(int px, const T (&m)[6], T (&y)[4][4]) {
  // column px of A: (1, 0, 0, 0), (1, 1, 1, 1), (1, -1, 1, -1), (1, 2, 4, 8), (1, -2, 4, -8), (0, 0, 0, 1)
  constexpr float kA[6][4] = {{1.f, 0.f, 0.f, 0.f}, {1.f, 1.f, 1.f, 1.f}, {1.f, -1.f, 1.f, -1.f},
                              {1.f, 2.f, 4.f, 8.f}, {1.f, -2.f, 4.f, -8.f}, {0.f, 0.f, 0.f, 1.f}};
  T t[4];
  wino4_at_col(m, t);
#pragma unroll
  for (int dy = 0; dy < 4; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx)
      if (kA[px][dx] != 0.f) wino4_axpy(y[dy][dx], kA[px][dx], t[dy]);
}

// ---- the parameter fields conv_wino4_kernel and conv_wino4r_kernel share: tiling (ssde_wino_tiling_fill), epilogue
// (ssde_fill_epilogue), split of the reduction ----------------------------------------------------------------------------
struct Wino4Shared {
  int N, H, W, Cout;
  int lTWt, lTHt;          // log2 tiles per patch row / column
  int tiles_x, tiles_per_img, m_tiles, n_tiles;
  const float* bias; const float* chan_add; int chan_add_ld;
  const float* resid; int resid_post;
  float scale;
  float* dst;
  float* gn_part;
  int ksplit;              // 1, 2 or 4 workgroups per tile, each reducing its share of the channel stages (the kernel's kKs)
  unsigned* sync;          // ksplit > 1: this launch's (shares started, shares handed over) pairs, one per tile, from
                           // conv_mfma.hip's g_conv_sync (zero before and after)
  int ticket_off;          // float index of the hand-over ticket in LDS (behind everything else)
  int T, tiles_h, tiles_w; // 4x4 tiles of the whole batch / per image column / per image row
};

// ---- the tile map: workgroup tile mt = 32 tiles of 4x4 pixels, 2^lTWt x 2^lTHt of each of 32 >> (lTWt + lTHt) images -------
struct Wino4TileMap {
  int lTWt, lTHt, N, H, W;
  int img0, trem, ty, tx;  // first image; patch index, row and column inside an image
  __device__ __forceinline__ Wino4TileMap(const Wino4Shared& p, int mt)
      : lTWt(p.lTWt), lTHt(p.lTHt), N(p.N), H(p.H), W(p.W) {
    img0 = (mt / p.tiles_per_img) * (32 >> (lTWt + lTHt));
    trem = mt % p.tiles_per_img;
    ty = trem / p.tiles_x; tx = trem % p.tiles_x;
  }
  // tile of the workgroup -> (image in the workgroup, tile row, tile column)
  __device__ __forceinline__ void decode(int tile, int& il, int& tr, int& tc) const {
    il = tile >> (lTWt + lTHt);
    tr = (tile >> lTWt) & ((1 << lTHt) - 1); tc = tile & ((1 << lTWt) - 1);
  }
  // row of the parked [256 px][64 couts] tile of epilogue round rnd -> pixel of dst; false: outside the batch / the image
  __device__ __forceinline__ bool pixel(int rnd, int row, size_t& pix, int& img) const {
    const int tile = rnd * 16 + (row >> 4), dy = (row >> 2) & 3, dx = row & 3;
    int il, tr, tc;
    decode(tile, il, tr, tc);
    img = img0 + il;
    const int oy = ((ty << lTHt) + tr) * 4 + dy, ox = ((tx << lTWt) + tc) * 4 + dx;
    if (img >= N || oy >= H || ox >= W) return false;
    pix = ((size_t)img * H + oy) * W + ox;
    return true;
  }
};
// (the callable ssde_store_tile asks for)
struct Wino4RoundPixels {
  const Wino4TileMap& tm; int rnd;
  __device__ __forceinline__ bool operator()(int row, size_t& pix, int& img) const { return tm.pixel(rnd, row, pix, img); }
};

// ---- the workgroup epilogue -----------------------------------------------------------------------------------------
// 8 waves hold 72 accumulator blocks of 32 tiles x 32 couts: all 36 positions x two cout halves of 32 tiles x 64 couts.  16 tiles
// (= accumulator rows r < 8, then r >= 8 of every wave) at a time: the products of a round go to LDS as M[pos][tile 16][64 couts]
// (pitch kW4Ldm), every thread applies A^T M A to one (tile, cout pair), parks the 4x4 outputs as [256 pixels][64 couts] (pitch
// kW4Ldt, aliasing the products) and the shared epilogue stores them (ssde_store_tile: bias, temb addend, residual, scale,
// GroupNorm partials).  All waves take part in both rounds and each round retires half of a wave's accumulators, so nothing
// spills.  (Rounds over the two 32-cout halves instead kept 144 accumulators live through the transform of the other half: 81
// scratch stores per lane and 105 k cycles of epilogue per workgroup, tools/wino4_trace.py.)
// Split reduction (kKs > 1; `ks` = this workgroup's share, `sy` = the tile's slot pair): share 0 leaves its raw 4x4 outputs in the
// tile's own part of dst, shares 1 .. kKs - 2 add theirs to them in turn, the last share adds its own and runs the epilogue.  The
// sums travel as agent-scope 16-byte accesses, coherent at the device level by themselves (no __threadfence(): that is a
// write-back of the whole L2 per workgroup, conv_mfma.hip; as dword atomics the hand-over was 64 loads and 64 stores per thread
// and share).
constexpr int kW4Threads = 512, kW4Blocks = 9;
constexpr int kW4Ldm = 66;                          // row pitch of the product exchange [pos][16 tiles][64 couts]
constexpr int kW4Ldt = 68;                          // row pitch of the parked output tile [256 pixels][64 couts]
constexpr int kW4EpiLds = 36 * 16 * kW4Ldm * 4;     // bytes of the exchange (the parked tile fits inside)
static_assert(256 * kW4Ldt <= 36 * 16 * kW4Ldm, "parked tile");

// what the epilogue reports to a kernel's trace hook (Tr::stamp(phase, round); the default does nothing)
enum Wino4EpiPhase {
  kW4ProductsWritten, kW4ProductsThere, kW4Transformed, kW4ProductsRead, kW4ParkWritten, kW4Parked, kW4PrevShareThere, kW4SumsFormed,
  kW4Signalled, kW4Stored, kW4RoundDone, kW4Done
};
struct Wino4EpiNoTrace {
  __device__ __forceinline__ void stamp(int, int) const {}
};

// Tr (a kernel's traits, by reference: a trace build keeps its state there) says
//   position(wave, j), half(wave, j)   which (transform position, cout half) accumulator block j of a wave is
//   barrier()                          the barrier between the exchange phases
//   lane_index(tid, li, lh)            lane & 31, lane >> 5 -- the values are the same, the registers they cost are not
//   stamp(phase, rnd)                  trace hook
template <int kKs, class Tr>
__device__ __forceinline__ void wino4_epilogue(f32x16 (&acc)[kW4Blocks], float* smem, const Wino4Shared& p, const Wino4TileMap& tm,
                                               int wave, int nt, int ks, unsigned* sy, const Tr& tr) {
  constexpr bool kSplit = kKs > 1;
  const int tid = threadIdx.x;
  const int IMGS = 32 >> (p.lTWt + p.lTHt);
  const int n0 = nt * 64;
  SsdeEpi e{p.bias, p.chan_add, p.chan_add_ld, p.resid, p.resid_post, p.scale, p.dst, p.Cout, p.gn_part};
  // GroupNorm partials: one entry per (image, workgroup tile, round) when the tile is part of one image; per image when a
  // round holds IMGS / 2 whole images (IMGS >= 2: 16 / (tiles per image) images per round)
  const int gn_base = !p.gn_part ? -1 : (IMGS == 1 ? (tm.img0 * p.tiles_per_img + tm.trem) * 2 : tm.img0);
  const int rpi_log2 = IMGS > 2 ? 8 - (4 - p.lTWt - p.lTHt) : 30;             // rows per image in a round: 256 / (IMGS / 2)
  const int gn_max = IMGS == 1 ? p.N * p.tiles_per_img * 2 : p.N;
  int li, lh;
  Tr::lane_index(tid, li, lh);
  const int e_tl = tid >> 5, e_cp = tid & 31;                                 // this thread's (tile of the round, cout pair)
  float* park = smem;                                                         // [256][kW4Ldt], aliases the products
#pragma unroll
  for (int rnd = 0; rnd < 2; ++rnd) {
    const Wino4RoundPixels pixfn{tm, rnd};
#pragma unroll
    for (int j = 0; j < kW4Blocks; ++j)
#pragma unroll
      for (int r8 = 0; r8 < 8; ++r8) {
        const int r = rnd * 8 + r8;
        const int tl = (r & 3) + 4 * lh + 8 * ((r >> 2) & 1);
        smem[(Tr::position(wave, j) * 16 + tl) * kW4Ldm + Tr::half(wave, j) * 32 + li] = acc[j][r];
      }
    tr.stamp(kW4ProductsWritten, rnd);
    Tr::barrier();
    tr.stamp(kW4ProductsThere, rnd);
    float2 y[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) y[a][b] = make_float2(0.f, 0.f);
    const float* mp = smem + e_tl * kW4Ldm + 2 * e_cp;
#pragma unroll
    for (int px = 0; px < 6; ++px) {
      float2 m[6];
#pragma unroll
      for (int py = 0; py < 6; ++py) m[py] = *reinterpret_cast<const float2*>(mp + (py * 6 + px) * (16 * kW4Ldm));
      wino4_out_column(px, m, y);
    }
    tr.stamp(kW4Transformed, rnd);
    Tr::barrier();                             // every thread has read its products: the parked tile may overwrite them
    tr.stamp(kW4ProductsRead, rnd);
#pragma unroll
    for (int dy = 0; dy < 4; ++dy)
#pragma unroll
      for (int dx = 0; dx < 4; ++dx)
        *reinterpret_cast<float2*>(park + (e_tl * 16 + dy * 4 + dx) * kW4Ldt + 2 * e_cp) = y[dy][dx];
    tr.stamp(kW4ParkWritten, rnd);
    Tr::barrier();
    tr.stamp(kW4Parked, rnd);                  // the store phase starts
    const int gn_entry = gn_base < 0 ? -1 : (IMGS == 1 ? gn_base + rnd : gn_base + rnd * (IMGS >> 1));
    if constexpr (kSplit) {
      const bool first = ks == 0, last = ks == kKs - 1;
      // sy[1] counts the shares that have handed over, round 0 in its low half and round 1 in its high half -- share k starts
      // adding to round 0 while share k - 1 is still busy with its round 1
      if (!first) {
        if (tid == 0)
          while (((__hip_atomic_load(sy + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (16 * rnd)) & 0xffffu) != (unsigned)ks)
            __builtin_amdgcn_s_sleep(4);
        __syncthreads();
      }
      tr.stamp(kW4PrevShareThere, rnd);
      constexpr int kIters = 256 * 16 / kW4Threads, kBatch = 4;      // (4 float4 of a thread at a time: round 0 still holds half of the accumulators)
      static_assert(kBatch == 4, "SSDE_WAIT_VMCNT_FOR4");
#pragma unroll
      for (int ib = 0; ib < kIters; ib += kBatch) {
        float* tp[kBatch];
        float* dp[kBatch];
#pragma unroll
        for (int it = 0; it < kBatch; ++it) {
          const int q = tid + (ib + it) * kW4Threads;
          const int row = q >> 4, j = (q & 15) * 4;
          size_t pix; int img;
          const bool ok = pixfn(row, pix, img) && n0 + j < p.Cout;       // c_out % 4 == 0 on this path
          tp[it] = park + row * kW4Ldt + j;
          dp[it] = ok ? p.dst + pix * p.Cout + n0 + j : nullptr;
        }
        ssde_f32x4 o[kBatch];
        if (!first) {
#pragma unroll
          for (int it = 0; it < kBatch; ++it) SSDE_GLOAD16_AGENT(o[it], dp[it] ? dp[it] : p.dst);     // the batch's loads in flight before the first add
          SSDE_WAIT_VMCNT_FOR4(0, o[0], o[1], o[2], o[3]);
#pragma unroll
          for (int it = 0; it < kBatch; ++it) o[it] += *reinterpret_cast<const ssde_f32x4*>(tp[it]);   // (sum so far) + own share
        } else {
#pragma unroll
          for (int it = 0; it < kBatch; ++it) o[it] = *reinterpret_cast<const ssde_f32x4*>(tp[it]);
        }
        if (last) {
#pragma unroll
          for (int it = 0; it < kBatch; ++it) *reinterpret_cast<ssde_f32x4*>(tp[it]) = o[it];
        } else {
#pragma unroll
          for (int it = 0; it < kBatch; ++it)
            if (dp[it]) SSDE_GSTORE16_AGENT(dp[it], o[it]);
        }
      }
      tr.stamp(kW4SumsFormed, rnd);            // handed on, or parked for the epilogue
      if (!last) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0);      // every store of this thread is acknowledged ...
        __syncthreads();                    // ... and every thread's (and park may be refilled by round 1)
        if (tid == 0) atomicAdd(sy + 1, rnd == 0 ? 1u : 0x10000u);
        tr.stamp(kW4Signalled, rnd);
        if (rnd == 0) continue;
        return;
      }
      __syncthreads();
      if (rnd == 1 && tid == 0) { sy[0] = 0u; sy[1] = 0u; }              // ready for the next launch that is dealt these slots
    }
    // round 1 has no accumulators left: all 8 rows of a thread (residual loads) in flight instead of 4.
    // (Fetching the residual rows ahead of the exchange / transform / park phases was built twice and measured neutral:
    //  profiles/r6_w4r_epilogue_prefetch_v1_in_scratch_rejected.txt, r6_w4r_epilogue_prefetch_v2_neutral.txt)
    if (rnd == 0) ssde_store_tile<256, 64, kW4Threads, 4, 0>(park, kW4Ldt, n0, e, pixfn, gn_entry, rpi_log2, gn_max);
    else ssde_store_tile<256, 64, kW4Threads, 8, 0>(park, kW4Ldt, n0, e, pixfn, gn_entry, rpi_log2, gn_max);
    tr.stamp(kW4Stored, rnd);
    if (rnd == 0) { Tr::barrier(); tr.stamp(kW4RoundDone, rnd); }
  }
  tr.stamp(kW4Done, 0);
}

// ---- host side --------------------------------------------------------------------------------------------------------
// what every F(4x4,3x3) forward route asks of a launch's shape; `route` prefixes the messages, min_edge = 8: maps below 8x8 are
// refused (0: the position-batched route takes them)
static inline int wino4_check_shape(const ssde_conv_args* a, const char* route, int min_edge) {
  SSDE_REQUIRE(a && a->dst && a->main.p0 && a->w_main, "%s: null args", route);
  SSDE_REQUIRE(a->ksize == 3 && a->stride == 1 && a->pad == 1, "%s: needs 3x3, stride 1, pad 1", route);
  SSDE_REQUIRE(a->aux.p0 == nullptr, "%s: fused 1x1 source not supported (issue it as a second conv)", route);
  const bool same = a->h_in == a->h_out && a->w_in == a->w_out && a->h_out % 4 == 0 && a->w_out % 4 == 0;
  if (min_edge > 0)
    SSDE_REQUIRE(same && a->h_out >= min_edge && a->w_out >= min_edge, "%s: same-size output, multiples of 4, at least %dx%d (got %dx%d)",
                 route, min_edge, min_edge, a->h_out, a->w_out);
  else
    SSDE_REQUIRE(a->n > 0 && same && a->h_out > 0 && a->w_out > 0, "%s: same-size output, multiples of 4 (got %dx%d)", route, a->h_out, a->w_out);
  return SSDE_OK;
}

// The fields of Wino4Shared that follow from the shape, and the GroupNorm slices of the launch (0: this tiling cannot write
// partials).  A workgroup tile is part of one image (two epilogue rounds: 2 x tiles_per_img slices of 8 wave entries) or holds
// `imgs` >= 2 whole images (imgs / 2 per round; 512 / imgs rows per image >= the 32 rows of one epilogue trip)
static inline int wino4_fill_shared(Wino4Shared& p, const ssde_conv_args* a, const char* route, ssde_wino_tiling* t, int* gn_slices) {
  p.N = a->n; p.H = a->h_out; p.W = a->w_out; p.Cout = a->c_out;
  *t = ssde_wino_tiling_fill(p, a, 4, 32);
  ssde_fill_epilogue(p, a);
  p.tiles_h = a->h_out / 4; p.tiles_w = a->w_out / 4; p.T = a->n * p.tiles_h * p.tiles_w;
  SSDE_REQUIRE(!a->gn_part || t->gn_ok, "%s: GroupNorm partials not available for this tiling", route);
  *gn_slices = t->gn_ok ? (t->imgs == 1 ? 2 * p.tiles_per_img : 1) * (kW4Threads / 64) : 0;
  return SSDE_OK;
}

// Split the reduction when the launch would leave half of the CUs or more without a workgroup (8x8 maps at batch 256: 128 tiles
// of 8 images x 64 couts); splits_fn = the route's own rule.  dst is the hand-over buffer: not when the residual aliases it; and
// not without hand-over slots.  Returns the workgroups of the launch.
static inline int wino4_split_setup(Wino4Shared& p, const ssde_conv_args* a, int (*splits_fn)(int, int, int, unsigned)) {
  const int wgs = ssde_cdiv(p.m_tiles, 8) * 8 * p.n_tiles;
  p.ksplit = a->resid != a->dst ? splits_fn(wgs, a->main.c0 + a->main.c1, a->c_out, a->flags) : 1;
  p.sync = p.ksplit > 1 ? ssde_conv_sync_slots(p.m_tiles * p.n_tiles) : nullptr;
  if (!p.sync) p.ksplit = 1;
  return wgs * p.ksplit;
}

// ksplit -> the instantiation: K1, K2, K4 = the kernel for 1, 2, 4 shares
template <auto K1, auto K2, auto K4, class P>
static inline int wino4_launch_split(const char* route, const P& p, int wgs, int lds, hipStream_t st) {
  const dim3 grid(wgs), block(kW4Threads);
  switch (p.ksplit) {
    case 4: return ssde_launch_lds<K4>(route, grid, block, lds, st, p);
    case 2: return ssde_launch_lds<K2>(route, grid, block, lds, st, p);
    default: return ssde_launch_lds<K1>(route, grid, block, lds, st, p);
  }
}
