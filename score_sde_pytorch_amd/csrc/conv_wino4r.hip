// 3x3 / stride 1 / pad 1 convolution by Winograd F(4x4, 3x3), two-kernel form, matrix kernel fed from REGISTERS.
//
//   wino4_xform_vq_kernel (wino4_xform.hip)   V[pos][Cin/4][t][4] = B^T pro(x) B      HBM-bound pass
//   conv_wino4r_kernel (this file)            Y = A^T [ sum_ci U .* V ] A             no LDS, no barrier in the main loop
//
// Round 4's matrix kernel (conv_wino4g.hip, now tools/experiments/conv_wino4g_lds_fed/) moved both operands through LDS by LDS-DMA and sits at ~3050 cycles per 4-channel
// stage for 2304 matrix cycles.  tools/microbench/fill_path.hip (profiles/r5_fill_path_microbench.txt) separates the causes:
// beside a running fp32 MFMA chain the CU takes 64 KB per stage from L2 at NO cost by either route (LDS-DMA 2376 cycles per
// stage, global_load_dwordx4 into VGPRs 2304 = the matrix bound), so neither the TA, nor the TCP -> LDS write, nor the L2 is the
// 18 B/clk/CU "fill bound" of round 4.  What the product pays for is its lock step: one barrier per stage makes every wave wait
// for the slowest LDS-DMA piece of the stage (V streams from HBM), with the weights fetched only half a stage ahead.  And the
// 36 KB of weights per stage are wave-PRIVATE: the LDS round trip shares them with nobody.
//
// This kernel therefore keeps NOTHING in LDS during the main loop.  A workgroup is 8 waves = 32 tiles x 64 couts x 36 transform
// positions, as in conv_wino4.hip, but the 72 (position, cout half) blocks of 32 x 32 are dealt so that a wave needs as few
// DIFFERENT operand bytes as possible: wave w owns positions 4 w .. 4 w + 3 with BOTH cout halves (two MFMA blocks share one A
// fragment) and one cout half (w & 1) of position 32 + (w >> 1): nine accumulator blocks, 18 MFMAs per 4-channel stage, fed by
//   A: V[pos][stage][tile = lane & 31][2 (lane >> 5) .. + 1]        one global_load_dwordx2 per position: FIVE per stage
//   B: U[pos][cout = (lane & 31), 32 + (lane & 31)][2 (lane >> 5) .. + 1]   packed per LANE (SSDE_PACK_WINO4R): one dwordx4 per
//                                                                   full position + one dwordx2 for the half position
// straight into the registers its v_mfma_f32_32x32x2_f32 read.  (The first version dealt wave (q, h) the positions q + 4 j of cout
// half h: every V run was loaded by two waves, 72 KB per stage and CU -- and the CU's path from L2 saturates at ~28 B/clk when
// every CU pulls at once, tools/microbench/fill_path.hip and profiles/r5_wino4r_simd_pair_balance_ab.txt: ~2500 cycles per stage
// whatever the waves' priorities.  This dealing moves 56 KB.)  A register is re-loaded for stage st + 2 right after the MFMAs
// that consumed it in stage st (two register sets), so every load has two whole stages to land, ~18 loads are in flight per wave
// at any time, and the only synchronisation is the wave's own counted s_waitcnt vmcnt (five per stage).  Waves drift freely: a
// late V piece stalls one wave while its SIMD sibling keeps the matrix pipe busy.  LDS is used by the epilogue only
// (wino4_common.h's wino4_epilogue: products -> LDS, A^T M A, parked tile, shared coalesced store with GroupNorm partials).
#include "wino4_common.h"
#include <type_traits>

// -DSSDE_W4R_TRACE (a variant library only): s_memtime stamps of waves 0 and 7 of the first workgroup
#ifdef SSDE_W4R_TRACE
__device__ unsigned long long* g_w4r_trace;
extern "C" int ssde_debug_w4r_trace(void* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_w4r_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -5;
}
#define SSDE_RT(slot)                                                                                     \
  do {                                                                                                    \
    if (tr_on) g_w4r_trace[tr_base + (slot)] = __builtin_amdgcn_s_memtime();                              \
  } while (0)
#else
#define SSDE_RT(slot) do { } while (0)
#endif

namespace {

constexpr int kNP = 9;                              // accumulator blocks per wave: (4 positions) x (2 cout halves) + 1
constexpr int kNV = 5;                              // positions a wave loads V for
constexpr int kURegion = kNP * 32 * 4;              // floats of a stage's weight image only wave (q, h) reads (4.5 KB)
constexpr int kUFloats = 8 * kURegion;              // one (stage, 64-cout tile) of the image
// 8 waves, 32 tiles x 64 couts, one workgroup per CU (conv_wino4.hip's shape).  A 4-wave form with two workgroups per CU, the
// second one started half a tile late so that one's epilogue would run under the other's MFMAs, was built and measured level:
// the epilogue is VALU / issue work and fp32 MFMAs share the VALU datapath (tools/experiments/conv_wino4r_two_workgroups_per_cu/)
constexpr int kWaves = 8, kThreads = 64 * kWaves, kBN = 64;
constexpr int kLds = kW4EpiLds;                     // the epilogue's product exchange (the parked tile fits inside)
static_assert(kThreads == kW4Threads && kNP == kW4Blocks && kBN == 64, "wino4_epilogue");

struct Wino4rParams : Wino4Shared {
  const float* v;          // [36][Ctot / 4][T][4]
  const float* wpk;        // SSDE_PACK_WINO4R: [Ctot / 4][n_tiles][8 waves][4 positions x [64 lanes][4] | [64 lanes][2]]
  int Ctot;
};

// What wino4_epilogue (wino4_common.h) asks of this kernel
struct Wino4rEpi : Wino4EpiNoTrace {
  // wave w: positions 4 w + i (i = 0..3), both cout halves -> blocks 2 i, 2 i + 1; position 32 + (w >> 1), cout half w & 1 -> block 8
  static __device__ __forceinline__ int position(int wave, int j) { return j < 8 ? 4 * wave + (j >> 1) : 32 + (wave >> 1); }
  static __device__ __forceinline__ int half(int wave, int j) { return j < 8 ? (j & 1) : (wave & 1); }
  // LDS-only barriers throughout: a __syncthreads() would wait out the previous round's global stores
  static __device__ __forceinline__ void barrier() { SSDE_LDS_BARRIER(); }
  // li / lh derived from tid rather than lane: the same values, but from lane hipcc keeps them live across the matrix loop --
  // 240 VGPRs instead of 210
  static __device__ __forceinline__ void lane_index(int tid, int& li, int& lh) { li = tid & 31; lh = (tid >> 5) & 1; }
#ifdef SSDE_W4R_TRACE
  bool tr_on; int tr_base;
  // slots 32 + 4 rnd .. (products written, there, transformed, parked), 40 / 42 / 44 + rnd (split), 4 and 5
  __device__ __forceinline__ void stamp(int phase, int rnd) const {
    constexpr int kSlot[] = {32, 33, 34, -1, -1, 35, 40, 42, 44, -1, 4, 5};
    constexpr int kPerRound[] = {4, 4, 4, 0, 0, 4, 1, 1, 1, 0, 0, 0};
    if (kSlot[phase] >= 0) SSDE_RT(kSlot[phase] + kPerRound[phase] * rnd);
  }
#endif
};

// kKs = 2 or 4: that many workgroups per tile, each reducing its share of the channel stages (conv_wino4.hip's split, the hand-over
// is wino4_common.h's: shares are dealt in the order the workgroups START -- an atomic counter per tile -- so share k only ever waits for
// shares < k, which are resident or done; the sums are formed in the fixed order ((s0 + s1) + s2) + s3).  The maps this is for
// are the 8x8 ones at batch 256: 1024 tiles = 32 workgroup tiles x 4 cout tiles = 128 workgroups on 256 CUs; two shares each
// cover the chip with one workgroup per CU, and the matrix loop of a share is half as long.  (Eight shares on the 4x4 maps -- one
// tile per image -- were built and measured slower than the direct kernel: the hand-over chain outlasts the 8 stages a share
// computes, profiles/r5_wino4r_4x4_maps_eight_shares_rejected.txt, tools/experiments/conv_wino4r_4x4_maps_eight_shares/.)
//
// (A persistent form, one workgroup per CU walking the tiles, was built and measured slower: DESIGN.md 11.6.)
template <int kKs>
__global__ __launch_bounds__(kThreads, 2) void conv_wino4r_kernel(const Wino4rParams p) {
  constexpr bool kSplit = kKs > 1;
  SSDE_LDS(smem);                               // the epilogue's only (+ the split's ticket)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  // wave w: positions 4 w + i (i = 0..3), both cout halves -> blocks 2 i, 2 i + 1; position 32 + (w >> 1), cout half w & 1 -> block 8
  auto pos_of = [&](int i) { return i < 4 ? 4 * wave + i : 32 + (wave >> 1); };
  const int TWt = 1 << p.lTWt, THt = 1 << p.lTHt;
  // ---- operand addresses of a tile.  A: the lane's byte offset of position slot j inside one stage's [36][Q][T][4] view of V
  // (32-bit: the launcher checks V < 4 GB); the stage rides in the scalar base.  Tiles outside the batch / the image read tile 0's
  // run (a valid address; their outputs are never stored).  B: the wave's 4.5 KB of a stage, lane-major; four 1 KB pieces at
  // immediates -2048 .. 1024 around the base and one 512-byte piece behind them
  const size_t v_stage = (size_t)p.T * 16;
  const size_t u_stage = (size_t)p.n_tiles * kUFloats * 4;
  const uint32_t u_off = (uint32_t)lane * 16u, u_off8 = 2048u + (uint32_t)lane * 8u;
  // TWO register sets per operand: stage st lives in set st & 1 and is loaded while stage st - 2 is consumed, so a wave has two
  // whole stages of loads in flight.  (With one set -- the first version -- a stage could not be shorter than one memory
  // latency: ~3000 cycles for a wave alone on its SIMD, profiles/r5_wino4r_v2_two_workgroups_per_cu.txt, against 1152 matrix
  // cycles; two waves per SIMD at 2304 cycles each sat right at that bound.)
  ssde_f32x2 va[2][kNV], u2[2];
  ssde_f32x4 u4[2][4];
  uint32_t v_off[kNV];
  const char* vs = nullptr;
  const char* us = nullptr;
  // the loads of one stage into register set S: V0 U0 | V1 U1 | V2 U2 | V3 U3 | V4 U4 (the order the loop's counted waits assume)
#define SSDE_W4R_ROUND_AT(S, VN, UN)                                                               \
  do {                                                                                             \
    SSDE_GLOAD8_I_SAFE(va[S][0], v_off[0], VN, 0); SSDE_GLOAD16_I_SAFE(u4[S][0], u_off, UN, -2048);          \
    SSDE_GLOAD8_I_SAFE(va[S][1], v_off[1], VN, 0); SSDE_GLOAD16_I_SAFE(u4[S][1], u_off, UN, -1024);          \
    SSDE_GLOAD8_I_SAFE(va[S][2], v_off[2], VN, 0); SSDE_GLOAD16_I_SAFE(u4[S][2], u_off, UN, 0);              \
    SSDE_GLOAD8_I_SAFE(va[S][3], v_off[3], VN, 0); SSDE_GLOAD16_I_SAFE(u4[S][3], u_off, UN, 1024);           \
    SSDE_GLOAD8_I_SAFE(va[S][4], v_off[4], VN, 0); SSDE_GLOAD8_I_SAFE(u2[S], u_off8, UN, 0);                 \
  } while (0)

  // XCD-aware order (conv_wino4.hip): the cout tiles of one pixel tile run on one XCD at the same time -- they read the same V
  const int bid = blockIdx.x;
  const int nt = (bid >> 3) % p.n_tiles;
  const int mt = ((bid >> 3) / (p.n_tiles * kKs)) * 8 + (bid & 7);   // (the kKs workgroups of a tile: same XCD, 8 * n_tiles blocks apart)
#ifdef SSDE_W4R_TRACE
  const bool tr_on = lane == 0 && (wave == 0 || wave == kWaves - 1) && g_w4r_trace != nullptr && bid == (int)g_w4r_trace[255];   // (the host names the workgroup)
  const int tr_base = (wave == 0 ? 0 : 1) * 128;
#endif
  SSDE_RT(0);
  if (mt >= p.m_tiles) return;                   // (the grid is padded to whole groups of 8 pixel tiles)

  const Wino4TileMap tm(p, mt);
  const int img0 = tm.img0, ty = tm.ty, tx = tm.tx;
  // this workgroup's share of the reduction: stages st_off .. st_off + nst (an even count: the launcher splits only channel
  // counts that are multiples of 8 kKs)
  int nst = p.Ctot >> 2, ks = 0, st_off = 0;
  unsigned* sy = kSplit ? p.sync + 2 * ((size_t)mt * p.n_tiles + nt) : nullptr;
  if constexpr (kSplit) {
    int* ticket = reinterpret_cast<int*>(smem + p.ticket_off);
    if (tid == 0) *ticket = (int)atomicAdd(sy, 1u);
    __syncthreads();
    ks = __builtin_amdgcn_readfirstlane(*ticket);
    const int nst_all = nst;
    st_off = nst_all * ks / kKs;
    nst = nst_all * (ks + 1) / kKs - st_off;
  }
  // (a lambda rather than a plain block: as a block, hipcc arranges this address arithmetic differently)
  auto operands = [&]() {
    int il, tr, tc;
    tm.decode(li, il, tr, tc);
    const int img = img0 + il, yy = ty * THt + tr, xx = tx * TWt + tc;
    const uint32_t t = (img < p.N && yy < p.tiles_h && xx < p.tiles_w) ? (uint32_t)((img * p.tiles_h + yy) * p.tiles_w + xx) : 0u;
    const uint32_t QT = (uint32_t)(p.Ctot >> 2) * (uint32_t)p.T;
#pragma unroll
    for (int j = 0; j < kNV; ++j) v_off[j] = ((uint32_t)pos_of(j) * QT + t) * 16u + 8u * (uint32_t)lh;
    vs = reinterpret_cast<const char*>(p.v) + (size_t)st_off * v_stage;      // (local) stage st: + st * T * 16 bytes
    us = reinterpret_cast<const char*>(p.wpk + ((size_t)nt * kWaves + wave) * kURegion) + 2048 + (size_t)st_off * u_stage;
  };
  operands();

  f32x16 acc[kNP];
#pragma unroll
  for (int j = 0; j < kNP; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  // The VMEM queue of a wave is a ring of 10 loads per stage, always in this order (loads return in order):
  //   V0 U0 | V1 U1 | V2 U2 | V3 U3 | V4 U4              (position i of the wave: its V run, then its weights)
  // each re-issued for stage st + 2 right after the MFMAs that consumed it in stage st.  Position i needs Ui of this stage (index
  // 2 i + 1; Vi is older): the loads issued since are the rest of its own round (8 - 2 i), the whole round of stage st + 1 (10)
  // and what this stage has re-issued so far (2 i) = 18, so s_waitcnt vmcnt(18) before every position.  kMode 1 = the stage
  // before the last (nothing is issued any more, the last stage's round is in flight): vmcnt(18 - 2 i); kMode 2 = the last
  // stage: vmcnt(8 - 2 i).
#define SSDE_W4R_LOADV(S, J) SSDE_GLOAD8_I(va[S][J], v_off[J], vn, 0)
#define SSDE_W4R_MFMA(S, J, BLK, B0, B1)                                                           \
  do {                                                                                             \
    acc[BLK] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[S][J].x, (B0), acc[BLK], 0, 0, 0);          \
    acc[BLK] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[S][J].y, (B1), acc[BLK], 0, 0, 0);          \
  } while (0)
#define SSDE_W4R_POS(S, I, IMM)                                                                    \
  do {                                                                                             \
    SSDE_WAIT_VMCNT_FOR(kMode == 0 ? 18 : kMode == 1 ? 18 - 2 * (I) : 8 - 2 * (I), va[S][I], u4[S][I]); \
    SSDE_W4R_MFMA(S, I, 2 * (I), u4[S][I].x, u4[S][I].y);                                          \
    __builtin_amdgcn_sched_barrier(0);                                                             \
    SSDE_W4R_MFMA(S, I, 2 * (I) + 1, u4[S][I].z, u4[S][I].w);                                      \
    __builtin_amdgcn_sched_barrier(0);                                                             \
    if (kMode == 0) { SSDE_W4R_LOADV(S, I); SSDE_GLOAD16_I(u4[S][I], u_off, un, IMM); }            \
    __builtin_amdgcn_sched_barrier(0);                                                             \
  } while (0)

  SSDE_RT(1);
  SSDE_W4R_ROUND_AT(0, vs, us);
  SSDE_W4R_ROUND_AT(1, vs + v_stage, us + u_stage);
#undef SSDE_W4R_ROUND_AT
  SSDE_RT(2);
  // stage st in register set S (= st & 1, a compile-time constant: the loop below is unrolled by two)
  auto stage = [&](auto SetC, auto ModeC, const int st) __attribute__((always_inline)) {
    constexpr int S = decltype(SetC)::value, kMode = decltype(ModeC)::value;
    const char* vn = vs + (size_t)(st + 2) * v_stage;
    const char* un = us + (size_t)(st + 2) * u_stage;
    if (st < 8) SSDE_RT(8 + st * 2);
    SSDE_W4R_POS(S, 0, -2048);
    SSDE_W4R_POS(S, 1, -1024);
    SSDE_W4R_POS(S, 2, 0);
    if (st < 8) SSDE_RT(8 + st * 2 + 1);
    SSDE_W4R_POS(S, 3, 1024);
    SSDE_WAIT_VMCNT_FOR(kMode == 0 ? 18 : kMode == 1 ? 10 : 0, va[S][4], u2[S]);
    SSDE_W4R_MFMA(S, 4, 8, u2[S].x, u2[S].y);
    __builtin_amdgcn_sched_barrier(0);
    if (kMode == 0) { SSDE_W4R_LOADV(S, 4); SSDE_GLOAD8_I(u2[S], u_off8, un, 0); }
    __builtin_amdgcn_sched_barrier(0);
  };
  {
    using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
    using Steady = std::integral_constant<int, 0>; using Penult = std::integral_constant<int, 1>; using Last = std::integral_constant<int, 2>;
    // (the launcher admits even stage counts only -- input channels a multiple of 8 -- so the tail is the same straight-line
    //  code for every launch: a branch per tail shape made hipcc spill hundreds of registers around the joins)
    int st = 0;
    // (The two waves of a SIMD share its matrix pipe and the older one wins every arbitration; a balance -- each wave posts its
    //  stage number in LDS, reads its partner's and takes the lower issue priority while it is ahead -- evened them out and
    //  changed nothing: the pair is bound by the bytes it pulls, not by who runs first.  profiles/r5_wino4r_simd_pair_balance_ab.txt)
    for (; st + 3 < nst; st += 2) { stage(S0{}, Steady{}, st); stage(S1{}, Steady{}, st + 1); }
    stage(S0{}, Penult{}, st);
    stage(S1{}, Last{}, st + 1);
  }
#undef SSDE_W4R_POS
#undef SSDE_W4R_MFMA
#undef SSDE_W4R_LOADV
  SSDE_RT(3);

  // ---- epilogue (wino4_common.h): products -> LDS, A^T M A per (tile, cout pair), parked 4x4 outputs, shared coalesced store ----
#ifdef SSDE_W4R_TRACE
  const Wino4rEpi epi{{}, tr_on, tr_base};
#else
  const Wino4rEpi epi{};
#endif
  wino4_epilogue<kKs>(acc, smem, p, tm, wave, nt, ks, sy, epi);
}

}  // namespace

// over how many workgroups per tile (1, 2 or 4) a launch of `wgs` tiles over `ctot` input channels splits its reduction: the
// shares must fit ONE round of workgroups (one per CU: the kernel owns a CU's registers), every share an even number of at least
// 8 channel stages.  SSDE_CONVF_NO_KSPLIT in the launch's flags switches it off.
int ssde_conv_wino4r_splits(int wgs, int ctot, int c_out, unsigned flags) {
  if ((flags & SSDE_CONVF_NO_KSPLIT) || c_out % 4 != 0) return 1;
  const int cus = ssde_num_cus();
  // (measured on 8x8 maps, profiles/r5_wino4r_split_8x8.txt, r5_wino4r_split_8x8_batch128.txt: at batch 256 two shares of 32 / 64
  //  stages take 0.077 / 0.112 ms against 0.098 / 0.163 unsplit, two shares of 16 stages -- 128 input channels -- are level; at
  //  batch 128 four shares 0.063 / 0.082 against 0.092 / 0.153.  The last share spends 13-15 k cycles on the hand-over,
  //  profiles/r5_wino4r_split_trace.txt: what ~6 stages cost)
  if (wgs * 4 <= cus && ctot % 32 == 0 && ctot >= 256) return 4;
  if (wgs * 2 <= cus && ctot % 16 == 0 && ctot >= 256) return 2;
  return 1;
}

namespace {

// Everything a launch needs, without touching a device: the parameter block (but for the split of the reduction, which takes
// hand-over slots), and the plan the queries report.  The source's prologue is the transform pass's business (wino4_xform.hip).
int wino4r_plan(const ssde_conv_args* a, Wino4rParams* pp, ssde_conv_plan* pl) {
  constexpr const char* kRoute = "conv(winograd 4x4, register-fed)";
  if (int rc = wino4_check_shape(a, kRoute, 8)) return rc;
  const ssde_src& s = a->main;
  if (int rc = ssde_src_check(s, kRoute, "", 4, SSDE_SRC_NEEDS_C0)) return rc;
  SSDE_REQUIRE((s.c0 + s.c1) % 8 == 0, "conv(winograd 4x4, register-fed): input channels must be a multiple of 8 (the stage loop runs in pairs)");
  Wino4rParams& p = *pp;
  p.v = a->wino_v; p.wpk = a->w_main; p.Ctot = s.c0 + s.c1;
  ssde_wino_tiling t;
  if (int rc = wino4_fill_shared(p, a, kRoute, &t, &pl->gn_slices)) return rc;
  p.ticket_off = kLds / 4;
  pl->lds_bytes = kLds + 16;
  static_assert(kLds + 16 <= 160 * 1024, "LDS of a CU");
  pl->ws_floats = 0;
  return SSDE_OK;
}

}  // namespace

// The route of a->tile == SSDE_TILE_WINOGRAD4R: the matrix kernel; ssde_conv2d issues the transform pass in front of it.
int ssde_conv_wino4r_plan(const ssde_conv_args* a, ssde_conv_plan* pl) {
  Wino4rParams p;
  return wino4r_plan(a, &p, pl);
}

int ssde_conv_wino4r_launch(const ssde_conv_args* a, hipStream_t st) {
  constexpr const char* kRoute = "conv(winograd 4x4, register-fed)";
  Wino4rParams p;
  ssde_conv_plan pl;
  if (int rc = wino4r_plan(a, &p, &pl)) return rc;
  SSDE_REQUIRE(a->wino_v, "conv(winograd 4x4, register-fed): the transformed-input buffer (ssde_conv_args.wino_v) is missing");
  SSDE_REQUIRE(36ull * (unsigned long long)p.T * (unsigned)p.Ctot * 4ull < (1ull << 32),
               "conv(winograd 4x4, register-fed): a transformed input of 4 GB or more is not addressable by this kernel");
  // the shares of the reduction: ssde_conv_wino4r_splits, the rule engine.Lowering.conv3_route mirrors
  const int grid = wino4_split_setup(p, a, ssde_conv_wino4r_splits);
  return wino4_launch_split<conv_wino4r_kernel<1>, conv_wino4r_kernel<2>, conv_wino4r_kernel<4>>(kRoute, p, grid, pl.lds_bytes, st);
}
