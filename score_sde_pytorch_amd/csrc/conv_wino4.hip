// 3x3 / stride 1 / pad 1 convolution by Winograd F(4x4, 3x3) on the exact-fp32 matrix pipe.
//
//   Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A     with 6x6 transformed tiles, 4x4 outputs per tile (Lavin & Gray,
//                                                    interpolation points 0, +-1, +-2)
// Per 4x4 output tile and (ci, co) pair the 144 multiply-adds of the direct form become 36 (F(2x2,3x3), conv_wino.hip:
// 64): the matrix pipe does 4x less work than the direct kernel and 1.78x less than F(2x2,3x3).  The price is
// rounding: the transforms multiply by up to 8 and the products are ~4-5x less accurate than F(2x2,3x3) in fp32.
// tools/experiments/wino43_error_budget.py runs the whole CIFAR-10 NCSN++ with every 3x3 layer in this form against
// an fp64 run: 2.5e-6 .. 1.3e-5 relative L2 error of the score (direct fp32: 4e-7 .. 1.2e-5), against the 1e-4 the
// parity tests allow.
//
// One workgroup (8 waves, two per SIMD) owns 32 tiles (a 32x16 output patch, or whole small images) x 64 output
// channels x all 36 transform positions; K advances 4 input channels per stage:
//   raw halo (+ fused GroupNorm / SiLU / dropout prologue)      -> LDS raw[pair][pixel][2]
//   input transform B^T d B in two 1-D passes, in place         -> LDS V[pos][tile][4]      (pitch 144 floats)
//   host-transformed weights G g G^T, packed as the LDS image   -> LDS U[pos][cout][4]      (36 KB, by LDS-DMA)
//   wave (q, h) = 9 positions {q, q+4, ..} x (32 tiles x 32 couts) on v_mfma_f32_32x32x2_f32: a lane's ds_read_b64 is
//   the channel pair (2k, 2k+1), k = lane >> 5 = the MFMA k index, one read of each operand feeds two MFMAs; all 64
//   lanes of a fragment read are 512 contiguous bytes (no bank conflicts)
// V and raw are double buffered, ONE LDS-only barrier per stage: a wave transforms 8 of the 64 (tile, channel pair) items
// with all their 6 lines, so the second 1-D pass reads what the same wave wrote in the first.  Every wave runs the same
// program; its halo loads, its weight DMA pieces and the LDS round trips of the two transform passes ride between its 18
// MFMAs (an MFMA only occupies the matrix pipe; the wave keeps issuing).
// The 36 positions of an output live in 4 waves, so the workgroup exchanges the products through LDS -- 16 tiles (half of
// every wave's accumulators) at a time, M[pos][16 tiles][64 couts] = 150 KB -- every thread applies A^T M A to one
// (tile, cout pair), and the result goes through the shared coalesced epilogue (ssde_store_tile: bias, temb addend,
// residual, scale, GroupNorm partials).
//
// Round 3 (profiles/r3_wino4_*.txt; every figure a same-box A/B against the round-2 kernel built as a variant library):
//   * U is PRIVATE per wave: the packed image of a stage is ordered [wave][position j][32 couts][4], wave (q, h) moves its
//     own 4.5 KB by LDS-DMA and is their only reader.  The stage barrier therefore carries no vmcnt(0) any more (it cost
//     400-570 cycles per stage: the last piece landed ~1500 cycles after its issue); a wave counts its own pieces with
//     vmcnt right before the fragment read that needs them.  The halo loads are issued from inline asm as well, so that
//     hipcc's waitcnt insertion (which cannot see the asm DMA pieces behind them) does not turn every use into vmcnt(0).
//   * The halo prologue (GroupNorm, SiLU, dropout -> raw) moved from the END of a stage to the HEAD of the next one (one
//     stage more of load latency covered, nothing between the last MFMA and the barrier), with the GroupNorm table reads
//     ahead of the head's burst of fragment / transform reads.
//   * The stage body is branch-free: flags are template parameters, the last three stages are peeled, lanes 48-63 of the
//     transforms work on padding columns.  hipcc's waitcnt counts are exact only in straight-line code (with the exec-masked
//     transform blocks every MFMA waited for the transform's LDS writes as well).
//   * One vector-memory instruction per position slot (as a burst in slots 0-1 they queued behind each other: 1500 cycles
//     for two positions); addressing by scalar base + 32-bit lane offset (no vector address arithmetic per stage).
//   Together +7 .. +10 % per layer (241-315 TF/s direct-equivalent with GroupNorm + SiLU, 240-333 without).
//   Measured and NOT adopted (profiles/r3_wino4_ab.txt): the transform as scalar v_fma_f32 instead of packed v_pk_*
//   (neutral: beside fp32 MFMAs, which share the VALU datapath, packing costs nothing); the two waves of a SIMD running
//   their prologue at opposite ends of the stage (neutral: a VALU instruction of one wave waits out the 64-cycle MFMA the
//   other has in the pipe, its head took 2100 cycles instead of 1500); the MFMAs of the
//   last three positions issued after the barrier inside the next head, fragments carried in registers (2-3 % slower: the
//   head grew by exactly the matrix cycles it gained -- LDS burst latency, VALU and fp32 MFMA time ADD on a SIMD).
//   Where a stage's ~4400 cycles go (s_memtime, tools/wino4_trace.py): 2304 are MFMAs of the SIMD's two waves, ~950 VALU
//   (prologue 2 x 130-260, transforms 2 x 120, bookkeeping), the rest LDS / VMEM issue latency that nothing overlaps
//   because all eight waves are in the same phase (one barrier per stage, double buffers: no wave may run ahead).
// Matrix-pipe occupancy, two ways.  Cycle trace of an unprofiled launch (tools/wino4_trace.py, profiles/r3_wino4_trace_e_*):
// matrix cycles / workgroup cycles = 0.40 for 128 -> 128 channels (73.7 k of 183 k: loop 146.5 k, fill 9.6 k, epilogue 27 k),
// 0.46 for 256 -> 256, 0.49 for 512 -> 256; inside the main loop 0.50-0.52.  PMC (SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE
// over all launches of the bench command): 0.40 in round 2 and in round 3 -- under rocprofv3 --pmc the kernel runs 26 %
// slower than unprofiled (408 vs 323 us per launch in one process), so the ratio understates the unprofiled kernel and moved
// less than the +7-10 % the same-box A/B shows.  The shader clock inside the kernel (s_memtime / s_memrealtime): 2.09-2.17 GHz.
#include "wino4_common.h"
#include <type_traits>

// -DSSDE_W4_TRACE (tools/wino4_trace.py, a variant library only): s_memtime stamps of waves 0 and 7 of the first workgroup
#ifdef SSDE_W4_TRACE
__device__ unsigned long long* g_w4_trace;
extern "C" int ssde_debug_w4_trace(void* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_w4_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -5;
}
#define SSDE_TR(slot)                                                                                     \
  do {                                                                                                    \
    if (tr_on) g_w4_trace[tr_base + (slot)] = __builtin_amdgcn_s_memtime();                               \
  } while (0)
// the same with the constant 100 MHz counter: (s_memtime delta) / (s_memrealtime delta) x 100 MHz = the shader clock the
// kernel actually ran at
#define SSDE_TRR(slot)                                                                                    \
  do {                                                                                                    \
    if (tr_on) g_w4_trace[tr_base + (slot)] = __builtin_amdgcn_s_memrealtime();                           \
  } while (0)
#else
#define SSDE_TR(slot) do { } while (0)
#define SSDE_TRR(slot) do { } while (0)
#endif


// fragment reads run this many positions (2 MFMAs = 128 matrix cycles each) ahead of their MFMAs
#ifndef SSDE_W4_PF
#define SSDE_W4_PF 3
#endif

namespace {

// 8 waves per workgroup, two per SIMD: 9 positions x one 32x32 block = 144 accumulator registers each.  (12 waves, three per
// SIMD at 96 accumulators, measured 11-25 % slower -- profiles/r2_wino4_ab_12_waves.txt: the stalls of this kernel are not
// latencies a third wave would cover, and the output transform spilled at 168 registers; the variant is no longer built.)
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kNP = 72 / kWaves;                   // positions per wave
constexpr int kPS = kWaves / 2;                    // wave (q, h) owns positions q + kPS * j
constexpr int kPos = 36, kTiles = 32, kKc = 4;
// LDS paddings, A/B-timed (profiles/r2_wino4_ab_lds_padding.txt): a V pitch of 128 + 24 (second transform pass free of bank
// conflicts instead of the first) and raw channel-pair planes 32 banks apart are both neutral: 35 % of the LDS cycles are
// bank conflicts (PMC), but the LDS is active only a third of the time
#ifndef SSDE_W4_VPAD
#define SSDE_W4_VPAD 16
#endif
constexpr int kVP = kTiles * kKc + SSDE_W4_VPAD;               // floats per position of V: 128 + 16, so that the 6 lines x 8 items of a
                                                    // wave's transform writes (b64) spread over all banks
constexpr int kVFloats = kPos * kVP;                // one V stage
constexpr int kUFloats = kPos * 64 * kKc;           // 9216: one U stage
constexpr int kURegion = kNP * 32 * kKc;            // 1152: the floats of a stage only wave (q, h) reads: [9 positions][32 couts][4]
static_assert(SSDE_W4_VPAD >= 16, "lanes 48-63 of the transform write the padding columns of V");
constexpr int kMaxRaw = 2;                          // float4 halo items per thread per stage (halo <= 1024 pixels)
static_assert(kThreads == kW4Threads && kNP == kW4Blocks, "wino4_epilogue");

struct Wino4Params : Wino4Shared {
  ssde_src src;
  const float* wpk;        // [ceil(C/4)][n_tiles][8 waves][9][32][4] (LDS image per stage, a wave's 4.5 KB contiguous)
  float* wino_v;           // kEmitV: V[pos][t][Ctot] = B^T pro(x) B for the F(4x4,3x3) weight gradient (ssde_conv_args.wino_v)
};

// What wino4_epilogue (wino4_common.h) asks of this kernel
struct Wino4Epi : Wino4EpiNoTrace {
  // wave (q, h) owns positions q + kPS j of cout half h
  static __device__ __forceinline__ int position(int wave, int j) { return (wave >> 1) + kPS * j; }
  static __device__ __forceinline__ int half(int wave, int) { return wave & 1; }
  static __device__ __forceinline__ void barrier() { __syncthreads(); }
  static __device__ __forceinline__ void lane_index(int tid, int& li, int& lh) { const int lane = tid & 63; li = lane & 31; lh = lane >> 5; }
#ifdef SSDE_W4_TRACE
  bool tr_on; int tr_base;
  // slots 100-106 and 4 of round 0, 5 and the 100 MHz counter at the end
  __device__ __forceinline__ void stamp(int phase, int rnd) const {
    constexpr int kSlot[] = {100, 101, 102, 103, 104, 105, -1, -1, -1, 106, 4, 5};
    if (rnd == 0 && kSlot[phase] >= 0) SSDE_TR(kSlot[phase]);
    if (phase == kW4Done) SSDE_TRR(111);
  }
#endif
};

// kKs = 2 or 4: that many workgroups per tile, each reducing its share of the channel stages (own instantiations: the
// hand-over costs the epilogue registers, and the unsplit kernel is the one the big layers run).  The shares are dealt in
// the order the workgroups START (an atomic counter per tile, as a decoupled look-back scan numbers its blocks): share k
// only ever waits for shares < k, which are resident or done -- no assumption about the dispatch order -- and the sums are
// formed in the fixed order ((s0 + s1) + s2) + s3, so the result does not depend on who arrived when.
// kEmitV (training forward, ssde_conv_args.wino_v): the workgroups of the FIRST cout tile also leave the transformed input of
// every stage in HBM, in the layout the F(4x4,3x3) weight-gradient GEMM reads (wgrad_wino4.hip: V[pos][t][ci]) -- the
// weight gradient of the layer then skips its own input-transform pass (wino4_xform_v_kernel: one read of x, the prologue and
// the 6x6 transform per element, 2.25x the tensor written: 2.4-2.7 ms of a training step).  Layout [pos][Ctot / 4][t][4].  Per stage 1152 float4 (36 positions
// x 32 tiles x 4 channels) leave LDS V[cur], 2.25 per thread, in the last three position slots, which carry no other
// vector-memory instruction.  Stores count in vmcnt like the loads: the counted waits of the stage stay correct (a wait for
// "at most n outstanding" can only become stricter when younger stores are still in flight), and the stores sit as far
// from the next counted wait -- the head of the next stage -- as the stage allows.
template <bool kGn, int kKs, bool kEmitV = false>
__global__ __launch_bounds__(kThreads, kWaves / 4) void conv_wino4_kernel(const Wino4Params p) {
  constexpr bool kSplit = kKs > 1;
  SSDE_LDS(smem);
  float* Vb = smem;                            // [2][kVFloats]
  float* Ub = smem + 2 * kVFloats;             // [2][8 waves][9 positions][32 couts][4]: a wave reads only its own region
  float* rawb = Ub + 2 * kUFloats;             // [2][2 pairs][halo_px][2], then the GroupNorm tables
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 31, lh = lane >> 5;

  // XCD-aware order (as conv_mfma.hip): the cout tiles of one pixel tile run on one XCD
  const int bid = blockIdx.x;
  const int xcd = bid & 7, l = bid >> 3;
  const int nt = l % p.n_tiles;
                                                             // (the kKs workgroups of a tile: same XCD, 8 * n_tiles blocks apart)
  const int mt = (l / (p.n_tiles * kKs)) * 8 + xcd;
#ifdef SSDE_W4_TRACE
  const bool tr_on = lane == 0 && (wave == 0 || wave == 7) && bid == 0 && g_w4_trace != nullptr;
  const int tr_base = (wave == 0 ? 0 : 1) * 128;
#endif
  SSDE_TR(0);
  SSDE_TRR(110);
  if (mt >= p.m_tiles) return;

  const int TWt = 1 << p.lTWt, THt = 1 << p.lTHt;
  const int IMGS = kTiles >> (p.lTWt + p.lTHt);
  const int HWd = 4 * TWt + 2, HH = 4 * THt + 2;
  const int halo_px = IMGS * HH * HWd;
  const int raw_plane = 2 * halo_px;           // floats between the two channel-pair planes of a raw buffer
  const int raw_stride = 2 * raw_plane;        // floats per raw buffer
  const Wino4TileMap tm(p, mt);
  const int img0 = tm.img0, ty = tm.ty, tx = tm.tx;

  const ssde_src& s = p.src;
  const int Ctot = s.c0 + s.c1;
  const int nst_all = (Ctot + 3) >> 2;
  // this workgroup's share of the reduction: stages st_off .. st_off + nst (`st` below counts from 0: LDS buffer parity and
  // the peeled last stages go by the local count, channels and weights by st + st_off)
  unsigned* sy = kSplit ? p.sync + 2 * ((size_t)mt * p.n_tiles + nt) : nullptr;
  int* ticket = reinterpret_cast<int*>(smem + p.ticket_off);
  if (kSplit && tid == 0) *ticket = (int)atomicAdd(sy, 1u);       // (read after the index set-up below)
  int ks = 0, st_off = 0, nst = nst_all;
  SsdePro pro = ssde_pro_decode(s);
  pro.gn = kGn;
  const int cpg = kGn ? Ctot / s.gn_groups : 1;
  const float inv_cpg = 1.0f / (float)cpg;

  // ---- raw staging plan: item = halo pixel (its 4 channels of the stage are one float4).  The byte offset of the pixel in
  // either source is a 32-bit VGPR, the channel offset of a stage rides in the scalar base (global_load ... v, s[:]): no
  // vector address arithmetic per stage (the launcher checks that a source is smaller than 4 GB) ----
  int goff[kMaxRaw], gil[kMaxRaw];
  uint32_t voff0[kMaxRaw], voff1[kMaxRaw];
#pragma unroll
  for (int it = 0; it < kMaxRaw; ++it) {
    const int q = tid + it * kThreads;
    goff[it] = -2; gil[it] = 0;
    if (q < halo_px) {
      const int il = q / (HH * HWd);
      const int rem = q - il * (HH * HWd);
      const int hy = rem / HWd, hx = rem - hy * HWd;
      const int iy = ty * 4 * THt - 1 + hy, ix = tx * 4 * TWt - 1 + hx;
      const int img = img0 + il;
      const bool inb = img < p.N && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      goff[it] = inb ? (img * p.H + iy) * p.W + ix : -1;
      gil[it] = inb ? il * (kGn ? s.gn_groups : 0) : 0;
    }
    const uint32_t px = (uint32_t)(goff[it] >= 0 ? goff[it] : 0);      // outside the image: a clamped, valid address
    voff0[it] = px * (uint32_t)s.c0 * 4u;
    voff1[it] = px * (uint32_t)s.c1 * 4u;
  }
  // ---- transform plan: a wave owns 8 of the 64 items (tile, channel pair) with all their 6 lines: lane = line * 8 + item,
  // so that pass 2 reads what the SAME wave wrote in pass 1 -- LDS executes a wave's operations in order, and no workgroup
  // barrier is needed between the passes.  Lanes 48-63 repeat lines 0 and 1 of the same items into the padding columns of V
  // (128 .. 143, never read by a fragment): every lane runs the same straight-line code, no exec-masked branch in the
  // stage body (hipcc's waitcnt insertion is exact only in straight-line code) ----
  const int t_line6 = lane >> 3;                          // 0..7
  const bool t_real = t_line6 < 6;
  const int t_line = t_real ? t_line6 : t_line6 - 6;
  const int t_item = wave * 8 + (lane & 7);
  const int t_tile = t_item >> 1, t_pair = t_item & 1;
  int t_base;
  {
    int il, tr, tc;
    tm.decode(t_tile, il, tr, tc);
    t_base = (il * HH + 4 * tr) * HWd + 4 * tc;
  }
  const int t_vcol = t_real ? t_tile * 4 + t_pair * 2 : kTiles * kKc + (lane & 7) * 2;
  const int t_rawoff = t_pair * raw_plane + (t_base + t_line) * 2;

  // V by-product plan: thread = (tile tid & 31, positions (tid >> 5) + 16 i).  One 32-bit byte offset per thread (the launcher
  // checks that V is smaller than 4 GB), the position block i and the stage's channels ride in the scalar base; 0xFFFFFFFF =
  // this thread stores nothing (another cout tile, a tile outside the batch)
  uint32_t ev_off = 0xFFFFFFFFu;
  const uint32_t ev_lds = (uint32_t)(((tid >> 5) * kVP + (tid & 31) * 4) * 4);
  if constexpr (kEmitV) {
    int eil, etr, etc;
    tm.decode(tid & 31, eil, etr, etc);
    const int eimg = img0 + eil, eyy = ty * THt + etr, exx = tx * TWt + etc;
    // layout [pos][Ctot / 4][t][4]: the 32 tiles of a workgroup are consecutive t for every map the networks have (a patch is
    // whole tile rows of one image, or whole images) -> one 512-byte run per position and stage.  (As [pos][t][Ctot], the
    // layout wino4_xform_v_kernel writes, every lane's 16 bytes were a separate memory transaction: the forward + input-gradient
    // class went from 25.0 to 31.6 ms, profiles/r4_wino_v_from_forward_ab.txt)
    if (p.wino_v != nullptr && nt == 0 && eimg < p.N && eyy < p.tiles_h && exx < p.tiles_w)
      ev_off = (uint32_t)((((tid >> 5) * (Ctot >> 2)) * p.T + (eimg * p.tiles_h + eyy) * p.tiles_w + exx) * 16);
  }
  auto emit_v = [&](const float* Vc, int st, int it) __attribute__((always_inline)) {
    if constexpr (kEmitV) {
      if (ev_off != 0xFFFFFFFFu && (it < 2 || tid < 128)) {          // positions 32..35: the first four 32-thread rows
        const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(Vc) + it * (16 * kVP * 4) + ev_lds);
        char* base = reinterpret_cast<char*>(p.wino_v) + ((size_t)it * 16 * (Ctot >> 2) + (size_t)(st + st_off)) * p.T * 16;
        *reinterpret_cast<float4*>(base + ev_off) = v;
      }
    }
  };
  // GroupNorm tables in LDS: (mean, rstd) of every (tile image, group), gamma and beta of every channel
  float* gn_tab = rawb + 2 * raw_stride;       // [IMGS][groups][2]
  // (rounded up to whole float4s: gamma / beta are read four channels at a time, and IMGS * groups may be odd)
  float* gb_tab = gn_tab + ((2 * IMGS * (kGn ? s.gn_groups : 0) + 3) & ~3);   // [2][Ctot]
  // halo loads of stage st: opaque to hipcc (SSDE_GLOAD16), their vmcnt accounting is the stage body's
  ssde_f32x4 rv[kMaxRaw];
  auto load_piece = [&](int st, int k) __attribute__((always_inline)) {
    const int c_base = (st + st_off) * 4;
    const bool second = c_base >= s.c0;
    const float* sb = second ? s.p1 + (c_base - s.c0) : s.p0 + c_base;
    const uint32_t vo = second ? voff1[k] : voff0[k];
    SSDE_GLOAD16(rv[k], vo, sb);
  };
  // prologue + raw LDS store (channel-pair major) of the halo in rv = stage st, in two steps so that a stage can put the few
  // LDS reads of the GroupNorm tables AHEAD of its burst of fragment / transform reads (LDS returns in order: the prologue
  // arithmetic then starts when 4 reads have come back instead of 16)
  struct GnRegs { float4 gam, bet; float2 mr[kMaxRaw]; };
  auto gn_fetch = [&](int st) __attribute__((always_inline)) {
    GnRegs r;
    r.gam = make_float4(1.f, 1.f, 1.f, 1.f); r.bet = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int it = 0; it < kMaxRaw; ++it) r.mr[it] = make_float2(0.f, 1.f);
    if (kGn) {
      const int c_cur = (st + st_off) * 4;
      r.gam = *reinterpret_cast<const float4*>(gb_tab + c_cur);
      r.bet = *reinterpret_cast<const float4*>(gb_tab + Ctot + c_cur);
      const int g = (int)(((float)c_cur + 0.5f) * inv_cpg);          // c_cur / cpg, exact for these small integers
#pragma unroll
      for (int it = 0; it < kMaxRaw; ++it) r.mr[it] = *reinterpret_cast<const float2*>(gn_tab + 2 * (gil[it] + g));   // (item 1 of most lanes: entry 0)
    }
    return r;
  };
  auto store_raw_with = [&](float* rw, int st, const GnRegs& r) __attribute__((always_inline)) {
    const int c_cur = (st + st_off) * 4;
#pragma unroll
    for (int it = 0; it < kMaxRaw; ++it) {
      if (goff[it] == -2) continue;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (goff[it] >= 0)
        v = ssde_pro_apply(make_float4(rv[it].x, rv[it].y, rv[it].z, rv[it].w), r.mr[it].x, r.mr[it].y, r.gam, r.bet,
                           (uint32_t)goff[it] * (uint32_t)Ctot + (uint32_t)c_cur, pro);
      const int q = tid + it * kThreads;
      *reinterpret_cast<float2*>(rw + q * 2) = make_float2(v.x, v.y);
      *reinterpret_cast<float2*>(rw + raw_plane + q * 2) = make_float2(v.z, v.w);
    }
  };
  auto store_raw = [&](float* rw, int st) __attribute__((always_inline)) { store_raw_with(rw, st, gn_fetch(st)); };
  // B^T d B in two 1-D passes over the 6x6 tile, the second in place: pass 1 lane = (column x), pass 2 lane = (row y)
  auto pass1 = [&](const float* rw, float* Vn) {
    const float* rp = rw + t_rawoff;
    float2 d[6], o[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) d[a] = *reinterpret_cast<const float2*>(rp + a * HWd * 2);
    bt6(d, o);
#pragma unroll
    for (int a = 0; a < 6; ++a) *reinterpret_cast<float2*>(Vn + (a * 6 + t_line) * kVP + t_vcol) = o[a];
  };
  auto pass2 = [&](float* Vn) {
    float* vp = Vn + (t_line * 6) * kVP + t_vcol;
    float2 d[6], o[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) d[b] = *reinterpret_cast<const float2*>(vp + b * kVP);
    bt6(d, o);
#pragma unroll
    for (int b = 0; b < 6; ++b) *reinterpret_cast<float2*>(vp + b * kVP) = o[b];
  };
  // Weights of a stage: the host packed them as the LDS image (36 KB per stage) in the order [wave][position j][32 couts][4]:
  // wave (q, h) moves -- and is the only reader of -- the 9 x 512 B of its positions q + 4 j and its cout half h, as 4.5
  // LDS-DMA pieces of 1 KB (the last one on lanes 0-31).  No other wave waits for these bytes: the wave counts its own
  // pieces with vmcnt right before the fragment read that needs them, and the stage barrier carries no vmcnt(0).
  // One scalar base per stage, the lane's bytes as a constant 32-bit offset, the pieces as immediates -2048 .. +2048.
  const uint32_t w_voff = (uint32_t)((wave * kURegion + 2 * 256 + lane * 4) * 4);
  auto w_base = [&](int st) { return p.wpk + ((size_t)(st + st_off) * p.n_tiles + nt) * kUFloats; };
  auto w_ldst = [&](float* Un) { return Un + wave * kURegion + 2 * 256; };

  const int wq = wave >> 1;                     // this wave's positions wq + 4 j (its cout half is wave & 1)
  f32x16 acc[kNP];
#pragma unroll
  for (int j = 0; j < kNP; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const int a_off = li * 4 + 2 * lh, b_off = wave * kURegion + li * 4 + 2 * lh;

  if constexpr (kSplit) {
    __syncthreads();
    ks = __builtin_amdgcn_readfirstlane(*ticket);
    st_off = nst_all * ks / kKs;
    nst = nst_all * (ks + 1) / kKs - st_off;
  }
  // ---- pipeline fill.  Leaves what every stage expects on entry: V[cur] transformed, the wave's weight pieces of the stage
  // issued, raw[nxt] = the activated halo of stage st + 1, rv = the halo of stage st + 2 ----
  SSDE_TR(1);
  {
    const float* wb = w_base(0);
    float* ld = w_ldst(Ub);
    SSDE_GLDS16_S(w_voff, wb, ld, -2048);
    SSDE_GLDS16_S_SAME_BASE(w_voff, wb, ld, -1024);
    SSDE_GLDS16_S_SAME_BASE(w_voff, wb, ld, 0);
    SSDE_GLDS16_S_SAME_BASE(w_voff, wb, ld, 1024);
    SSDE_GLDS16_S_SAME_BASE_LO32(w_voff, wb, ld, 2048);
  }
#pragma unroll
  for (int k = 0; k < kMaxRaw; ++k) load_piece(0, k);
  // (the table loads below are issued behind the weight pieces and the halo of stage 0: one memory latency for all of them)
  if (kGn) {
    for (int q = tid; q < IMGS * s.gn_groups; q += kThreads) {
      const int il = q / s.gn_groups, img = img0 + il < p.N ? img0 + il : 0;
      const int gi = img * s.gn_groups + (q - il * s.gn_groups);
      *reinterpret_cast<float2*>(gn_tab + 2 * q) = make_float2(s.gn_mean[gi], s.gn_rstd[gi]);
    }
    for (int q = tid; q < Ctot; q += kThreads) { gb_tab[q] = s.gn_gamma[q]; gb_tab[Ctot + q] = s.gn_beta[q]; }
  }
  __syncthreads();                             // publishes the GroupNorm tables
  SSDE_WAIT_VMCNT_FOR(0, rv[0], rv[1]);
  store_raw(rawb, 0);
  if (nst > 1) {
#pragma unroll
    for (int k = 0; k < kMaxRaw; ++k) load_piece(1, k);
  }
  SSDE_LDS_BARRIER();
  pass1(rawb, Vb);
  SSDE_LDS_BARRIER();                          // (a wave's lanes run in lockstep: only the test emulator's fibers need this one)
  pass2(Vb);
  SSDE_WAIT_VMCNT_FOR(0, rv[0], rv[1]);        // unconditional: every path from a halo load to its use passes a counted wait
  if (nst > 1) store_raw(rawb + raw_stride, 1);
  if (nst > 2) {
#pragma unroll
    for (int k = 0; k < kMaxRaw; ++k) load_piece(2, k);
  }
  SSDE_WAIT_VMCNT_FOR(0, rv[0], rv[1]);
  SSDE_LDS_BARRIER();
  SSDE_TR(2);

  // ---- one stage.  HAS1: a stage st + 1 exists (its weights are fetched and its input transformed here), HAS2: the halo of
  // stage st + 2 is activated and stored, HASL: the halo of stage st + 3 is fetched (stored at the head of the next stage).
  // Compile-time flags: the main loop runs the all-true body, the last stages are peeled, and the body has no branch.
  //
  //   head     own weight pieces 0, 1 landed | fragment reads of positions 0..2 | pass-1 reads | prologue of rv -> raw[cur]
  //   slot j   fragment reads of position j + 3 | 2 MFMAs of position j | ONE vector-memory instruction (slots 0..6:
  //            P0' H0' P1' H1' P2' P3' P4' -- as a burst in slots 0-1 the halo loads and the first pieces queued behind each
  //            other in the address path: 1500 cycles for two positions, tools/wino4_trace.py / profiles/r3_wino4_trace_a.txt)
  //            after slot 1: pass-1 arithmetic and writes; after 3: pass-2 reads; after 5: pass-2 arithmetic and writes
  //   tail     LDS-only barrier
  // The short VALU / LDS bursts of the prologue and of the transforms run at s_setprio 2, as conv_wino.hip's staging.
  //
  // VMEM queue of a wave (in issue order; P = weight piece of this stage, ' = of the next, H = halo load):
  //   on entry           [P0 H0 P1 H1 P2 P3 P4]                         vmcnt(3): pieces 0, 1 (positions 0..3) and rv
  //   slot 1 (pos 4, 5)  [P2 P3 P4 P0']                                 piece 2 <=> vmcnt(2 + HAS1)
  //   slot 3 (pos 6, 7)  [P3 P4 P0' H0' P1']                            piece 3 <=> vmcnt(1 + 2 HAS1 + HASL)
  //   slot 5 (pos 8)     [P4 P0' H0' P1' H1' P2']                       piece 4 <=> vmcnt(3 HAS1 + 2 HASL)
  // (fragment reads run SSDE_W4_PF = 3 positions ahead, so the read of position j + 3 is what a slot's count protects) ----
  static_assert(SSDE_W4_PF == 3 && kWaves == 8, "the vmcnt counts of the stage body assume reads 3 positions ahead");
  auto stage = [&](auto H1, auto H2, auto HL, const int st) __attribute__((always_inline)) {
    constexpr bool has1 = decltype(H1)::value, has2 = decltype(H2)::value, hasl = decltype(HL)::value;
    constexpr int n1 = has1 ? 1 : 0, nl = hasl ? 1 : 0;
    const int cur = st & 1, nxt = cur ^ 1;
    const float* Vc = Vb + cur * kVFloats;
    const float* Uc = Ub + cur * kUFloats;
    float* Vn = Vb + nxt * kVFloats;
    ssde_f32x2 td[6], to[6];
    ssde_lds_float* tw = (ssde_lds_float*)(Vn + t_line * kVP + t_vcol);            // pass-1 column of this lane
    ssde_lds_float* vp = (ssde_lds_float*)(Vn + (t_line * 6) * kVP + t_vcol);      // pass-2 row of this lane
    SSDE_OPAQUE_VGPR(tw);
    SSDE_OPAQUE_VGPR(vp);
    ssde_f32x2 af[SSDE_W4_PF + 1], bf[SSDE_W4_PF + 1];
    const float* wb = w_base(has1 ? st + 1 : st);
    float* wl = w_ldst(Ub + nxt * kUFloats);
    // one fragment base per operand, opaque to the compiler: the 9 positions are immediate offsets of the ds_read (left
    // alone, hipcc kept a VGPR and a 3-operand add per position and operand: 18 VALU per stage and 16 registers)
    ssde_lds_cfloat* va = (ssde_lds_cfloat*)(Vc + wq * kVP + a_off);
    ssde_lds_cfloat* ua = (ssde_lds_cfloat*)(Uc + b_off);
    SSDE_OPAQUE_VGPR(va);
    SSDE_OPAQUE_VGPR(ua);
    // ---- head ----
    GnRegs gnr;
    if (has2) gnr = gn_fetch(st + 2);                   // (tables: no dependence on the weight pieces)
    if (has2) SSDE_WAIT_VMCNT_FOR(3, rv[0], rv[1]); else SSDE_WAIT_VMCNT_FENCE(3);
#pragma unroll
    for (int j = 0; j < SSDE_W4_PF; ++j) {
      af[j] = *(ssde_lds_cfloat2*)(va + kPS * j * kVP);
      bf[j] = *(ssde_lds_cfloat2*)(ua + j * 128);
    }
    if (has1) {
      const float* rp = rawb + nxt * raw_stride + t_rawoff;
#pragma unroll
      for (int a = 0; a < 6; ++a) { const float2 q = *reinterpret_cast<const float2*>(rp + a * HWd * 2); td[a].x = q.x; td[a].y = q.y; }
    }
    if (has2) {
      __builtin_amdgcn_s_setprio(2);
      store_raw_with(rawb + cur * raw_stride, st + 2, gnr);
      __builtin_amdgcn_s_setprio(0);
    }
    if (st < 8) SSDE_TR(8 + st * 10 + 1);
    __builtin_amdgcn_sched_barrier(0);
#define SSDE_W4_POS(J)                                                                                          \
    do {                                                                                                         \
      if ((J) + SSDE_W4_PF < kNP) {                                                                                \
        af[((J) + SSDE_W4_PF) % (SSDE_W4_PF + 1)] =                                                              \
            *(ssde_lds_cfloat2*)(va + kPS * ((J) + SSDE_W4_PF) * kVP);                                           \
        bf[((J) + SSDE_W4_PF) % (SSDE_W4_PF + 1)] =                                                              \
            *(ssde_lds_cfloat2*)(ua + ((J) + SSDE_W4_PF) * 128);                                                 \
      }                                                                                                          \
      acc[J] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[(J) % (SSDE_W4_PF + 1)].x, bf[(J) % (SSDE_W4_PF + 1)].x, acc[J], 0, 0, 0); \
      acc[J] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[(J) % (SSDE_W4_PF + 1)].y, bf[(J) % (SSDE_W4_PF + 1)].y, acc[J], 0, 0, 0); \
      __builtin_amdgcn_sched_barrier(0);                                                                         \
    } while (0)
    // ---- slots ----
    SSDE_W4_POS(0);
    if (has1) SSDE_GLDS16_S(w_voff, wb, wl, -2048);
    __builtin_amdgcn_sched_barrier(0);
    SSDE_WAIT_VMCNT_FENCE(2 + n1);
    SSDE_W4_POS(1);
    if (hasl) load_piece(st + 3, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (st < 8) SSDE_TR(8 + st * 10 + 2);
    if (has1) {
      __builtin_amdgcn_s_setprio(2);
      bt6(td, to);
#pragma unroll
      for (int a = 0; a < 6; ++a) *(ssde_lds_float2*)(tw + a * 6 * kVP) = to[a];
      __builtin_amdgcn_s_setprio(0);
    }
    if (st < 8) SSDE_TR(8 + st * 10 + 3);
    __builtin_amdgcn_sched_barrier(0);
    SSDE_W4_POS(2);
    if (has1) SSDE_GLDS16_S_SAME_BASE(w_voff, wb, wl, -1024);
    __builtin_amdgcn_sched_barrier(0);
    SSDE_WAIT_VMCNT_FENCE(1 + 2 * n1 + nl);
    SSDE_W4_POS(3);
    if (hasl) load_piece(st + 3, 1);
    __builtin_amdgcn_sched_barrier(0);
    if (st < 8) SSDE_TR(8 + st * 10 + 4);
    if (has1) {
#pragma unroll
      for (int b = 0; b < 6; ++b) td[b] = *(ssde_lds_float2*)(vp + b * kVP);
    }
    __builtin_amdgcn_sched_barrier(0);
    SSDE_W4_POS(4);
    if (has1) SSDE_GLDS16_S_SAME_BASE(w_voff, wb, wl, 0);
    __builtin_amdgcn_sched_barrier(0);
    SSDE_WAIT_VMCNT_FENCE(3 * n1 + 2 * nl);
    SSDE_W4_POS(5);
    if (has1) SSDE_GLDS16_S_SAME_BASE(w_voff, wb, wl, 1024);
    __builtin_amdgcn_sched_barrier(0);
    if (has1) {
      __builtin_amdgcn_s_setprio(2);
      bt6(td, to);
#pragma unroll
      for (int b = 0; b < 6; ++b) *(ssde_lds_float2*)(vp + b * kVP) = to[b];
      __builtin_amdgcn_s_setprio(0);
    }
    if (st < 8) SSDE_TR(8 + st * 10 + 5);
    __builtin_amdgcn_sched_barrier(0);
    SSDE_W4_POS(6);
    if (has1) SSDE_GLDS16_S_SAME_BASE_LO32(w_voff, wb, wl, 2048);
    emit_v(Vc, st, 0);
    __builtin_amdgcn_sched_barrier(0);
    SSDE_W4_POS(7);
    emit_v(Vc, st, 1);
    __builtin_amdgcn_sched_barrier(0);
    SSDE_W4_POS(8);
    emit_v(Vc, st, 2);
#undef SSDE_W4_POS
    if (st < 8) SSDE_TR(8 + st * 10 + 6);
    SSDE_LDS_BARRIER();
    if (st < 8) SSDE_TR(8 + st * 10 + 8);
  };
  {
    using T = std::true_type; using F = std::false_type;
    // (written so that the stage that consumes the halo in flight is the only successor of the stage that fetched it: the
    //  registers of an asm load are not protected by hipcc on a path it merely cannot rule out, tests/test_isa_guards.py)
    int st = 0;
    if (nst >= 3) {
      for (; st + 3 < nst; ++st) stage(T{}, T{}, T{}, st);
      stage(T{}, T{}, F{}, st); ++st;
      stage(T{}, F{}, F{}, st); ++st;
    } else if (nst == 2) {
      stage(T{}, F{}, F{}, st); ++st;
    }
    stage(F{}, F{}, F{}, st);
  }
  SSDE_TR(3);

  // ---- epilogue (wino4_common.h).  The 36 positions of an output live in 4 waves: the workgroup exchanges the products
  // through LDS, 16 tiles at a time ----
#ifdef SSDE_W4_TRACE
  const Wino4Epi epi{{}, tr_on, tr_base};
#else
  const Wino4Epi epi{};
#endif
  wino4_epilogue<kKs>(acc, smem, p, tm, wave, nt, ks, sy, epi);
}

}  // namespace

// over how many workgroups per tile (1, 2 or 4) a launch of `wgs` tiles over `ctot` input channels splits its reduction: up
// to 256 workgroups, at least 16 channel stages each (engine.py picks this kernel for 8x8 maps only where the split fills
// the chip -- same rule there).  SSDE_CONVF_NO_KSPLIT in the launch's flags switches it off.
int ssde_conv_wino4_splits(int wgs, int ctot, int c_out, unsigned flags) {
  if ((flags & SSDE_CONVF_NO_KSPLIT) || c_out % 4 != 0) return 1;
  const int cus = ssde_num_cus();                   // (256 on the MI355X: a quarter / half of the chip covered)
  if (wgs <= cus / 4 && ctot >= 256) return 4;
  if (wgs <= cus / 2 && ctot >= 128) return 2;
  return 1;
}

namespace {

// Everything a launch needs, without touching a device: the parameter block (but for the split of the reduction, which takes
// hand-over slots), and the plan the queries report.
int wino4_plan(const ssde_conv_args* a, Wino4Params* pp, ssde_conv_plan* pl) {
  constexpr const char* kRoute = "conv(winograd 4x4)";
  if (int rc = wino4_check_shape(a, kRoute, 8)) return rc;
  const ssde_src& s = a->main;
  if (int rc = ssde_src_check(s, kRoute, "", 4, SSDE_SRC_ALL)) return rc;
  // the halo loads address a source as scalar base + 32-bit byte offset
  SSDE_REQUIRE((unsigned long long)a->n * a->h_in * a->w_in * (unsigned)(s.c0 > s.c1 ? s.c0 : s.c1) * 4ull < (1ull << 32),
               "conv(winograd 4x4): a source of 4 GB or more is not addressable by this kernel");
  Wino4Params& p = *pp;
  p.src = s; p.wpk = a->w_main; p.wino_v = a->wino_v;
  SSDE_REQUIRE(!a->wino_v || 36ull * (unsigned long long)(a->n * (a->h_out / 4) * (a->w_out / 4)) * (unsigned)(s.c0 + s.c1) * 4ull < (1ull << 32),
               "conv(winograd 4x4): a transformed-input by-product of 4 GB or more is not addressable by this kernel");
  ssde_wino_tiling t;
  if (int rc = wino4_fill_shared(p, a, kRoute, &t, &pl->gn_slices)) return rc;
  const int halo_px = t.imgs * (4 * t.tht + 2) * (4 * t.twt + 2);
  SSDE_REQUIRE(halo_px <= kMaxRaw * kThreads, "conv(winograd 4x4): halo of %d pixels exceeds the staging plan", halo_px);
  int lds = (2 * kVFloats + 2 * kUFloats + 2 * 2 * 2 * halo_px) * 4;
  if (s.pro_mode == SSDE_PRO_GN || s.pro_mode == SSDE_PRO_GN_SILU) lds += (((2 * t.imgs * s.gn_groups + 3) & ~3) + 2 * (s.c0 + s.c1)) * 4;
  if (lds < kW4EpiLds) lds = kW4EpiLds;
  p.ticket_off = lds / 4;
  lds += 16;
  SSDE_REQUIRE(lds <= 160 * 1024, "conv(winograd 4x4): %d bytes of LDS", lds);
  pl->lds_bytes = lds;
  pl->ws_floats = 0;
  return SSDE_OK;
}

// the instantiation of a launch: GroupNorm prologue, V written as a by-product; wino4_launch_split: the shares of the reduction
template <bool kGn, bool kV>
int wino4_launch_as(const Wino4Params& p, int wgs, int lds, hipStream_t st) {
  return wino4_launch_split<conv_wino4_kernel<kGn, 1, kV>, conv_wino4_kernel<kGn, 2, kV>, conv_wino4_kernel<kGn, 4, kV>>(
      "conv(winograd 4x4)", p, wgs, lds, st);
}

}  // namespace

// The route of a->tile == SSDE_TILE_WINOGRAD4.
int ssde_conv_wino4_plan(const ssde_conv_args* a, ssde_conv_plan* pl) {
  Wino4Params p;
  return wino4_plan(a, &p, pl);
}

int ssde_conv_wino4_launch(const ssde_conv_args* a, hipStream_t st) {
  Wino4Params p;
  ssde_conv_plan pl;
  if (int rc = wino4_plan(a, &p, &pl)) return rc;
  const int grid = wino4_split_setup(p, a, ssde_conv_wino4_splits);
  const bool gn = p.src.pro_mode == SSDE_PRO_GN || p.src.pro_mode == SSDE_PRO_GN_SILU;
  if (a->wino_v) return gn ? wino4_launch_as<true, true>(p, grid, pl.lds_bytes, st) : wino4_launch_as<false, true>(p, grid, pl.lds_bytes, st);
  return gn ? wino4_launch_as<true, false>(p, grid, pl.lds_bytes, st) : wino4_launch_as<false, false>(p, grid, pl.lds_bytes, st);
}
