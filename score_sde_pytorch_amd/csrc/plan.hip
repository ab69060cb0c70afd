// Plan-level C entry points: a whole lowered program (U-Net evaluation, or a predictor-corrector iteration) loaded from a
// PLAN BLOB and driven by a host that has no Python -- SURVEY 8(b): ssde_plan_*, ssde_unet_forward, ssde_pc_*, ssde_ode_*.
//
// The reference's host is Python (NCSNpp.forward models/ncsnpp.py:232-381, pc_sampler sampling.py:390-409); its lowering
// to kernels stays in ONE place, score_sde_pytorch_amd/engine.py + pc_engine.py.  plan_export.py serialises what that
// lowering produced -- the flat ssde_op array, the liveness-planned activation arena, the packed kernel-layout weights,
// the reference-layout parameters with their state_dict names, the device-side re-pack descriptor tables, the step
// tables of the sampler -- as a position-independent blob: every pointer field is a (region, byte offset) relocation.
// This file allocates the regions on the device, uploads their initial contents, patches the pointers and runs the
// program; a C / C++ / Go / Rust host needs only libssde_hip.so, the blob and (optionally) a checkpoint to copy into
// the parameter regions followed by ssde_plan_refresh_weights.
#include "ssde_common.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

namespace {

struct Region { void* dev = nullptr; int64_t bytes = 0; int kind = 0; char name[32]; };

}  // namespace

struct ssde_plan {
  ssde_plan_header hdr;
  std::vector<Region> regions;
  std::vector<ssde_op> ops, refresh_ops;
  std::vector<ssde_plan_param_entry> params;
  void* graph = nullptr;
  hipStream_t graph_stream = nullptr;
  // ODE plans: which of the two state buffers holds y; host ring of per-evaluation records (ode.py: _FusedRhs._upload)
  int ode_cur = 0;
  ssde_ode_dyn* ode_ring = nullptr;
  int ode_slot = 0, ode_inflight = 0;
  hipStream_t ode_stream = nullptr;
  // sampler plans with a projection: ssde_pc_set_known has filled the known-data and mask regions
  bool known_set = false;
};

namespace {

void ode_ring_free(ssde_ode_dyn* ring);

int fail_free(ssde_plan* p, int rc) {
  if (p) {
    for (auto& r : p->regions)
      if (r.dev) hipFree(r.dev);
    ode_ring_free(p->ode_ring);
    delete p;
  }
  return rc;
}

void* region_ptr(const ssde_plan* p, int id) {
  return (id >= 0 && id < (int)p->regions.size()) ? p->regions[id].dev : nullptr;
}

}  // namespace

extern "C" int ssde_plan_load(const void* blob, size_t bytes, ssde_plan** out) {
  SSDE_REQUIRE(blob && out && bytes >= sizeof(ssde_plan_header), "plan: blob too small");
  const char* base = static_cast<const char*>(blob);
  ssde_plan_header h;
  memcpy(&h, base, sizeof(h));
  SSDE_REQUIRE(memcmp(h.magic, "SSDEPLN1", 8) == 0, "plan: bad magic");
  SSDE_REQUIRE(h.abi_version == SSDE_ABI_VERSION && h.sizeof_op == (int)sizeof(ssde_op),
               "plan: blob built for ABI %d / op size %d, library has %d / %d", h.abi_version, h.sizeof_op, SSDE_ABI_VERSION,
               (int)sizeof(ssde_op));
  const size_t need = sizeof(h) + (size_t)h.n_regions * sizeof(ssde_plan_region) + (size_t)(h.n_ops + h.n_refresh_ops) * sizeof(ssde_op) +
                      (size_t)h.n_relocs * sizeof(ssde_plan_reloc) + (size_t)h.n_params * sizeof(ssde_plan_param_entry) + (size_t)h.data_bytes;
  SSDE_REQUIRE(bytes >= need, "plan: blob truncated (%zu of %zu bytes)", bytes, need);
  const ssde_plan_region* regs = reinterpret_cast<const ssde_plan_region*>(base + sizeof(h));
  const char* ops_raw = reinterpret_cast<const char*>(regs + h.n_regions);
  const ssde_plan_reloc* rel = reinterpret_cast<const ssde_plan_reloc*>(ops_raw + (size_t)(h.n_ops + h.n_refresh_ops) * sizeof(ssde_op));
  const ssde_plan_param_entry* par = reinterpret_cast<const ssde_plan_param_entry*>(rel + h.n_relocs);
  const char* data = reinterpret_cast<const char*>(par + h.n_params);

  ssde_plan* p = new ssde_plan;
  p->hdr = h;
  p->regions.resize(h.n_regions);
  // staging copies of the constant regions (pointers inside them are patched before the upload)
  std::vector<std::vector<char>> staged(h.n_regions);
  for (int i = 0; i < h.n_regions; ++i) {
    Region& r = p->regions[i];
    r.bytes = regs[i].bytes; r.kind = regs[i].kind;
    memcpy(r.name, regs[i].name, sizeof(r.name));
    if (r.bytes <= 0) continue;
    if (hipMalloc(&r.dev, (size_t)r.bytes) != hipSuccess) {
      ssde_set_error("plan: hipMalloc of %lld bytes for region %d (%s) failed", (long long)r.bytes, i, r.name);
      return fail_free(p, SSDE_EHIP);
    }
    if (regs[i].kind == SSDE_REGION_CONST) {
      if (regs[i].data_offset < 0 || regs[i].data_offset + r.bytes > h.data_bytes) { ssde_set_error("plan: region %d data out of range", i); return fail_free(p, SSDE_EINVAL); }
      staged[i].assign(data + regs[i].data_offset, data + regs[i].data_offset + r.bytes);
    }
  }
  p->ops.resize(h.n_ops);
  p->refresh_ops.resize(h.n_refresh_ops);
  if (h.n_ops) memcpy(p->ops.data(), ops_raw, (size_t)h.n_ops * sizeof(ssde_op));
  if (h.n_refresh_ops) memcpy(p->refresh_ops.data(), ops_raw + (size_t)h.n_ops * sizeof(ssde_op), (size_t)h.n_refresh_ops * sizeof(ssde_op));
  for (int i = 0; i < h.n_relocs; ++i) {
    const ssde_plan_reloc& q = rel[i];
    if (q.region < 0 || q.region >= h.n_regions || q.offset < 0 || q.offset > p->regions[q.region].bytes) {
      ssde_set_error("plan: relocation %d points outside region %d", i, q.region);
      return fail_free(p, SSDE_EINVAL);
    }
    char* target = static_cast<char*>(p->regions[q.region].dev) + q.offset;
    char* where = nullptr;
    if (q.target_kind == SSDE_RELOC_OP && q.target >= 0 && q.target < h.n_ops) where = reinterpret_cast<char*>(&p->ops[q.target]);
    else if (q.target_kind == SSDE_RELOC_REFRESH_OP && q.target >= 0 && q.target < h.n_refresh_ops) where = reinterpret_cast<char*>(&p->refresh_ops[q.target]);
    else if (q.target_kind == SSDE_RELOC_REGION && q.target >= 0 && q.target < h.n_regions && !staged[q.target].empty()) where = staged[q.target].data();
    const int64_t limit = q.target_kind == SSDE_RELOC_REGION ? (where ? (int64_t)staged[q.target].size() : 0) : (int64_t)sizeof(ssde_op);
    if (!where || q.byte_offset < 0 || q.byte_offset + (int64_t)sizeof(void*) > limit) {
      ssde_set_error("plan: relocation %d has a bad target", i);
      return fail_free(p, SSDE_EINVAL);
    }
    memcpy(where + q.byte_offset, &target, sizeof(void*));
  }
  for (int i = 0; i < h.n_regions; ++i) {
    Region& r = p->regions[i];
    if (r.bytes <= 0) continue;
    hipError_t e = staged[i].empty() ? hipMemset(r.dev, 0, (size_t)r.bytes)
                                     : hipMemcpy(r.dev, staged[i].data(), (size_t)r.bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { ssde_set_error("plan: initialising region %d failed", i); return fail_free(p, SSDE_EHIP); }
  }
  p->params.assign(par, par + h.n_params);
  *out = p;
  return SSDE_OK;
}

extern "C" int ssde_plan_load_file(const char* path, ssde_plan** out) {
  SSDE_REQUIRE(path && out, "plan: null args");
  FILE* f = fopen(path, "rb");
  SSDE_REQUIRE(f, "plan: cannot open %s", path);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf(n > 0 ? (size_t)n : 0);
  const size_t got = n > 0 ? fread(buf.data(), 1, (size_t)n, f) : 0;
  fclose(f);
  SSDE_REQUIRE(n > 0 && got == (size_t)n, "plan: short read of %s", path);
  return ssde_plan_load(buf.data(), buf.size(), out);
}

extern "C" int ssde_plan_destroy(ssde_plan* p) {
  if (!p) return SSDE_OK;
  if (p->graph) ssde_graph_destroy(p->graph);
  fail_free(p, 0);
  return SSDE_OK;
}

extern "C" int ssde_plan_info(const ssde_plan* p, ssde_plan_header* out) {
  SSDE_REQUIRE(p && out, "plan: null args");
  *out = p->hdr;
  return SSDE_OK;
}

// Device address of a reference-layout parameter ("all_modules.3.weight", ...) for the host to copy checkpoint data
// into; index < 0 looks the name up, else `name_out` receives the index-th name.
extern "C" int ssde_plan_param(const ssde_plan* p, const char* name, int index, float** dev, int64_t* numel, const char** name_out) {
  SSDE_REQUIRE(p, "plan: null plan");
  int found = -1;
  if (index >= 0) found = index < (int)p->params.size() ? index : -1;
  else if (name)
    for (size_t i = 0; i < p->params.size(); ++i)
      if (strncmp(p->params[i].name, name, sizeof(p->params[i].name)) == 0) { found = (int)i; break; }
  SSDE_REQUIRE(found >= 0, "plan: no parameter %s", name ? name : "(index out of range)");
  const ssde_plan_param_entry& q = p->params[found];
  if (dev) *dev = reinterpret_cast<float*>(static_cast<char*>(region_ptr(p, q.region)) + q.offset);
  if (numel) *numel = q.numel;
  if (name_out) *name_out = q.name;
  return SSDE_OK;
}

extern "C" int ssde_plan_refresh_weights(ssde_plan* p, void* stream) {
  SSDE_REQUIRE(p, "plan: null plan");
  return ssde_program_run(p->refresh_ops.data(), (int)p->refresh_ops.size(), stream);
}

namespace {
int copy_in(const ssde_plan* p, int slot, const void* src, size_t bytes, hipStream_t st) {
  void* dst = region_ptr(p, p->hdr.io[slot]);
  SSDE_REQUIRE(dst && src, "plan: I/O slot %d missing", slot);
  SSDE_REQUIRE((int64_t)bytes <= p->regions[p->hdr.io[slot]].bytes, "plan: I/O slot %d too small", slot);
  SSDE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
  return SSDE_OK;
}
}  // namespace

// out = model(x, cond): x, out [B, C, H, W] fp32, cond [B] (the noise level sigma or the time label, exactly what
// NCSNpp.forward receives), all DEVICE pointers.  `sigma` (discrete-label models with scale_by_sigma) and `std`
// (VP score head) may be NULL when the plan has no such input.
extern "C" int ssde_unet_forward(ssde_plan* p, const float* x, const float* cond, const float* sigma, const float* std_,
                                 float* out, void* stream) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_UNET, "unet_forward: not a U-Net plan");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float);
  if (int rc = copy_in(p, SSDE_IO_X, x, img, st)) return rc;
  if (int rc = copy_in(p, SSDE_IO_COND, cond, (size_t)h.batch * sizeof(float), st)) return rc;
  if (h.io[SSDE_IO_SIGMA] >= 0 && h.io[SSDE_IO_SIGMA] != h.io[SSDE_IO_COND])
    if (int rc = copy_in(p, SSDE_IO_SIGMA, sigma, (size_t)h.batch * sizeof(float), st)) return rc;
  if (h.io[SSDE_IO_STD] >= 0)
    if (int rc = copy_in(p, SSDE_IO_STD, std_, (size_t)h.batch * sizeof(float), st)) return rc;
  if (int rc = ssde_program_run(p->ops.data(), (int)p->ops.size(), stream)) return rc;
  SSDE_REQUIRE(out, "unet_forward: null output");
  SSDE_HIP_CHECK(hipMemcpyAsync(out, region_ptr(p, h.io[SSDE_IO_OUT]), img, hipMemcpyDeviceToDevice, st));
  return SSDE_OK;
}

// ---- predictor-corrector sampler plans (pc_engine.FusedPCSampler: one program = one PC iteration) ----
extern "C" int ssde_pc_reset(ssde_plan* p, const float* x_T, uint64_t seed, void* stream) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_PC, "pc_reset: not a sampler plan");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float);
  if (int rc = copy_in(p, SSDE_IO_X, x_T, img, st)) return rc;
  if (int rc = copy_in(p, SSDE_IO_XMEAN, x_T, img, st)) return rc;
  SSDE_HIP_CHECK(hipMemsetAsync(region_ptr(p, h.io[SSDE_IO_STEP]), 0, sizeof(int32_t), st));
  SSDE_HIP_CHECK(hipStreamSynchronize(st));
  SSDE_HIP_CHECK(hipMemcpy(region_ptr(p, h.io[SSDE_IO_SEED]), &seed, sizeof(seed), hipMemcpyHostToDevice));
  return SSDE_OK;
}

// n PC iterations on `stream`; use_graph != 0: the iteration is captured into a hipGraph on first use (stream must then
// be a non-default stream) and replayed -- the device step counter and seed word make every replay a new iteration.
// What the iteration of a sampler plan says about itself (controllable generation: pc_engine's emit_projection puts one
// SSDE_OP_PROJECT after the corrector block and one after the predictor block, both on the same known data and mask).
namespace {
struct PcView {
  const ssde_project_args* proj[2] = {nullptr, nullptr};   // after the corrector, after the predictor
  float* noise[4] = {nullptr, nullptr, nullptr, nullptr};  // corrector, predictor, the two projections (the order of `noises[:, k]`)
  int n_proj = 0;
  bool draws_noise = false;                                // the iteration holds SSDE_OP_RANDN: it fills the buffers itself
};

int pc_view(const ssde_plan* p, PcView* v, const char* who) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_PC, "%s: not a sampler plan", who);
  for (const ssde_op& op : p->ops) {
    if (op.kind == SSDE_OP_RANDN) v->draws_noise = true;
    else if (op.kind == SSDE_OP_LANGEVIN && !v->noise[0]) v->noise[0] = const_cast<float*>(op.u.langevin.noise);
    else if (op.kind == SSDE_OP_PREDICTOR && !v->noise[1]) v->noise[1] = const_cast<float*>(op.u.predictor.noise);
    else if (op.kind == SSDE_OP_PROJECT) {
      if (v->n_proj < 2) { v->proj[v->n_proj] = &op.u.project; v->noise[2 + v->n_proj] = const_cast<float*>(op.u.project.noise); }
      v->n_proj++;
    }
  }
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float);
  auto holds = [&](const void* q) {                        // a whole image at q lies inside one region of the plan
    const char* c = static_cast<const char*>(q);
    for (const Region& r : p->regions) {
      const char* base = static_cast<const char*>(r.dev);
      if (base && c >= base && c + img <= base + r.bytes) return true;
    }
    return false;
  };
  for (int k = 0; k < 4; ++k) SSDE_REQUIRE(!v->noise[k] || holds(v->noise[k]), "%s: noise buffer %d of the plan is smaller than the state", who, k);
  if (v->n_proj == 0) return SSDE_OK;
  const ssde_project_args *a = v->proj[0], *b = v->proj[1];
  SSDE_REQUIRE(v->n_proj == 2 && a->data && a->mask && a->x && a->x_mean && a->data == b->data && a->mask == b->mask && a->x == b->x &&
                   a->x_mean == b->x_mean && a->use_matrix == b->use_matrix,
               "%s: the plan's iteration holds %d projections that do not share one known-data / mask / state (expected two that do)", who, v->n_proj);
  SSDE_REQUIRE(a->n == h.batch && a->c == h.channels && a->hw == h.height * h.width, "%s: the projection is [%d,%d,%d], the plan [%d,%d,%d x %d]", who,
               a->n, a->c, a->hw, h.batch, h.channels, h.height, h.width);
  SSDE_REQUIRE(holds(a->data) && holds(a->mask) && holds(a->x) && holds(a->x_mean), "%s: a projection buffer of the plan is smaller than the state", who);
  return SSDE_OK;
}

// the launch arguments shared by set_known and reset_known: shape, form and matrices of the plan's own projection
void prepare_args_of(const ssde_project_args* pj, ssde_project_prepare_args* a) {
  memset(a, 0, sizeof(*a));
  a->n = pj->n; a->c = pj->c; a->hw = pj->hw; a->use_matrix = pj->use_matrix;
  memcpy(a->M, pj->M, sizeof(a->M));
  memcpy(a->invM, pj->invM, sizeof(a->invM));
}
}  // namespace

extern "C" int ssde_pc_projection(const ssde_plan* p) {
  PcView v;
  if (int rc = pc_view(p, &v, "pc_projection")) return rc;
  return v.n_proj == 0 ? SSDE_PC_PROJ_NONE : v.proj[0]->use_matrix ? SSDE_PC_PROJ_COLOR : SSDE_PC_PROJ_MASK;
}

extern "C" int ssde_pc_set_known(ssde_plan* p, const float* data, const float* mask, void* stream) {
  PcView v;
  if (int rc = pc_view(p, &v, "pc_set_known")) return rc;
  SSDE_REQUIRE(v.n_proj > 0, "pc_set_known: the plan's iteration has no projection (an unconditional sampler)");
  SSDE_REQUIRE(data, "pc_set_known: null data");
  SSDE_REQUIRE(mask || v.proj[0]->use_matrix, "pc_set_known: an inpainting plan needs a mask (NULL = the task's own mask: colorization only)");
  ssde_project_prepare_args a;
  prepare_args_of(v.proj[0], &a);
  a.data = data; a.mask = mask;
  a.known = const_cast<float*>(v.proj[0]->data);
  a.mask_out = const_cast<float*>(v.proj[0]->mask);
  if (int rc = ssde_project_prepare(&a, stream)) return rc;
  p->known_set = true;
  return SSDE_OK;
}

extern "C" int ssde_pc_reset_known(ssde_plan* p, const float* prior, uint64_t seed, void* stream) {
  PcView v;
  if (int rc = pc_view(p, &v, "pc_reset_known")) return rc;
  SSDE_REQUIRE(v.n_proj > 0, "pc_reset_known: the plan's iteration has no projection (an unconditional sampler: ssde_pc_reset)");
  SSDE_REQUIRE(p->known_set, "pc_reset_known: the known data was never set (ssde_pc_set_known comes first)");
  SSDE_REQUIRE(prior, "pc_reset_known: null prior");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ssde_plan_header& h = p->hdr;
  SSDE_REQUIRE(region_ptr(p, h.io[SSDE_IO_STEP]) && region_ptr(p, h.io[SSDE_IO_SEED]), "pc_reset_known: the plan has no step counter / seed word");
  ssde_project_prepare_args a;
  prepare_args_of(v.proj[0], &a);
  a.prior = prior;
  a.known = const_cast<float*>(v.proj[0]->data);     // read: data == NULL
  a.mask = v.proj[0]->mask;
  a.x = v.proj[0]->x; a.x_mean = v.proj[0]->x_mean;
  if (int rc = ssde_project_prepare(&a, stream)) return rc;
  SSDE_HIP_CHECK(hipMemsetAsync(region_ptr(p, h.io[SSDE_IO_STEP]), 0, sizeof(int32_t), st));
  SSDE_HIP_CHECK(hipStreamSynchronize(st));
  SSDE_HIP_CHECK(hipMemcpy(region_ptr(p, h.io[SSDE_IO_SEED]), &seed, sizeof(seed), hipMemcpyHostToDevice));
  return SSDE_OK;
}

extern "C" int ssde_pc_set_noise(ssde_plan* p, int32_t which, const float* z, void* stream) {
  PcView v;
  if (int rc = pc_view(p, &v, "pc_set_noise")) return rc;
  SSDE_REQUIRE(!v.draws_noise, "pc_set_noise: the plan draws its own noise (it contains SSDE_OP_RANDN; export it with with_rng=False)");
  SSDE_REQUIRE(which >= 0 && which < 4 && z, "pc_set_noise: which = %d (0 corrector, 1 predictor, 2 / 3 the projections) or null noise", which);
  static const char* const kStage[4] = {"corrector", "predictor", "projection after the corrector", "projection after the predictor"};
  SSDE_REQUIRE(v.noise[which], "pc_set_noise: the plan has no %s stage", kStage[which]);
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float);
  SSDE_HIP_CHECK(hipMemcpyAsync(v.noise[which], z, img, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return SSDE_OK;
}

extern "C" int ssde_pc_run(ssde_plan* p, int32_t n_iterations, int32_t use_graph, void* stream) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_PC && n_iterations >= 0, "pc_run: bad args");
  if (!p->known_set) {
    PcView v;
    if (int rc = pc_view(p, &v, "pc_run")) return rc;
    SSDE_REQUIRE(v.n_proj == 0, "pc_run: the plan's iteration projects onto known data that was never set (ssde_pc_set_known; a zero mask "
                                "would run an unconditional sampler)");
  }
  if (use_graph) {
    if (!p->graph || p->graph_stream != static_cast<hipStream_t>(stream)) {
      if (p->graph) { ssde_graph_destroy(p->graph); p->graph = nullptr; }
      if (int rc = ssde_graph_capture(p->ops.data(), (int)p->ops.size(), stream, &p->graph)) return rc;
      p->graph_stream = static_cast<hipStream_t>(stream);
    }
    for (int i = 0; i < n_iterations; ++i)
      if (int rc = ssde_graph_launch(p->graph, stream)) return rc;
    return SSDE_OK;
  }
  for (int i = 0; i < n_iterations; ++i)
    if (int rc = ssde_program_run(p->ops.data(), (int)p->ops.size(), stream)) return rc;
  return SSDE_OK;
}

extern "C" int ssde_pc_state(ssde_plan* p, float* x, float* x_mean, void* stream) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_PC, "pc_state: not a sampler plan");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float);
  if (x) SSDE_HIP_CHECK(hipMemcpyAsync(x, region_ptr(p, h.io[SSDE_IO_X]), img, hipMemcpyDeviceToDevice, st));
  if (x_mean) SSDE_HIP_CHECK(hipMemcpyAsync(x_mean, region_ptr(p, h.io[SSDE_IO_XMEAN]), img, hipMemcpyDeviceToDevice, st));
  return SSDE_OK;
}

// ---- ODE plans (ode.FusedDrift / ode.FusedLikelihoodRhs: one program = one right-hand-side evaluation) ----
// The driver below is ode._initial_step + ode.solve_rk line for line (scipy's explicit methods RK23, RK45 and DOP853: the
// method's table, FSAL, RMS error norm -- DOP853: its combined 5th / 3rd-order estimate --, factor 0.9 err^(-1/(order+1))
// in [0.2, 10]); host arithmetic in double, one scalar read per step.  It holds no SDE formulas: the four floats of the
// device record come from the host's callback.
namespace {
constexpr int kOdeRing = 32;
// scipy 1.15's tables (scipy/integrate/_ivp/rk.py, dop853_coefficients.py: the first 12 stages), the values of ode.TABLEAUS.
// A is stored with 12 columns for every method; e2 is the second error row of DOP853's estimator (then e = E5, e2 = E3).
struct Tableau {
  const char* name;
  int n_stages, order;
  const double* c;
  const double (*a)[12];
  const double* b;
  const double* e;
  const double* e2;
};
const double kRk23C[3] = {0.0, 1.0 / 2, 3.0 / 4};
const double kRk23A[3][12] = {{0}, {1.0 / 2}, {0.0, 3.0 / 4}};
const double kRk23B[3] = {2.0 / 9, 1.0 / 3, 4.0 / 9};
const double kRk23E[4] = {5.0 / 72, -1.0 / 12, -1.0 / 9, 1.0 / 8};
const double kRk45C[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
const double kRk45A[6][12] = {{0},
                              {1.0 / 5},
                              {3.0 / 40, 9.0 / 40},
                              {44.0 / 45, -56.0 / 15, 32.0 / 9},
                              {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
                              {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
const double kRk45B[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
const double kRk45E[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
const double kDopC[12] = {0.0, 0.05260015195876773, 0.0789002279381516, 0.1183503419072274, 0.2816496580927726, 0.3333333333333333, 0.25, 0.3076923076923077, 0.6512820512820513, 0.6, 0.8571428571428571, 1.0};
const double kDopA[12][12] = {{0},
    {0.05260015195876773},
    {0.0197250569845379, 0.0591751709536137},
    {0.02958758547680685, 0.0, 0.08876275643042054},
    {0.2413651341592667, 0.0, -0.8845494793282861, 0.924834003261792},
    {0.037037037037037035, 0.0, 0.0, 0.17082860872947386, 0.12546768756682242},
    {0.037109375, 0.0, 0.0, 0.17025221101954405, 0.06021653898045596, -0.017578125},
    {0.03709200011850479, 0.0, 0.0, 0.17038392571223998, 0.10726203044637328, -0.015319437748624402, 0.008273789163814023},
    {0.6241109587160757, 0.0, 0.0, -3.3608926294469414, -0.868219346841726, 27.59209969944671, 20.154067550477894, -43.48988418106996},
    {0.47766253643826434, 0.0, 0.0, -2.4881146199716677, -0.590290826836843, 21.230051448181193, 15.279233632882423, -33.28821096898486, -0.020331201708508627},
    {-0.9371424300859873, 0.0, 0.0, 5.186372428844064, 1.0914373489967295, -8.149787010746927, -18.52006565999696, 22.739487099350505, 2.4936055526796523, -3.0467644718982196},
    {2.273310147516538, 0.0, 0.0, -10.53449546673725, -2.0008720582248625, -17.9589318631188, 27.94888452941996, -2.8589982771350235, -8.87285693353063, 12.360567175794303, 0.6433927460157636}};
const double kDopB[12] = {0.054293734116568765, 0.0, 0.0, 0.0, 0.0, 4.450312892752409, 1.8915178993145003, -5.801203960010585, 0.3111643669578199, -0.1521609496625161, 0.20136540080403034, 0.04471061572777259};
const double kDopE3[13] = {-0.18980075407240762, 0.0, 0.0, 0.0, 0.0, 4.450312892752409, 1.8915178993145003, -5.801203960010585, -0.4226823213237919, -0.1521609496625161, 0.20136540080403034, 0.02265179219836082, 0.0};
const double kDopE5[13] = {0.01312004499419488, 0.0, 0.0, 0.0, 0.0, -1.2251564463762044, -0.4957589496572502, 1.6643771824549864, -0.35032884874997366, 0.3341791187130175, 0.08192320648511571, -0.022355307863886294, 0.0};
const Tableau kTableaus[3] = {{"RK45", 6, 4, kRk45C, kRk45A, kRk45B, kRk45E, nullptr},      // indexed by SSDE_ODE_*
                              {"RK23", 3, 2, kRk23C, kRk23A, kRk23B, kRk23E, nullptr},
                              {"DOP853", 12, 7, kDopC, kDopA, kDopB, kDopE5, kDopE3}};
constexpr double kSafety = 0.9, kMinFactor = 0.2, kMaxFactor = 10.0;

// The pinned ring: the six evaluations of a step are enqueued without a host wait, so the record of an evaluation must
// not be overwritten before its upload has executed.  (The test emulator executes every copy at the call.)
ssde_ode_dyn* ode_ring_alloc() {
#ifdef SSDE_EMULATED
  return static_cast<ssde_ode_dyn*>(malloc(kOdeRing * sizeof(ssde_ode_dyn)));
#else
  void* q = nullptr;
  return hipHostMalloc(&q, kOdeRing * sizeof(ssde_ode_dyn), hipHostMallocDefault) == hipSuccess ? static_cast<ssde_ode_dyn*>(q) : nullptr;
#endif
}
void ode_ring_free(ssde_ode_dyn* ring) {
  if (!ring) return;
#ifdef SSDE_EMULATED
  free(ring);
#else
  (void)hipHostFree(ring);
#endif
}

struct Ode {                       // the regions of an ODE plan, bounds checked
  int64_t n = 0, N = 0;            // image elements; state length (n, or n + B)
  int rows = 0;                    // slope rows of K the plan holds (>= 7)
  double *K = nullptr, *y[2] = {nullptr, nullptr}, *y_stage = nullptr, *partial = nullptr, *out = nullptr;
  float* x32 = nullptr;            // the U-Net program's input
  ssde_ode_dyn* dyn = nullptr;
};

int ode_view(const ssde_plan* p, Ode* o, const char* who) {
  SSDE_REQUIRE(p && (p->hdr.kind == SSDE_PLAN_ODE || p->hdr.kind == SSDE_PLAN_LIKELIHOOD), "%s: not an ODE plan", who);
  const ssde_plan_header& h = p->hdr;
  o->n = (int64_t)h.batch * h.channels * h.height * h.width;
  o->N = o->n + (h.kind == SSDE_PLAN_LIKELIHOOD ? h.batch : 0);
  auto bytes = [&](int slot) { const int id = h.io[slot]; return (id >= 0 && id < (int)p->regions.size()) ? p->regions[id].bytes : (int64_t)0; };
  SSDE_REQUIRE(o->n > 0 && bytes(SSDE_IO_X) >= o->n * (int64_t)sizeof(float) && bytes(SSDE_IO_ODE_DYN) >= (int64_t)sizeof(ssde_ode_dyn) &&
                   bytes(SSDE_IO_ODE_K) >= 7 * o->N * (int64_t)sizeof(double) &&
                   bytes(SSDE_IO_ODE_STATE) >= (3 * o->N + SSDE_ODE_PARTIALS + 1) * (int64_t)sizeof(double),
               "%s: the plan's solver regions are missing or too small", who);
  if (h.kind == SSDE_PLAN_LIKELIHOOD)
    SSDE_REQUIRE(bytes(SSDE_IO_ODE_PROBE) >= o->n * (int64_t)sizeof(float) && bytes(SSDE_IO_GOUT) >= o->n * (int64_t)sizeof(float),
                 "%s: the likelihood plan has no probe / cotangent region", who);
  o->x32 = static_cast<float*>(region_ptr(p, h.io[SSDE_IO_X]));
  o->rows = (int)(bytes(SSDE_IO_ODE_K) / (o->N * (int64_t)sizeof(double)));
  o->dyn = static_cast<ssde_ode_dyn*>(region_ptr(p, h.io[SSDE_IO_ODE_DYN]));
  o->K = static_cast<double*>(region_ptr(p, h.io[SSDE_IO_ODE_K]));
  double* s = static_cast<double*>(region_ptr(p, h.io[SSDE_IO_ODE_STATE]));
  o->y[0] = s; o->y[1] = s + o->N; o->y_stage = s + 2 * o->N; o->partial = s + 3 * o->N; o->out = o->partial + SSDE_ODE_PARTIALS;
  return SSDE_OK;
}

// dst = y + sum_j coef[j] K[j], and its fp32 copy into the U-Net input (the log-density tail of a likelihood state stays fp64)
int ode_combine(const Ode& o, const double* y, const double* coef, int n_coef, double* dst, void* stream) {
  ssde_rk_combine_rows_args a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < n_coef; ++j) {
    a.coef[j] = coef[j];
    if (coef[j] != 0.0) a.terms = j + 1;
  }
  a.y = y; a.k = o.K; a.n = o.N; a.dst = dst; a.dst32 = o.x32; a.n32 = o.n;
  return ssde_rk_combine_rows(&a, stream);
}

// scipy's error norm over atol + max(|y|, |y_new|) rtol, the one host read of a step.  coef2 == NULL: the RMS norm of
// sum_j coef[j] K[j] (coef = E_j h); else DOP853's norm of the pair (coef = E5, coef2 = E3, not scaled) and |h|.
int ode_norm(ssde_plan* p, const Ode& o, const double* y, const double* y_new, const double* coef, const double* coef2, int rows, double h_abs,
             double atol, double rtol, double* value, hipStream_t st) {
  ssde_rk_error_rows_args a;
  memset(&a, 0, sizeof(a));
  a.y = y; a.y_new = y_new; a.k = o.K; a.n = o.N; a.rows = rows; a.pair = coef2 != nullptr; a.h_abs = h_abs; a.atol = atol; a.rtol = rtol;
  a.partial = o.partial; a.partial_len = SSDE_ODE_PARTIALS; a.out = o.out;
  for (int j = 0; j < rows; ++j) {
    a.coef[j] = coef[j];
    if (coef2) a.coef2[j] = coef2[j];
  }
  if (int rc = ssde_rk_error_norm_rows(&a, st)) return rc;
  SSDE_HIP_CHECK(hipMemcpyAsync(value, o.out, sizeof(double), hipMemcpyDeviceToHost, st));
  SSDE_HIP_CHECK(hipStreamSynchronize(st));
  p->ode_inflight = 0;
  return SSDE_OK;
}

// upload the record of one evaluation (the callback's four floats and the slope row to fill), then run the program
int ode_evaluate(ssde_plan* p, const Ode& o, double t, ssde_ode_scalars_fn scalars, void* user, double* dst, int use_graph, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const int cb = scalars(t, user, v);
  SSDE_REQUIRE(cb == 0, "ode: the scalars callback returned %d at t = %.17g", cb, t);
  if (!p->ode_ring) {
    p->ode_ring = ode_ring_alloc();
    SSDE_REQUIRE(p->ode_ring, "ode: allocating the host record ring failed");
  }
  if (p->ode_inflight > 0 && (p->ode_stream != st || p->ode_inflight >= kOdeRing)) {
    SSDE_HIP_CHECK(hipStreamSynchronize(p->ode_stream));
    p->ode_inflight = 0;
  }
  p->ode_stream = st;
  ssde_ode_dyn& r = p->ode_ring[p->ode_slot];
  p->ode_slot = (p->ode_slot + 1) % kOdeRing;
  p->ode_inflight++;
  r.label = v[0]; r.std = v[1]; r.a = v[2]; r.g2 = v[3]; r.dst = dst;
  SSDE_HIP_CHECK(hipMemcpyAsync(o.dyn, &r, sizeof(r), hipMemcpyHostToDevice, st));
  if (!use_graph) return ssde_program_run(p->ops.data(), (int)p->ops.size(), stream);
  if (!p->graph || p->graph_stream != st) {
    if (p->graph) { ssde_graph_destroy(p->graph); p->graph = nullptr; }
    if (int rc = ssde_graph_capture(p->ops.data(), (int)p->ops.size(), stream, &p->graph)) return rc;
    p->graph_stream = st;
  }
  return ssde_graph_launch(p->graph, stream);
}
}  // namespace

extern "C" int ssde_ode_reset(ssde_plan* p, const float* x0, const float* probe, void* stream) {
  Ode o;
  if (int rc = ode_view(p, &o, "ode_reset")) return rc;
  SSDE_REQUIRE(x0, "ode_reset: null x0");
  const bool lik = p->hdr.kind == SSDE_PLAN_LIKELIHOOD;
  SSDE_REQUIRE(lik || !probe, "ode_reset: a sampler plan takes no probe");
  hipStream_t st = static_cast<hipStream_t>(stream);
  // y = (double)x0 (exact), log-density terms 0: widened on the host, once per solve
  std::vector<float> x((size_t)o.n);
  std::vector<double> y((size_t)o.N, 0.0);
  SSDE_HIP_CHECK(hipMemcpyAsync(x.data(), x0, (size_t)o.n * sizeof(float), hipMemcpyDeviceToHost, st));
  SSDE_HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < o.n; ++i) y[(size_t)i] = (double)x[(size_t)i];
  p->ode_cur = 0;
  SSDE_HIP_CHECK(hipMemcpyAsync(o.y[0], y.data(), (size_t)o.N * sizeof(double), hipMemcpyHostToDevice, st));
  if (probe) {      // fixed for the whole solve (likelihood.py:76-81); it is also the cotangent of the input-gradient program
    if (int rc = copy_in(p, SSDE_IO_ODE_PROBE, probe, (size_t)o.n * sizeof(float), st)) return rc;
    if (int rc = copy_in(p, SSDE_IO_GOUT, probe, (size_t)o.n * sizeof(float), st)) return rc;
  }
  SSDE_HIP_CHECK(hipStreamSynchronize(st));                           // `y` is this frame's
  return SSDE_OK;
}

extern "C" int ssde_ode_eval(ssde_plan* p, double t, ssde_ode_scalars_fn scalars, void* user, double* slope, void* stream) {
  Ode o;
  if (int rc = ode_view(p, &o, "ode_eval")) return rc;
  SSDE_REQUIRE(scalars && slope, "ode_eval: null callback / slope");
  if (int rc = ode_combine(o, o.y[p->ode_cur], nullptr, 0, o.y_stage, stream)) return rc;
  return ode_evaluate(p, o, t, scalars, user, slope, 0, stream);
}

extern "C" int ssde_ode_solve_method(ssde_plan* p, int32_t method, double t0, double t1, double rtol, double atol, ssde_ode_scalars_fn scalars,
                                     void* user, int32_t use_graph, int32_t max_nfev, int32_t* nfev_out, void* stream) {
  Ode o;
  if (int rc = ode_view(p, &o, "ode_solve")) return rc;
  SSDE_REQUIRE(method >= 0 && method < 3, "ode_solve: method %d is none of SSDE_ODE_RK45, SSDE_ODE_RK23, SSDE_ODE_DOP853", method);
  const Tableau& tab = kTableaus[method];
  const int S = tab.n_stages;
  SSDE_REQUIRE(o.rows >= S + 1, "ode_solve: %s needs %d slope rows, the plan holds %d (export_ode_plan(rhs, method=...) sizes them)", tab.name,
               S + 1, o.rows);
  SSDE_REQUIRE(scalars, "ode_solve: null scalars callback");
  SSDE_REQUIRE(t0 != t1 && isfinite(t0) && isfinite(t1), "ode_solve: t0 == t1 (or a non-finite time)");
  SSDE_REQUIRE(rtol > 0 && atol > 0 && max_nfev >= 0, "ode_solve: rtol, atol must be positive and max_nfev >= 0");
  SSDE_REQUIRE(!use_graph || stream, "ode_solve: graph replay needs a non-default stream");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int limit = max_nfev > 0 ? max_nfev : 100000;
  const double exponent = -1.0 / (tab.order + 1);
  int nfev = 0;
  if (nfev_out) *nfev_out = 0;
  double t = t0;
  const double t_bound = t1, direction = t_bound >= t ? 1.0 : -1.0;
  const size_t row = (size_t)o.N * sizeof(double);
  double* y = o.y[p->ode_cur];
  double* y_new = o.y[p->ode_cur ^ 1];
  auto K = [&](int j) { return o.K + (size_t)j * o.N; };
  SSDE_REQUIRE(limit >= 2, "ode_solve: max_nfev = %d reached after 0 evaluations", limit);
  // The Dormand-Prince solve keeps the launches it always had, this clear of its rows among them; the stage kernels do not
  // read a row whose coefficient is zero, so no method needs it.
  if (method == SSDE_ODE_RK45) SSDE_HIP_CHECK(hipMemsetAsync(o.K, 0, 7 * row, st));
  if (int rc = ode_combine(o, y, nullptr, 0, o.y_stage, stream)) return rc;   // stage argument of the first evaluation (and its fp32 copy)
  if (int rc = ode_evaluate(p, o, t, scalars, user, K(0), use_graph, stream)) return rc;
  nfev = 1;
  // ---- ode._initial_step (scipy's select_initial_step with the method's order); with y_new = y the scale is atol + |y0| rtol.
  // Row 2 (every method has one) holds a copy of y for d0, before any stage fills it.
  double h_abs;
  {
    double c[3] = {0, 0, 0}, d0, d1, d2;
    SSDE_HIP_CHECK(hipMemcpyAsync(K(2), y, row, hipMemcpyDeviceToDevice, st));
    c[2] = 1.0;
    if (int rc = ode_norm(p, o, y, y, c, nullptr, 3, 0.0, atol, rtol, &d0, st)) return rc;
    c[2] = 0.0; c[0] = 1.0;
    if (int rc = ode_norm(p, o, y, y, c, nullptr, 3, 0.0, atol, rtol, &d1, st)) return rc;
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    const double step[1] = {h0 * direction};
    if (int rc = ode_combine(o, y, step, 1, o.y_stage, stream)) return rc;
    if (int rc = ode_evaluate(p, o, t + h0 * direction, scalars, user, K(1), use_graph, stream)) return rc;
    c[0] = -1.0; c[1] = 1.0;
    if (int rc = ode_norm(p, o, y, y, c, nullptr, 3, 0.0, atol, rtol, &d2, st)) return rc;
    d2 /= h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / (tab.order + 1));
    h_abs = fmin(100 * h0, h1);
    SSDE_REQUIRE(isfinite(h_abs), "ode_solve: the initial step is not finite (d0 %g, d1 %g, d2 %g)", d0, d1, d2);
  }
  nfev += 1;
  if (nfev_out) *nfev_out = nfev;
  while (direction * (t - t_bound) < 0) {
    const double min_step = 10 * fabs(nextafter(t, direction * INFINITY) - t);
    h_abs = fmax(h_abs, min_step);
    bool rejected = false;
    double t_new;
    for (;;) {
      SSDE_REQUIRE(!(h_abs < min_step), "ode_solve: step size underflow at t = %.17g (scipy: 'Required step size is less than spacing between numbers.')", t);
      SSDE_REQUIRE(nfev + S <= limit, "ode_solve: max_nfev = %d reached at t = %.17g after %d evaluations", limit, t, nfev);
      double h = h_abs * direction;
      t_new = t + h;
      if (direction * (t_new - t_bound) > 0) t_new = t_bound;
      h = t_new - t;
      h_abs = fabs(h);
      double c[SSDE_RK_MAX_ROWS];
      for (int s = 1; s < S; ++s) {
        for (int j = 0; j < s; ++j) c[j] = tab.a[s][j] * h;
        if (int rc = ode_combine(o, y, c, s, o.y_stage, stream)) return rc;
        if (int rc = ode_evaluate(p, o, t + tab.c[s] * h, scalars, user, K(s), use_graph, stream)) return rc;
      }
      for (int j = 0; j < S; ++j) c[j] = tab.b[j] * h;
      if (int rc = ode_combine(o, y, c, S, y_new, stream)) return rc;          // (its fp32 copy feeds the last evaluation)
      if (int rc = ode_evaluate(p, o, t + h, scalars, user, K(S), use_graph, stream)) return rc;
      nfev += S;
      if (nfev_out) *nfev_out = nfev;
      double err;
      if (tab.e2) {
        if (int rc = ode_norm(p, o, y, y_new, tab.e, tab.e2, S + 1, h_abs, atol, rtol, &err, st)) return rc;
      } else {
        for (int j = 0; j <= S; ++j) c[j] = tab.e[j] * h;
        if (int rc = ode_norm(p, o, y, y_new, c, nullptr, S + 1, 0.0, atol, rtol, &err, st)) return rc;
      }
      SSDE_REQUIRE(isfinite(err), "ode_solve: the error norm is not finite at t = %.17g (step %g)", t, h);
      if (err < 1) {
        double factor = err == 0 ? kMaxFactor : fmin(kMaxFactor, kSafety * pow(err, exponent));
        if (rejected) factor = fmin(1.0, factor);
        h_abs *= factor;
        break;
      }
      h_abs *= fmax(kMinFactor, kSafety * pow(err, exponent));
      rejected = true;
    }
    t = t_new;
    p->ode_cur ^= 1;                                                   // accept: swap buffers
    y = o.y[p->ode_cur];
    y_new = o.y[p->ode_cur ^ 1];
    SSDE_HIP_CHECK(hipMemcpyAsync(K(0), K(S), row, hipMemcpyDeviceToDevice, st));   // FSAL: the last slope is the next step's first
  }
  SSDE_HIP_CHECK(hipStreamSynchronize(st));
  p->ode_inflight = 0;
  return SSDE_OK;
}

extern "C" int ssde_ode_solve(ssde_plan* p, double t0, double t1, double rtol, double atol, ssde_ode_scalars_fn scalars, void* user,
                              int32_t use_graph, int32_t max_nfev, int32_t* nfev_out, void* stream) {
  return ssde_ode_solve_method(p, SSDE_ODE_RK45, t0, t1, rtol, atol, scalars, user, use_graph, max_nfev, nfev_out, stream);
}

extern "C" int ssde_ode_state(ssde_plan* p, float* x, double* delta_logp, void* stream) {
  Ode o;
  if (int rc = ode_view(p, &o, "ode_state")) return rc;
  SSDE_REQUIRE(p->hdr.kind == SSDE_PLAN_LIKELIHOOD || !delta_logp, "ode_state: a sampler plan has no log-density terms");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double* y = o.y[p->ode_cur];
  if (x) {          // the fp32 rounding of the state, formed by the combine launch in the U-Net's input buffer
    if (int rc = ode_combine(o, y, nullptr, 0, o.y_stage, stream)) return rc;
    SSDE_HIP_CHECK(hipMemcpyAsync(x, o.x32, (size_t)o.n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (delta_logp) SSDE_HIP_CHECK(hipMemcpyAsync(delta_logp, y + o.n, (size_t)p->hdr.batch * sizeof(double), hipMemcpyDeviceToDevice, st));
  return SSDE_OK;
}

// ---- training plans (losses.FusedTrainStep: perturb | forward | loss head | backward | clip + Adam + EMA) ----
namespace {
int run_segment(ssde_plan* p, int lo, int hi, void* stream) {
  SSDE_REQUIRE(0 <= lo && lo <= hi && hi <= (int)p->ops.size(), "plan: bad segment [%d, %d)", lo, hi);
  return ssde_program_run(p->ops.data() + lo, hi - lo, stream);
}
// host scalars of a call (dropout seed word, hyper-parameters) are copied from the caller's memory: the stream is
// synchronised before returning to the caller's frame
int set_seed(ssde_plan* p, const int32_t* seed_word, hipStream_t st) {
  if (p->hdr.io[SSDE_IO_DROP_SEED] < 0) return SSDE_OK;              // a plan lowered without dropout
  SSDE_HIP_CHECK(hipMemcpyAsync(region_ptr(p, p->hdr.io[SSDE_IO_DROP_SEED]), seed_word, sizeof(int32_t), hipMemcpyHostToDevice, st));
  return SSDE_OK;
}
}  // namespace

extern "C" int ssde_train_step(ssde_plan* p, const float* batch, const float* z, const float* a, const float* s, const float* labels,
                               const float* g2, const float* hyper, uint32_t dropout_seed, float* loss_out, void* stream) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_TRAIN && p->hdr.seg[3] > 0, "train_step: not a training plan with an optimizer segment");
  SSDE_REQUIRE(hyper, "train_step: null hyper-parameters");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float), vec = (size_t)h.batch * sizeof(float);
  if (int rc = copy_in(p, SSDE_IO_BATCH, batch, img, st)) return rc;
  if (int rc = copy_in(p, SSDE_IO_Z, z, img, st)) return rc;
  if (int rc = copy_in(p, SSDE_IO_A, a, vec, st)) return rc;
  if (int rc = copy_in(p, SSDE_IO_S, s, vec, st)) return rc;
  if (int rc = copy_in(p, SSDE_IO_COND, labels, vec, st)) return rc;
  if (h.io[SSDE_IO_STD] >= 0)                                         // VP score head: score = -h / std (models/utils.py:159)
    if (int rc = copy_in(p, SSDE_IO_STD, s, vec, st)) return rc;
  if (h.io[SSDE_IO_G2] >= 0 && g2)
    if (int rc = copy_in(p, SSDE_IO_G2, g2, vec, st)) return rc;
  SSDE_REQUIRE(region_ptr(p, h.io[SSDE_IO_HYPER]), "train_step: plan has no hyper-parameter record");
  SSDE_HIP_CHECK(hipMemcpyAsync(region_ptr(p, h.io[SSDE_IO_HYPER]), hyper, 9 * sizeof(float), hipMemcpyHostToDevice, st));
  const int32_t seed_word = (int32_t)(dropout_seed & 0x7FFFFFFFu);
  if (int rc = set_seed(p, &seed_word, st)) return rc;
  SSDE_HIP_CHECK(hipStreamSynchronize(st));                           // `hyper` and `seed_word` are the caller's / this frame's
  if (int rc = run_segment(p, 0, (int)p->ops.size(), stream)) return rc;
  if (int rc = ssde_plan_refresh_weights(p, stream)) return rc;       // packed copies follow the in-place parameter update
  if (loss_out) SSDE_HIP_CHECK(hipMemcpyAsync(loss_out, region_ptr(p, h.io[SSDE_IO_LOSS]), sizeof(float), hipMemcpyDeviceToDevice, st));
  return SSDE_OK;
}

extern "C" int ssde_train_forward(ssde_plan* p, const float* x, const float* cond, const float* sigma, const float* std_,
                                  uint32_t dropout_seed, float* out, void* stream) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_TRAIN, "train_forward: not a training plan");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float), vec = (size_t)h.batch * sizeof(float);
  if (int rc = copy_in(p, SSDE_IO_X, x, img, st)) return rc;
  if (int rc = copy_in(p, SSDE_IO_COND, cond, vec, st)) return rc;
  if (h.io[SSDE_IO_SIGMA] >= 0 && h.io[SSDE_IO_SIGMA] != h.io[SSDE_IO_COND])
    if (int rc = copy_in(p, SSDE_IO_SIGMA, sigma, vec, st)) return rc;
  if (h.io[SSDE_IO_STD] >= 0)
    if (int rc = copy_in(p, SSDE_IO_STD, std_, vec, st)) return rc;
  const int32_t seed_word = (int32_t)(dropout_seed & 0x7FFFFFFFu);
  if (int rc = set_seed(p, &seed_word, st)) return rc;
  SSDE_HIP_CHECK(hipStreamSynchronize(st));
  if (int rc = run_segment(p, h.seg[0], h.seg[1], stream)) return rc;
  if (out) SSDE_HIP_CHECK(hipMemcpyAsync(out, region_ptr(p, h.io[SSDE_IO_OUT]), img, hipMemcpyDeviceToDevice, st));
  return SSDE_OK;
}

extern "C" int ssde_unet_backward(ssde_plan* p, const float* dout, float* dx, float* dparams, void* stream) {
  SSDE_REQUIRE(p && p->hdr.kind == SSDE_PLAN_TRAIN && dout, "unet_backward: not a training plan / null cotangent");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ssde_plan_header& h = p->hdr;
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width * sizeof(float);
  if (int rc = copy_in(p, SSDE_IO_GOUT, dout, img, st)) return rc;
  if (int rc = run_segment(p, h.seg[2], h.seg[3] > 0 ? h.seg[3] : (int)p->ops.size(), stream)) return rc;
  if (dx) {
    SSDE_REQUIRE(region_ptr(p, h.io[SSDE_IO_GX]), "unet_backward: the plan was exported without the input gradient");
    SSDE_HIP_CHECK(hipMemcpyAsync(dx, region_ptr(p, h.io[SSDE_IO_GX]), img, hipMemcpyDeviceToDevice, st));
  }
  if (dparams) {
    SSDE_REQUIRE(region_ptr(p, h.io[SSDE_IO_GRAD]) && h.n_flat > 0, "unet_backward: the plan carries no parameter gradients");
    SSDE_HIP_CHECK(hipMemcpyAsync(dparams, region_ptr(p, h.io[SSDE_IO_GRAD]), (size_t)h.n_flat * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return SSDE_OK;
}

extern "C" int ssde_plan_copy_io(ssde_plan* p, int32_t slot, void* buf, int64_t bytes, int32_t to_plan, void* stream) {
  SSDE_REQUIRE(p && buf && slot >= 0 && slot < SSDE_IO_SLOTS && bytes >= 0, "plan_copy_io: bad args");
  void* reg = region_ptr(p, p->hdr.io[slot]);
  SSDE_REQUIRE(reg, "plan_copy_io: the plan has no I/O slot %d", slot);
  SSDE_REQUIRE(bytes <= p->regions[p->hdr.io[slot]].bytes, "plan_copy_io: %lld bytes exceed slot %d (%lld)", (long long)bytes, slot,
               (long long)p->regions[p->hdr.io[slot]].bytes);
  SSDE_HIP_CHECK(hipMemcpyAsync(to_plan ? reg : buf, to_plan ? buf : reg, (size_t)bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return SSDE_OK;
}
