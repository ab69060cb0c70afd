/* A host WITHOUT Python for controllable generation: loads a sampler plan blob whose iteration contains the data-consistency
 * projection (plan_export.export_pc_plan of the engine behind get_pc_inpainter / get_pc_colorizer), hands it the known data
 * and the mask, forms the reference's start state from a prior sample, runs the predictor-corrector iterations and writes
 * x_mean (include/ssde.h: ssde_pc_set_known / ssde_pc_reset_known / ssde_pc_run / ssde_pc_state).  What the reference does
 * in controllable_generation.py:54-83 (inpainting) and :146-180 (colorization); the inverse scaler is the host's own
 * arithmetic on the output and is not done here.
 *
 *   control_host <plan.blob> <data.f32> <mask.f32 | -> <prior.f32> <seed> <iterations> <use_graph> <x_mean_out.f32> [noises.f32]
 *       data:   [B,C,H,W] in the model's input scaling (colorization: the grey image repeated over R, G, B)
 *       mask:   [B,C,H,W] of 0 / 1, or "-" for the task's own mask (colorization)
 *       noises: plans exported with with_rng=False only: [iterations][4][B,C,H,W], per iteration the corrector, predictor,
 *               projection-after-corrector and projection-after-predictor noise (a stage the plan lacks is skipped)
 *
 * Plain C; under the test-only CPU emulator the same source is built against a small shim (HOST_IS_DEVICE). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssde.h"

#ifdef HOST_IS_DEVICE
static int dev_alloc(void** p, size_t n) { *p = malloc(n ? n : 1); return *p ? 0 : 1; }
static int h2d(void* d, const void* s, size_t n) { memcpy(d, s, n); return 0; }
static int d2h(void* d, const void* s, size_t n) { memcpy(d, s, n); return 0; }
static int dev_sync(void) { return 0; }
static int make_stream(void** s) { *s = NULL; return 0; }
#else
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
static int dev_alloc(void** p, size_t n) { return hipMalloc(p, n) != hipSuccess; }
static int h2d(void* d, const void* s, size_t n) { return hipMemcpy(d, s, n, hipMemcpyHostToDevice) != hipSuccess; }
static int d2h(void* d, const void* s, size_t n) { return hipMemcpy(d, s, n, hipMemcpyDeviceToHost) != hipSuccess; }
static int dev_sync(void) { return hipDeviceSynchronize() != hipSuccess; }
static int make_stream(void** s) { return hipStreamCreate((hipStream_t*)s) != hipSuccess; }   /* graph capture needs a non-default stream */
#endif

static float* read_f32(const char* path, size_t want) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (bytes < 0 || (size_t)bytes != want * 4) { fprintf(stderr, "%s has %ld bytes, expected %zu\n", path, bytes, want * 4); exit(2); }
  float* v = (float*)malloc((size_t)bytes ? (size_t)bytes : 1);
  if (fread(v, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "short read %s\n", path); exit(2); }
  fclose(f);
  return v;
}

static int write_file(const char* path, const void* v, size_t bytes) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(v, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path); return 1; }
  return fclose(f) != 0;
}

#define CHECK(call)                                                                  \
  do {                                                                               \
    int rc_ = (call);                                                                \
    if (rc_) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ssde_last_error()); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: %s plan.blob data.f32 mask.f32|- prior.f32 seed iterations use_graph x_mean_out.f32 [noises.f32]\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[5], NULL, 10);
  const int iterations = atoi(argv[6]), use_graph = atoi(argv[7]);
  const int own_mask = strcmp(argv[3], "-") == 0;

  ssde_plan* plan = NULL;
  CHECK(ssde_plan_load_file(argv[1], &plan));
  ssde_plan_header h;
  CHECK(ssde_plan_info(plan, &h));
  const int kind = ssde_pc_projection(plan);
  if (kind < 0) { fprintf(stderr, "ssde_pc_projection failed (%d): %s\n", kind, ssde_last_error()); return 1; }
  if (kind == SSDE_PC_PROJ_NONE) { fprintf(stderr, "the plan's iteration has no projection: an unconditional sampler\n"); return 2; }
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width;
  float* data = read_f32(argv[2], img);
  float* mask = own_mask ? NULL : read_f32(argv[3], img);
  float* prior = read_f32(argv[4], img);
  float* noises = argc > 9 ? read_f32(argv[9], (size_t)iterations * 4 * img) : NULL;
  void *ddata, *dmask = NULL, *dprior, *dnoise = NULL, *dout, *stream = NULL;
  if (dev_alloc(&ddata, img * 4) || h2d(ddata, data, img * 4) || dev_alloc(&dprior, img * 4) || h2d(dprior, prior, img * 4) ||
      dev_alloc(&dout, img * 4) || (mask && (dev_alloc(&dmask, img * 4) || h2d(dmask, mask, img * 4))) ||
      (noises && dev_alloc(&dnoise, 4 * img * 4))) {
    fprintf(stderr, "upload failed\n");
    return 1;
  }
  if (use_graph && make_stream(&stream)) { fprintf(stderr, "stream creation failed\n"); return 1; }

  CHECK(ssde_pc_set_known(plan, (const float*)ddata, (const float*)dmask, stream));
  CHECK(ssde_pc_reset_known(plan, (const float*)dprior, seed, stream));
  if (!noises) {
    CHECK(ssde_pc_run(plan, iterations, use_graph, stream));
  } else {
    /* a sampler without a corrector (or without a predictor) has no buffer for that stage's noise: found out once */
    int has[4] = {1, 1, 1, 1};
    for (int i = 0; i < iterations; ++i) {
      if (dev_sync() || h2d(dnoise, noises + (size_t)i * 4 * img, 4 * img * 4)) { fprintf(stderr, "noise upload failed\n"); return 1; }
      for (int k = 0; k < 4; ++k) {
        if (!has[k]) continue;
        const int rc = ssde_pc_set_noise(plan, k, (const float*)dnoise + (size_t)k * img, stream);
        if (rc && i == 0 && k < 2 && strstr(ssde_last_error(), "stage")) { has[k] = 0; continue; }
        if (rc) { fprintf(stderr, "ssde_pc_set_noise(%d) failed (%d): %s\n", k, rc, ssde_last_error()); return 1; }
      }
      CHECK(ssde_pc_run(plan, 1, use_graph, stream));
    }
  }
  CHECK(ssde_pc_state(plan, NULL, (float*)dout, stream));
  if (dev_sync()) { fprintf(stderr, "device synchronisation failed\n"); return 1; }
  float* out = (float*)malloc(img * 4);
  if (d2h(out, dout, img * 4) || write_file(argv[8], out, img * 4)) return 1;
  double sum = 0.0;
  for (size_t i = 0; i < img; ++i) sum += (double)out[i];
  printf("control_host: %s, %d ops per iteration, [%d,%d,%d,%d], %d iterations (%s), checksum %.9g\n",
         kind == SSDE_PC_PROJ_COLOR ? "colorization" : "inpainting", h.n_ops, h.batch, h.channels, h.height, h.width, iterations,
         use_graph ? "graph" : "eager", sum);
  CHECK(ssde_plan_destroy(plan));
  return 0;
}
