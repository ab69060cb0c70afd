/* A host WITHOUT Python for the probability-flow ODE: loads an ODE plan blob (plan_export.export_ode_plan), integrates it
 * with the library's adaptive RK45 driver (include/ssde.h: ssde_ode_reset / ssde_ode_solve / ssde_ode_state) and writes the
 * final state.  What the reference does with scipy.integrate.solve_ivp around the network (sampling.py:449-483,
 * likelihood.py:69-111); the denoising step, the inverse scaler, the prior log-density and the bits/dim constant are the
 * host's own arithmetic on these outputs and are not done here.
 *
 *   ode_host sample     <plan.blob> <sde> <p0> <p1> <t0> <t1> <rtol=atol> <use_graph> <x0.f32> <x_out.f32>
 *   ode_host likelihood <plan.blob> <sde> <p0> <p1> <t0> <t1> <rtol=atol> <use_graph> <x0.f32> <x_out.f32> <probe.f32> <dlogp_out.f64>
 *       <sde> = ve (p0, p1 = sigma_min, sigma_max) | vp | subvp (p0, p1 = beta_min, beta_max)
 *
 * The library holds no SDE formulas: `scalars` below is the worked example of the callback for continuously-trained
 * models.  Plain C; under the test-only CPU emulator the same source is built against a small shim (HOST_IS_DEVICE). */
#define _POSIX_C_SOURCE 200112L   /* clock_gettime */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

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

/* label, second, a, g2 at time t in fp32, as the SDE classes compute them for a continuously-trained model:
 *   f(x, t) = a x and g(t):   sde_lib.py VESDE.sde / VPSDE.sde / subVPSDE.sde
 *   marginal std:             sde_lib.py marginal_prob of the same classes
 *   label:                    models/utils.py get_score_fn -- t * 999 for VP / sub-VP, sigma(t) for VE
 *   second:                   the std the VP / sub-VP score head divides by; unused by a continuous VE model */
typedef struct { int kind; float p0, p1; } sde_params;   /* kind 0 = ve, 1 = vp, 2 = subvp */

static int scalars(double t64, void* user, float out[4]) {
  const sde_params* s = (const sde_params*)user;
  const float t = (float)t64;
  if (s->kind == 0) {
    const float sigma = s->p0 * powf(s->p1 / s->p0, t);
    const float g = sigma * sqrtf((float)(2 * (log(s->p1) - log(s->p0))));
    out[0] = sigma; out[1] = sigma; out[2] = 0.f; out[3] = g * g;
    return 0;
  }
  const float beta_t = s->p0 + t * (s->p1 - s->p0);
  const float lmc = -0.25f * (t * t) * (s->p1 - s->p0) - 0.5f * t * s->p0;
  float g;
  if (s->kind == 1) {
    g = sqrtf(beta_t);
    out[1] = sqrtf(1.f - expf(2.f * lmc));
  } else {
    const float discount = 1.f - expf(-2 * s->p0 * t - (s->p1 - s->p0) * (t * t));
    g = sqrtf(beta_t * discount);
    out[1] = 1 - expf(2.f * lmc);
  }
  out[0] = t * 999;
  out[2] = -0.5f * beta_t;
  out[3] = g * g;
  return 0;
}

static void* read_file(const char* path, size_t* bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  void* v = malloc((size_t)n);
  if (fread(v, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read %s\n", path); exit(2); }
  fclose(f);
  *bytes = (size_t)n;
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
  const int lik = argc > 1 && strcmp(argv[1], "likelihood") == 0;
  if (argc < (lik ? 14 : 12) || (!lik && strcmp(argv[1], "sample") != 0)) {
    fprintf(stderr, "usage: %s sample|likelihood plan.blob ve|vp|subvp p0 p1 t0 t1 tol use_graph x0.f32 x_out.f32 [probe.f32 dlogp_out.f64]\n", argv[0]);
    return 2;
  }
  sde_params sde;
  sde.kind = strcmp(argv[3], "ve") == 0 ? 0 : strcmp(argv[3], "vp") == 0 ? 1 : strcmp(argv[3], "subvp") == 0 ? 2 : -1;
  if (sde.kind < 0) { fprintf(stderr, "unknown sde %s\n", argv[3]); return 2; }
  sde.p0 = (float)atof(argv[4]); sde.p1 = (float)atof(argv[5]);
  const double t0 = atof(argv[6]), t1 = atof(argv[7]), tol = atof(argv[8]);
  const int use_graph = atoi(argv[9]);

  ssde_plan* plan = NULL;
  CHECK(ssde_plan_load_file(argv[2], &plan));
  ssde_plan_header h;
  CHECK(ssde_plan_info(plan, &h));
  if (h.kind != (lik ? SSDE_PLAN_LIKELIHOOD : SSDE_PLAN_ODE)) { fprintf(stderr, "plan kind %d does not fit mode %s\n", h.kind, argv[1]); return 2; }
  const size_t img = (size_t)h.batch * h.channels * h.height * h.width;
  size_t bytes;
  float* x0 = (float*)read_file(argv[10], &bytes);
  if (bytes != img * 4) { fprintf(stderr, "x0 has %zu bytes, the plan is [%d,%d,%d,%d]\n", bytes, h.batch, h.channels, h.height, h.width); return 2; }
  void *dx, *dprobe = NULL, *ddl = NULL, *stream = NULL;
  if (dev_alloc(&dx, img * 4) || h2d(dx, x0, img * 4)) { fprintf(stderr, "upload failed\n"); return 1; }
  if (lik) {
    float* probe = (float*)read_file(argv[12], &bytes);
    if (bytes != img * 4) { fprintf(stderr, "the probe has %zu bytes\n", bytes); return 2; }
    if (dev_alloc(&dprobe, img * 4) || h2d(dprobe, probe, img * 4) || dev_alloc(&ddl, (size_t)h.batch * 8)) { fprintf(stderr, "upload failed\n"); return 1; }
  }
  if (use_graph && make_stream(&stream)) { fprintf(stderr, "stream creation failed\n"); return 1; }

  CHECK(ssde_ode_reset(plan, (const float*)dx, (const float*)dprobe, stream));
  int32_t nfev = 0;
  struct timespec a, b;
  clock_gettime(CLOCK_MONOTONIC, &a);
  CHECK(ssde_ode_solve(plan, t0, t1, tol, tol, scalars, &sde, use_graph, 0, &nfev, stream));
  clock_gettime(CLOCK_MONOTONIC, &b);
  CHECK(ssde_ode_state(plan, (float*)dx, (double*)ddl, stream));
  if (dev_sync()) { fprintf(stderr, "device synchronisation failed\n"); return 1; }
  float* x = (float*)malloc(img * 4);
  if (d2h(x, dx, img * 4) || write_file(argv[11], x, img * 4)) return 1;
  if (lik) {
    double* dl = (double*)malloc((size_t)h.batch * 8);
    if (d2h(dl, ddl, (size_t)h.batch * 8) || write_file(argv[13], dl, (size_t)h.batch * 8)) return 1;
  }
  printf("ode_host %s: %d ops per evaluation, [%d,%d,%d,%d], t %g -> %g, nfev %d, solve %.6f s\n", argv[1], h.n_ops, h.batch, h.channels,
         h.height, h.width, t0, t1, (int)nfev, (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec));
  CHECK(ssde_plan_destroy(plan));
  return 0;
}
