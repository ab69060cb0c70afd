// HBM-bound glue kernels of the hot path: time embeddings, NCHW<->NHWC boundary,
// fused bias+activation, and the predictor/corrector state update.
// Reference lines are cited per kernel.  Arithmetic that the parity tests compare
// bit-for-bit against the reference's torch expression order uses ssde_fmul_rn /
// ssde_fadd_rn (ssde_common.h) so hipcc cannot contract it into FMAs.
#include "ssde_common.h"
#include <math.h>
#include <string.h>
#include <rocrand/rocrand_kernel.h>

namespace {

// ---- embeddings -----------------------------------------------------------------
// kind 0: GaussianFourierProjection(log(sigma)) -- layerspp.py:39-41 via ncsnpp.py:239:
//         x_proj = log(sigma) * W * 2 * pi ; out = [sin(x_proj), cos(x_proj)]
// kind 1: get_timestep_embedding -- layers.py:515-529: arg = t * freq[j] (freq table
//         exp(-j*log(1e4)/(half-1)) is built on the host exactly as the reference does)
__global__ void embed_kernel(const float* __restrict__ cond, const float* __restrict__ w, float* __restrict__ dst,
                             int n, int dim, int kind) {
  const int half = dim >> 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * half) return;
  const int b = idx / half, j = idx - b * half;
  float arg;
  if (kind == 0) {
    const float x = logf(cond[b]);
    arg = ssde_fmul_rn(ssde_fmul_rn(ssde_fmul_rn(x, w[j]), 2.0f), 3.14159265358979323846f);
  } else {
    arg = ssde_fmul_rn(cond[b], w[j]);
  }
  dst[(size_t)b * dim + j] = sinf(arg);
  dst[(size_t)b * dim + half + j] = cosf(arg);
}

// ---- layout boundary ----------------------------------------------------------------
// x = 2x - 1 for un-centred data is folded in (ncsnpp.py:259-261).
__global__ void to_nhwc_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int c, int h, int w,
                               int c_pad, float a, float b, int mode, const float* __restrict__ vec) {
  const size_t total = (size_t)n * h * w;
  const size_t hw = (size_t)h * w;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t img = idx / hw, pix = idx - img * hw;
    float f = a;
    if (mode == 1) f = ssde_fdiv_rn(a, vec[img]);
    else if (mode == 2) f = ssde_fdiv_rn(-a, vec[img]);
    for (int ch = 0; ch < c_pad; ++ch) {
      float v = 0.f;
      if (ch < c) v = ssde_fadd_rn(ssde_fmul_rn(f, src[(img * c + ch) * hw + pix]), b);
      dst[idx * c_pad + ch] = v;
    }
  }
}

// mode 1: h / sigma (scale_by_sigma, ncsnpp.py:377-379); mode 2: -h / std (models/utils.py:159)
__global__ void to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int c, int h, int w,
                               int c_src, int mode, const float* __restrict__ v, float alpha, int accumulate) {
  const size_t hw = (size_t)h * w;
  const size_t total = (size_t)n * c * hw;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = idx % hw;
    const size_t t = idx / hw;
    const int ch = (int)(t % c);
    const size_t img = t / c;
    float x = src[(img * hw + pix) * c_src + ch];
    if (mode == 1) x = ssde_fdiv_rn(x, v[img]);
    else if (mode == 2) x = ssde_fdiv_rn(-x, v[img]);
    if (alpha != 1.0f) x = ssde_fmul_rn(alpha, x);
    dst[idx] = accumulate ? dst[idx] + x : x;
  }
}

// ---- fused bias + activation (op/fused_bias_act_kernel.cu:18-49, forward only) ------
__global__ void bias_act_kernel(const float* __restrict__ src, const float* __restrict__ bias, float* __restrict__ dst,
                                size_t numel, int channels, int inner, int act, float alpha, float scale, int grad,
                                const float* __restrict__ ref) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < numel; idx += (size_t)gridDim.x * blockDim.x) {
    float x = src[idx];
    if (bias) x += bias[(idx / inner) % channels];
    if (grad == 1) {                       // gradient mode: slope chosen by the sign of the forward output
      if (act == 3) x = ref[idx] > 0.f ? x : x * alpha;
    } else if (act == 3) {
      x = x > 0.f ? x : x * alpha;
    }
    dst[idx] = x * scale;
  }
}

// ---- per-sample sum of squares (sampling.py:276-277) ----------------------------------
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                    float* __restrict__ oa, float* __restrict__ ob, int per) {
  SSDE_LDS(smem);
  float (*red)[4] = reinterpret_cast<float (*)[4]>(smem);   // [2][4]
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* pa = a + (size_t)n * per;
  const float* pb = b ? b + (size_t)n * per : nullptr;
  float sa = 0.f, sb = 0.f;
  for (int i = tid; i < per; i += 256) {
    const float x = pa[i]; sa += x * x;
    if (pb) { const float y = pb[i]; sb += y * y; }
  }
  sa = ssde_wave_sum(sa); sb = ssde_wave_sum(sb);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sa; red[1][tid >> 6] = sb; }
  __syncthreads();
  if (tid == 0) {
    oa[n] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    if (pb) ob[n] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// ---- standard-normal noise, Philox4x32-10 through rocRAND's device API ----------------
// (the reference draws torch.randn_like on the device, sampling.py:197,275)
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ dst, size_t numel, unsigned long long seed,
                                                    const int* __restrict__ step_ptr, int stream_id,
                                                    const unsigned long long* __restrict__ seed_ptr) {
  if (seed_ptr) seed += *seed_ptr;
  const unsigned long long step = step_ptr ? (unsigned long long)(*step_ptr) : 0ull;
  const unsigned long long gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  rocrand_state_philox4x32_10 st;
  // one subsequence per lane; (step, stream) select disjoint 2^32-long offsets inside it
  rocrand_init(seed, gid, ((step * 16ull + (unsigned long long)stream_id) << 32), &st);
  const size_t n4 = numel >> 2;
  for (size_t i = gid; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 r = rocrand_normal4(&st);
    *reinterpret_cast<float4*>(dst + i * 4) = r;
  }
  if (gid == 0) {
    for (size_t i = n4 * 4; i < numel; ++i) dst[i] = rocrand_normal(&st);
  }
}

// ---- Langevin corrector update (sampling.py:273-280) -----------------------------------
//   grad_norm = mean_n ||g_n|| ; noise_norm = mean_n ||z_n||
//   step = (snr * noise_norm / grad_norm)^2 * 2 * alpha
//   x_mean = x + step * g ; x = x_mean + sqrt(step * 2) * z
__global__ __launch_bounds__(256) void langevin_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                       const float* __restrict__ g, const float* __restrict__ z,
                                                       const float* __restrict__ gss, const float* __restrict__ zss,
                                                       const float* __restrict__ alpha_tab, const int* __restrict__ step_ptr,
                                                       int n, size_t numel, float snr) {
  SSDE_LDS(smem);
  float (*red)[4] = reinterpret_cast<float (*)[4]>(smem);   // [2][4]
  float* s_step = smem + 8;
  const int tid = threadIdx.x;
  float sg = 0.f, sz = 0.f;
  for (int i = tid; i < n; i += 256) { sg += sqrtf(gss[i]); sz += sqrtf(zss[i]); }
  sg = ssde_wave_sum(sg); sz = ssde_wave_sum(sz);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sg; red[1][tid >> 6] = sz; }
  __syncthreads();
  if (tid == 0) {
    const float gn = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)n;
    const float zn = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)n;
    const float alpha = alpha_tab ? alpha_tab[step_ptr ? *step_ptr : 0] : 1.0f;
    const float r = ssde_fdiv_rn(ssde_fmul_rn(snr, zn), gn);
    const float step = ssde_fmul_rn(ssde_fmul_rn(ssde_fmul_rn(r, r), 2.0f), alpha);
    s_step[0] = step;
    s_step[1] = sqrtf(ssde_fmul_rn(step, 2.0f));
  }
  __syncthreads();
  const float step = s_step[0], nz = s_step[1];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + tid; i < numel; i += (size_t)gridDim.x * blockDim.x) {
    const float xm = ssde_fadd_rn(x[i], ssde_fmul_rn(step, g[i]));
    x_mean[i] = xm;
    x[i] = ssde_fadd_rn(xm, ssde_fmul_rn(nz, z[i]));
  }
}

// ---- predictor update: x_mean = a*x + b*score ; x = x_mean + c*z ------------------------
// ReverseDiffusionPredictor on a VE SDE (sampling.py:195-200 with sde_lib.py:102-107,246-254):
// a = 1, b = G^2, c = G.  EulerMaruyama / VP variants supply their own (a, b, c) rows.
__global__ __launch_bounds__(256) void predictor_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                        const float* __restrict__ s, const float* __restrict__ z,
                                                        const float* __restrict__ coef, const int* __restrict__ step_ptr,
                                                        size_t numel) {
  const int st = step_ptr ? *step_ptr : 0;
  const float a = coef[3 * st], b = coef[3 * st + 1], c = coef[3 * st + 2];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (size_t)gridDim.x * blockDim.x) {
    const float xa = (a == 1.0f) ? x[i] : ssde_fmul_rn(a, x[i]);
    const float xm = ssde_fadd_rn(xa, ssde_fmul_rn(b, s[i]));
    x_mean[i] = xm;
    x[i] = z ? ssde_fadd_rn(xm, ssde_fmul_rn(c, z[i])) : xm;
  }
}

// the same update with per-sample coefficient vectors (ssde_sample_update: the generic path of sampling.py)
__global__ __launch_bounds__(256) void sample_update_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                            const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                            float* __restrict__ x_mean, float* __restrict__ x_out, int per, size_t numel) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (size_t)gridDim.x * blockDim.x) {
    const size_t n = i / (size_t)per;
    float xm = a ? ssde_fmul_rn(a[n], x[i]) : x[i];
    if (y) xm = ssde_fadd_rn(xm, ssde_fmul_rn(b[n], y[i]));
    x_mean[i] = xm;
    x_out[i] = z ? ssde_fadd_rn(xm, ssde_fmul_rn(c[n], z[i])) : xm;
  }
}

// ---- controllable-generation projection (controllable_generation.py:44-52, 136-144) ------
// Elementwise form (inpainting): x = x (1 - mask) + (m D + z s) mask ; x_mean = x (1 - mask) + m D mask.
__global__ __launch_bounds__(256) void project_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                      const float* __restrict__ data, const float* __restrict__ mask,
                                                      const float* __restrict__ z, const float* __restrict__ coef,
                                                      const int* __restrict__ step_ptr, size_t numel) {
  const int st = step_ptr ? *step_ptr : 0;
  const float m = coef[2 * st], s = coef[2 * st + 1];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (size_t)gridDim.x * blockDim.x) {
    const float mk = mask[i], inv = ssde_fsub_rn(1.0f, mk);
    const float mean = (m == 1.0f) ? data[i] : ssde_fmul_rn(m, data[i]);
    const float known = ssde_fadd_rn(mean, ssde_fmul_rn(z[i], s));
    const float xn = ssde_fadd_rn(ssde_fmul_rn(x[i], inv), ssde_fmul_rn(known, mk));
    x[i] = xn;
    x_mean[i] = ssde_fadd_rn(ssde_fmul_rn(xn, inv), ssde_fmul_rn(mean, mk));
  }
}

// Colour-space form (colorization): one thread per pixel, the three channels pass through M / M^-1 in registers.
struct SsdeMat3 { float m[9]; };
__device__ __forceinline__ void mat3_apply(const SsdeMat3& a, const float (&v)[3], float (&o)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) o[j] = fmaf(v[2], a.m[6 + j], fmaf(v[1], a.m[3 + j], ssde_fmul_rn(v[0], a.m[j])));
}
__global__ __launch_bounds__(256) void project_color_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                            const float* __restrict__ data, const float* __restrict__ mask,
                                                            const float* __restrict__ z, const float* __restrict__ coef,
                                                            const int* __restrict__ step_ptr, int n, int hw,
                                                            SsdeMat3 M, SsdeMat3 invM) {
  const int st = step_ptr ? *step_ptr : 0;
  const float m = coef[2 * st], s = coef[2 * st + 1];
  const size_t pixels = (size_t)n * hw;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (size_t)gridDim.x * blockDim.x) {
    const size_t base = (p / hw) * 3 * (size_t)hw + (p % hw);
    float xv[3], y[3], mean[3], mk[3], yn[3], xn[3], y2[3], ym[3], xm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xv[c] = x[base + (size_t)c * hw];
    mat3_apply(M, xv, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t i = base + (size_t)c * hw;
      mk[c] = mask[i];
      mean[c] = (m == 1.0f) ? data[i] : ssde_fmul_rn(m, data[i]);
      const float known = ssde_fadd_rn(mean[c], ssde_fmul_rn(z[i], s));
      yn[c] = ssde_fadd_rn(ssde_fmul_rn(y[c], ssde_fsub_rn(1.0f, mk[c])), ssde_fmul_rn(known, mk[c]));
    }
    mat3_apply(invM, yn, xn);
    mat3_apply(M, xn, y2);
#pragma unroll
    for (int c = 0; c < 3; ++c) ym[c] = ssde_fadd_rn(ssde_fmul_rn(y2[c], ssde_fsub_rn(1.0f, mk[c])), ssde_fmul_rn(mean[c], mk[c]));
    mat3_apply(invM, ym, xm);
#pragma unroll
    for (int c = 0; c < 3; ++c) { x[base + (size_t)c * hw] = xn[c]; x_mean[base + (size_t)c * hw] = xm[c]; }
  }
}

// ---- what controllable generation does before the loop (controllable_generation.py:73, :170-172; ssde_project_prepare) ----
// Identity form: known = data ; x = x_mean = data mask + prior (1 - mask), torch's operation order.  data == nullptr: known is
// read, not written.  No __restrict__: mask_out may alias mask.
__global__ __launch_bounds__(256) void project_prepare_kernel(const float* data, const float* mask, const float* prior, float* known,
                                                              float* mask_out, float* x, float* x_mean, size_t numel) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (size_t)gridDim.x * blockDim.x) {
    const float mk = mask[i];
    const float kn = data ? data[i] : known[i];
    if (data && known) known[i] = kn;
    if (mask_out) mask_out[i] = mk;
    if (prior) {
      const float xn = ssde_fadd_rn(ssde_fmul_rn(kn, mk), ssde_fmul_rn(prior[i], ssde_fsub_rn(1.0f, mk)));
      x[i] = xn;
      if (x_mean) x_mean[i] = xn;
    }
  }
}

// Colour-space form: one thread per pixel.  known = M data -- project_color_kernel's product, were `data` the state --, the
// prior is masked in PIXEL space before it is decoupled (:170-172), x = invM (known mask + M (prior (1 - mask))).
// mask == nullptr: the colorizer's own mask, 1 on the grey channel (get_mask, :148-151).
__global__ __launch_bounds__(256) void project_prepare_color_kernel(const float* data, const float* mask, const float* prior, float* known,
                                                                    float* mask_out, float* x, float* x_mean, int n, int hw,
                                                                    SsdeMat3 M, SsdeMat3 invM) {
  const size_t pixels = (size_t)n * hw;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (size_t)gridDim.x * blockDim.x) {
    const size_t base = (p / hw) * 3 * (size_t)hw + (p % hw);
    float d[3], kn[3], mk[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t i = base + (size_t)c * hw;
      mk[c] = mask ? mask[i] : (c == 0 ? 1.0f : 0.0f);
      if (data) d[c] = data[i];
      else kn[c] = known[i];
    }
    if (data) mat3_apply(M, d, kn);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t i = base + (size_t)c * hw;
      if (data && known) known[i] = kn[c];
      if (mask_out) mask_out[i] = mk[c];
    }
    if (prior) {
      float pm[3], ap[3], y[3], xn[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) pm[c] = ssde_fmul_rn(prior[base + (size_t)c * hw], ssde_fsub_rn(1.0f, mk[c]));
      mat3_apply(M, pm, ap);
#pragma unroll
      for (int c = 0; c < 3; ++c) y[c] = ssde_fadd_rn(ssde_fmul_rn(kn[c], mk[c]), ap[c]);
      mat3_apply(invM, y, xn);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        x[base + (size_t)c * hw] = xn[c];
        if (x_mean) x_mean[base + (size_t)c * hw] = xn[c];
      }
    }
  }
}

__global__ void fill_kernel(float* __restrict__ dst, const float* __restrict__ tab, const int* __restrict__ step_ptr, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = tab[step_ptr ? *step_ptr : 0];
}

__global__ void step_inc_kernel(int* step_ptr, int delta) { *step_ptr += delta; }

// ---- channel concatenation as a tensor (layerspp.Combine with method 'cat', layerspp.py:52-55) -----------------------
// dst[r, :] = [p0[r, :], p1[r, :]] over rows r = (image, pixel); q0 / q1: channel quads per row of p0 / p1.  One 16-byte load
// and one 16-byte store per quad, grid-stride; a copy, so the bits are the sources'.
__global__ __launch_bounds__(256) void concat_kernel(const float4* __restrict__ p0, const float4* __restrict__ p1,
                                                     float4* __restrict__ dst, size_t rows, int q0, int q1) {
  const size_t qt = (size_t)(q0 + q1), total = rows * qt;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / qt;
    const int q = (int)(i - r * qt);
    dst[i] = q < q0 ? p0[r * q0 + q] : p1[r * q1 + (q - q0)];
  }
}

inline unsigned grid_for(size_t total, int block = 256, unsigned cap = 256 * 16) {
  size_t b = (total + block - 1) / block;
  if (b < 1) b = 1;
  return (unsigned)(b > cap ? cap : b);
}

}  // namespace

extern "C" int ssde_embed(const ssde_embed_args* a, void* stream) {
  SSDE_REQUIRE(a && a->cond && a->w && a->dst, "embed: null args");
  SSDE_REQUIRE(a->n > 0 && a->dim > 0 && a->dim % 2 == 0 && (a->kind == 0 || a->kind == 1), "embed: bad shape/kind");
  const int tot = a->n * (a->dim / 2);
  hipLaunchKernelGGL(embed_kernel, dim3(ssde_cdiv(tot, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     a->cond, a->w, a->dst, a->n, a->dim, a->kind);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_to_nhwc(const ssde_to_nhwc_args* a, void* stream) {
  SSDE_REQUIRE(a && a->src && a->dst && a->n > 0 && a->c > 0 && a->c_pad >= a->c, "to_nhwc: bad args");
  SSDE_REQUIRE(a->mode == 0 || a->v, "to_nhwc: per-sample vector missing");
  hipLaunchKernelGGL(to_nhwc_kernel, dim3(grid_for((size_t)a->n * a->h * a->w)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a->src, a->dst, a->n, a->c, a->h, a->w, a->c_pad, a->a, a->b,
                     a->mode, a->v);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_to_nchw(const ssde_to_nchw_args* a, void* stream) {
  SSDE_REQUIRE(a && a->src && a->dst && a->n > 0 && a->c > 0 && a->c_src >= a->c, "to_nchw: bad args");
  SSDE_REQUIRE(a->mode == 0 || a->v, "to_nchw: per-sample vector missing");
  hipLaunchKernelGGL(to_nchw_kernel, dim3(grid_for((size_t)a->n * a->c * a->h * a->w)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a->src, a->dst, a->n, a->c, a->h, a->w, a->c_src, a->mode, a->v,
                     a->alpha == 0.f ? 1.0f : a->alpha, a->accumulate);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_fused_bias_act(const ssde_bias_act_args* a, void* stream) {
  SSDE_REQUIRE(a && a->src && a->dst && a->numel >= 0, "fused_bias_act: bad args");
  SSDE_REQUIRE(a->act == 1 || a->act == 3, "fused_bias_act: act must be 1 (linear) or 3 (leaky relu)");
  SSDE_REQUIRE(!a->bias || (a->channels > 0 && a->inner > 0), "fused_bias_act: bad bias geometry");
  SSDE_REQUIRE(a->grad == 0 || (a->grad == 1 && a->ref), "fused_bias_act: grad must be 0 or 1 (with ref)");
  if (a->numel == 0) return SSDE_OK;
  hipLaunchKernelGGL(bias_act_kernel, dim3(grid_for((size_t)a->numel)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     a->src, a->bias, a->dst, (size_t)a->numel, a->channels, a->inner, a->act, a->alpha, a->scale, a->grad, a->ref);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_sumsq(const ssde_sumsq_args* a, void* stream) {
  SSDE_REQUIRE(a && a->a && a->out_a && a->n > 0 && a->per > 0, "sumsq: bad args");
  SSDE_REQUIRE(!a->b || a->out_b, "sumsq: out_b missing");
  hipLaunchKernelGGL(sumsq_kernel, dim3(a->n), dim3(256), 64, static_cast<hipStream_t>(stream),
                     a->a, a->b, a->out_a, a->out_b, a->per);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

// ---- explicit Runge-Kutta stage arithmetic for the probability-flow ODE sampler / likelihood (sampling.py:466-475,
// likelihood.py:90-99: scipy.integrate.solve_ivp on fp64 numpy state in the reference; its RK23, RK45 and DOP853).  The
// fp64 state and the stage slopes K_j (up to 13 rows) live on the device; one launch forms a stage argument (and its fp32
// copy, the U-Net input: the reference casts the state to float32 per evaluation, models/utils.py:186-188), one launch +
// a fixed-order finish form scipy's error norm -- the only scalar the host reads per step.  One kernel each for every
// method: the launcher passes the rows with a non-zero coefficient, in ascending order, so a row a method never fills
// (or fills later in the step) is not read.  Adding a row times zero changes no bit of a finite sum, so leaving it out
// gives what the seven-row kernels of the Dormand-Prince driver gave.
struct rk_terms {
  int count;                          // rows read
  int row[SSDE_RK_MAX_ROWS];          // their indices into K, ascending
  double c[SSDE_RK_MAX_ROWS];         // coefficient per row read
  double c2[SSDE_RK_MAX_ROWS];        // pair form of the error norm: the second coefficient row (E3 beside E5)
};

__global__ __launch_bounds__(256) void rk_combine_kernel(const double* __restrict__ y, const double* __restrict__ k, size_t n, rk_terms c,
                                                         double* __restrict__ dst, float* __restrict__ dst32, size_t n32) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    // scipy: dy = np.dot(K[:s].T, a[:s]) * h ; y + dy   -- here a_j * h is folded on the host, summed j = 0, 1, ...
    double dy = 0.0;
    for (int t = 0; t < c.count; ++t) dy += k[(size_t)c.row[t] * n + i] * c.c[t];
    const double v = y[i] + dy;
    dst[i] = v;
    if (dst32 && i < n32) dst32[i] = (float)v;
  }
}

// partial[blockIdx.x] = this block's sum of (sum_j c_j K_j / scale)^2; pair form: partial[gridDim.x + blockIdx.x] the same with c2
__global__ __launch_bounds__(256) void rk_error_kernel(const double* __restrict__ y, const double* __restrict__ y_new, const double* __restrict__ k,
                                                       size_t n, rk_terms c, int pair, double atol, double rtol, double* __restrict__ partial) {
  SSDE_LDS(smem);
  double* red = reinterpret_cast<double*>(smem);      // [2][4]
  double acc = 0.0, acc2 = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    double e = 0.0, e2 = 0.0;
    for (int t = 0; t < c.count; ++t) {
      const double v = k[(size_t)c.row[t] * n + i];
      e += v * c.c[t];                                                         // single form: E_j * h folded on the host
      if (pair) e2 += v * c.c2[t];
    }
    const double scale = atol + fmax(fabs(y[i]), fabs(y_new[i])) * rtol;
    const double q = e / scale, q2 = e2 / scale;
    acc += q * q;
    acc2 += q2 * q2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    acc2 += __shfl_xor(acc2, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = acc;
    red[4 + (threadIdx.x >> 6)] = acc2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (pair) partial[gridDim.x + blockIdx.x] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}
// single form: sqrt(s / n), scipy's RMS norm.  Pair form (scipy's DOP853._estimate_error_norm):
// |h| s5 / sqrt((s5 + 0.01 s3) n), and 0 when both sums are 0.
__global__ void rk_error_finish_kernel(const double* __restrict__ partial, int blocks, size_t n, int pair, double h_abs, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0, s3 = 0.0;
    for (int i = 0; i < blocks; ++i) s += partial[i];       // fixed order: deterministic accept / reject decisions
    if (!pair) {
      out[0] = sqrt(s / (double)n);
      return;
    }
    for (int i = 0; i < blocks; ++i) s3 += partial[blocks + i];
    out[0] = (s == 0.0 && s3 == 0.0) ? 0.0 : h_abs * s / sqrt((s + 0.01 * s3) * (double)n);
  }
}

// drift of the probability-flow ODE for the stock SDEs, RSDE.sde with probability_flow=True (sde_lib.py:93-97):
//   drift = f(x, t) - g(t)^2 * score * 0.5,  f = a(t) * x  (a = -beta(t)/2 for VP / sub-VP, 0 for VE)
// evaluated in fp32 in the reference's operation order (no contraction), widened to the integrator's fp64.
__global__ __launch_bounds__(256) void pf_drift_kernel(const float* __restrict__ x, const float* __restrict__ score, double* __restrict__ dst,
                                                       size_t numel, float a, float g2, const ssde_ode_dyn* __restrict__ dyn) {
  if (dyn) { a = dyn->a; g2 = dyn->g2; dst = dyn->dst; }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (size_t)gridDim.x * blockDim.x) {
    const float f = ssde_fmul_rn(a, x[i]);
    const float d = ssde_fmul_rn(ssde_fmul_rn(g2, score[i]), 0.5f);
    dst[i] = (double)ssde_fsub_rn(f, d);
  }
}

// eps^T (d drift / d x) eps per sample (likelihood.py:29-35: grad of sum(drift * eps) wrt x, times eps, summed over the
// image): the cotangent of the input-gradient program is eps itself, so gx = J_score^T eps and the drift's own factors
// (a for the linear part, -g2/2 for the score part, sde_lib.py:93-97) are applied here.  fp32 terms as the reference,
// summed in fp64 in a fixed order (thread-strided partials, wave shuffles, 4 waves in order).
__global__ __launch_bounds__(256) void hutch_div_kernel(const float* __restrict__ gx, const float* __restrict__ eps, double* __restrict__ dst,
                                                        long long dst_off, int per, float a, float g2, const ssde_ode_dyn* __restrict__ dyn) {
  SSDE_LDS(smem);
  double* red = reinterpret_cast<double*>(smem);      // [4]
  if (dyn) { a = dyn->a; g2 = dyn->g2; dst = dyn->dst; }
  const size_t base = (size_t)blockIdx.x * per;
  double acc = 0.0;
  for (int i = threadIdx.x; i < per; i += 256) {
    const float e = eps[base + i];
    const float t = ssde_fsub_rn(ssde_fmul_rn(a, e), ssde_fmul_rn(ssde_fmul_rn(g2, gx[base + i]), 0.5f));
    acc += (double)ssde_fmul_rn(t, e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) dst[dst_off + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the rows with a non-zero coefficient (in either row of the pair form), ascending
static rk_terms rk_active_terms(const double* coef, const double* coef2, int rows) {
  rk_terms t;
  memset(&t, 0, sizeof(t));
  for (int j = 0; j < rows; ++j) {
    if (coef[j] == 0.0 && !(coef2 && coef2[j] != 0.0)) continue;
    t.row[t.count] = j;
    t.c[t.count] = coef[j];
    t.c2[t.count] = coef2 ? coef2[j] : 0.0;
    t.count++;
  }
  return t;
}

extern "C" int ssde_rk_combine_rows(const ssde_rk_combine_rows_args* a, void* stream) {
  SSDE_REQUIRE(a && a->y && a->dst && a->n > 0 && a->n32 >= 0, "rk_combine: bad args");
  SSDE_REQUIRE(a->terms >= 0 && a->terms <= SSDE_RK_MAX_TERMS && (a->terms == 0 || a->k), "rk_combine: terms = %d, at most %d (with K)",
               a->terms, SSDE_RK_MAX_TERMS);
  hipLaunchKernelGGL(rk_combine_kernel, dim3(grid_for((size_t)a->n)), dim3(256), 0, static_cast<hipStream_t>(stream), a->y, a->k, (size_t)a->n,
                     rk_active_terms(a->coef, nullptr, a->terms), a->dst, a->dst32, a->n32 > 0 ? (size_t)a->n32 : (size_t)a->n);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_rk_error_norm_rows(const ssde_rk_error_rows_args* a, void* stream) {
  SSDE_REQUIRE(a && a->y && a->y_new && a->k && a->partial && a->out && a->n > 0, "rk_error_norm: bad args");
  SSDE_REQUIRE(a->rows >= 1 && a->rows <= SSDE_RK_MAX_ROWS, "rk_error_norm: rows = %d, 1 to %d", a->rows, SSDE_RK_MAX_ROWS);
  SSDE_REQUIRE(!a->pair || (a->h_abs >= 0 && isfinite(a->h_abs)), "rk_error_norm: the pair form needs a finite |h|");
  const int pair = a->pair != 0;
  const unsigned blocks = grid_for((size_t)a->n, 256, pair ? 512 : 1024);
  SSDE_REQUIRE((int64_t)blocks * (pair ? 2 : 1) <= (int64_t)a->partial_len, "rk_error_norm: partial buffer needs %u doubles", blocks * (pair ? 2 : 1));
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rk_error_kernel, dim3(blocks), dim3(256), 64, st, a->y, a->y_new, a->k, (size_t)a->n,
                     rk_active_terms(a->coef, pair ? a->coef2 : nullptr, a->rows), pair, a->atol, a->rtol, a->partial);
  SSDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(rk_error_finish_kernel, dim3(1), dim3(64), 0, st, a->partial, (int)blocks, (size_t)a->n, pair, a->h_abs, a->out);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

// the Dormand-Prince entry points: the same launches with seven rows
extern "C" int ssde_rk_combine(const ssde_rk_combine_args* a, void* stream) {
  SSDE_REQUIRE(a && a->y && a->dst && a->n > 0 && a->terms >= 0 && a->terms <= 7 && (a->terms == 0 || a->k), "rk_combine: bad args");
  ssde_rk_combine_rows_args r;
  memset(&r, 0, sizeof(r));
  r.y = a->y; r.k = a->k; r.n = a->n; r.terms = a->terms; r.dst = a->dst; r.dst32 = a->dst32; r.n32 = a->n32;
  for (int j = 0; j < a->terms; ++j) r.coef[j] = a->coef.v[j];
  return ssde_rk_combine_rows(&r, stream);
}

extern "C" int ssde_rk_error_norm(const ssde_rk_error_args* a, void* stream) {
  SSDE_REQUIRE(a && a->y && a->y_new && a->k && a->partial && a->out && a->n > 0, "rk_error_norm: bad args");
  ssde_rk_error_rows_args r;
  memset(&r, 0, sizeof(r));
  r.y = a->y; r.y_new = a->y_new; r.k = a->k; r.n = a->n; r.rows = 7; r.atol = a->atol; r.rtol = a->rtol;
  r.partial = a->partial; r.partial_len = a->partial_len; r.out = a->out;
  for (int j = 0; j < 7; ++j) r.coef[j] = a->coef.v[j];
  return ssde_rk_error_norm_rows(&r, stream);
}

extern "C" int ssde_pf_drift(const ssde_pf_drift_args* a, void* stream) {
  SSDE_REQUIRE(a && a->x && a->score && (a->dst || a->dyn) && a->numel > 0, "pf_drift: bad args");
  hipLaunchKernelGGL(pf_drift_kernel, dim3(grid_for((size_t)a->numel)), dim3(256), 0, static_cast<hipStream_t>(stream), a->x, a->score, a->dst,
                     (size_t)a->numel, a->a, a->g2, a->dyn);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_hutch_div(const ssde_hutch_div_args* a, void* stream) {
  SSDE_REQUIRE(a && a->gx && a->eps && (a->dst || a->dyn) && a->n > 0 && a->per > 0 && a->dst_off >= 0, "hutch_div: bad args");
  hipLaunchKernelGGL(hutch_div_kernel, dim3(a->n), dim3(256), 64, static_cast<hipStream_t>(stream), a->gx, a->eps, a->dst,
                     (long long)a->dst_off, a->per, a->a, a->g2, a->dyn);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_randn(const ssde_randn_args* a, void* stream) {
  SSDE_REQUIRE(a && a->dst && a->numel > 0, "randn: bad args");
  SSDE_REQUIRE(a->stream_id >= 0 && a->stream_id < 16, "randn: stream_id must be in 0..15");
  SSDE_REQUIRE(reinterpret_cast<uintptr_t>(a->dst) % 16 == 0, "randn: dst must be 16-byte aligned (it is written as float4)");
  hipLaunchKernelGGL(randn_kernel, dim3(grid_for((size_t)a->numel / 4, 256, 1024)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a->dst, (size_t)a->numel, (unsigned long long)a->seed, a->step_ptr, a->stream_id,
                     reinterpret_cast<const unsigned long long*>(a->seed_ptr));
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_langevin_update(const ssde_langevin_args* a, void* stream) {
  SSDE_REQUIRE(a && a->x && a->x_mean && a->grad && a->noise && a->grad_sumsq && a->noise_sumsq, "langevin: null args");
  SSDE_REQUIRE(a->n > 0 && a->per > 0, "langevin: bad shape");
  const size_t numel = (size_t)a->n * a->per;
  hipLaunchKernelGGL(langevin_kernel, dim3(grid_for(numel)), dim3(256), 64, static_cast<hipStream_t>(stream),
                     a->x, a->x_mean, a->grad, a->noise, a->grad_sumsq, a->noise_sumsq, a->alpha_tab, a->step_ptr,
                     a->n, numel, a->snr);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_predictor_update(const ssde_predictor_args* a, void* stream) {
  SSDE_REQUIRE(a && a->x && a->x_mean && a->score && a->coef && a->numel > 0, "predictor: bad args");
  hipLaunchKernelGGL(predictor_kernel, dim3(grid_for((size_t)a->numel)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     a->x, a->x_mean, a->score, a->noise, a->coef, a->step_ptr, (size_t)a->numel);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_sample_update(const ssde_sample_update_args* a, void* stream) {
  SSDE_REQUIRE(a && a->x && a->x_mean && a->x_out && a->n > 0 && a->per > 0, "sample_update: bad args");
  SSDE_REQUIRE((!a->y || a->b) && (!a->z || a->c), "sample_update: a tensor term needs its coefficient vector");
  const size_t numel = (size_t)a->n * a->per;
  hipLaunchKernelGGL(sample_update_kernel, dim3(grid_for(numel)), dim3(256), 0, static_cast<hipStream_t>(stream), a->x, a->y, a->z, a->a,
                     a->b, a->c, a->x_mean, a->x_out, a->per, numel);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_fill_from_table(const ssde_fill_args* a, void* stream) {
  SSDE_REQUIRE(a && a->dst && a->tab && a->n > 0, "fill: bad args");
  hipLaunchKernelGGL(fill_kernel, dim3(ssde_cdiv(a->n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     a->dst, a->tab, a->step_ptr, a->n);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_project_update(const ssde_project_args* a, void* stream) {
  SSDE_REQUIRE(a && a->x && a->x_mean && a->data && a->mask && a->noise && a->coef, "project: null args");
  SSDE_REQUIRE(a->n > 0 && a->c > 0 && a->hw > 0, "project: bad shape");
  if (a->use_matrix) {
    SSDE_REQUIRE(a->c == 3, "project: the colour-space form needs 3 channels (got %d)", a->c);
    SsdeMat3 M, invM;
    for (int i = 0; i < 9; ++i) { M.m[i] = a->M[i]; invM.m[i] = a->invM[i]; }
    hipLaunchKernelGGL(project_color_kernel, dim3(grid_for((size_t)a->n * a->hw)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a->x, a->x_mean, a->data, a->mask, a->noise, a->coef, a->step_ptr, a->n, a->hw, M, invM);
  } else {
    hipLaunchKernelGGL(project_kernel, dim3(grid_for((size_t)a->n * a->c * a->hw)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a->x, a->x_mean, a->data, a->mask, a->noise, a->coef, a->step_ptr, (size_t)a->n * a->c * a->hw);
  }
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_project_prepare(const ssde_project_prepare_args* a, void* stream) {
  SSDE_REQUIRE(a, "project_prepare: null args");
  SSDE_REQUIRE(a->n > 0 && a->c > 0 && a->hw > 0, "project_prepare: bad shape");
  SSDE_REQUIRE(a->mask || a->use_matrix, "project_prepare: mask == NULL (the task's own mask) needs the colour-space form");
  SSDE_REQUIRE(a->data || (a->prior && a->known), "project_prepare: without data the launch reads known and needs a prior");
  SSDE_REQUIRE(a->data || !a->mask_out || a->mask_out == a->mask, "project_prepare: without data there is no mask to write");
  SSDE_REQUIRE(!a->prior || a->x, "project_prepare: a prior needs the state x to write");
  SSDE_REQUIRE(a->prior || a->known || a->mask_out, "project_prepare: nothing to write");
  if (a->use_matrix) {
    SSDE_REQUIRE(a->c == 3, "project_prepare: the colour-space form needs 3 channels (got %d)", a->c);
    SsdeMat3 M, invM;
    for (int i = 0; i < 9; ++i) { M.m[i] = a->M[i]; invM.m[i] = a->invM[i]; }
    hipLaunchKernelGGL(project_prepare_color_kernel, dim3(grid_for((size_t)a->n * a->hw)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a->data, a->mask, a->prior, a->known, a->mask_out, a->x, a->x_mean, a->n, a->hw, M, invM);
  } else {
    hipLaunchKernelGGL(project_prepare_kernel, dim3(grid_for((size_t)a->n * a->c * a->hw)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a->data, a->mask, a->prior, a->known, a->mask_out, a->x, a->x_mean, (size_t)a->n * a->c * a->hw);
  }
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_concat(const ssde_concat_args* a, void* stream) {
  SSDE_REQUIRE(a && a->p0 && a->p1 && a->dst, "concat: null args");
  SSDE_REQUIRE(a->n > 0 && a->hw > 0, "concat: bad shape (n %d, hw %d)", a->n, a->hw);
  SSDE_REQUIRE(a->c0 > 0 && a->c1 > 0 && a->c0 % 4 == 0 && a->c1 % 4 == 0,
               "concat: channel counts must be positive multiples of 4 (got %d and %d)", a->c0, a->c1);
  SSDE_REQUIRE((reinterpret_cast<uintptr_t>(a->p0) | reinterpret_cast<uintptr_t>(a->p1) | reinterpret_cast<uintptr_t>(a->dst)) % 16 == 0,
               "concat: p0, p1 and dst must be 16-byte aligned (they are read and written as float4)");
  const size_t rows = (size_t)a->n * a->hw;
  const int q0 = a->c0 / 4, q1 = a->c1 / 4;
  // (workgroups: 16 per compute unit at the most, the grid-stride loop takes the rest)
  hipLaunchKernelGGL(concat_kernel, dim3(grid_for(rows * (size_t)(q0 + q1), 256, (unsigned)ssde_num_cus() * 16)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const float4*>(a->p0), reinterpret_cast<const float4*>(a->p1),
                     reinterpret_cast<float4*>(a->dst), rows, q0, q1);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}

extern "C" int ssde_step_inc(const ssde_step_inc_args* a, void* stream) {
  SSDE_REQUIRE(a && a->step_ptr, "step_inc: null args");
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), a->step_ptr, a->delta);
  SSDE_LAUNCH_CHECK();
  return SSDE_OK;
}
