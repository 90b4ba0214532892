// The tail of a search / train step -- clip_grad_norm_ + SGD with momentum (reference search/mr_lp_search.py:243-245,
// torch.optim.SGD at :118-119) -- over ALL parameter tensors in three launches.  torch runs it as ~30 multi_tensor_apply
// launches (a kernel-argument block holds ~100 tensor pointers) of ~16 us each plus the norm's stack / clamp kernels: 0.45 ms of
// a 7 ms sampled step.  Here the tensors are addressed through a device table of pointers and the work is cut into fixed
// chunks (host-built once: the parameter shapes never change), so the launch count does not depend on the tensor count.
//   1. multi_sqnorm_k      chunk b: sum of squares of its <= CHUNK gradient elements, in double -> partial[b]
//   2. multi_norm_final_k  one workgroup: partial[0..nb) in fixed order -> coef = min(1, max_norm / (sqrt(sum) + 1e-6))
//   3. multi_sgd_k         chunk b: g = coef * grad (+ wd * p);  buf = momentum * buf + g;  p -= lr * buf
// A tensor whose gradient pointer is null takes no part (torch skips parameters without a gradient).  Deterministic.
//
// Adam (torch.optim.Adam, amsgrad / maximize off: the reference's architect, models/architect_lp.py:20-22, and its training driver,
// train/mr_lp_train.py:140) over the same tables in two launches:
//   1. multi_adam_tick_k   tensor t with a gradient: s = ++step[t];  scal[t] = { lr / (1 - beta1^s), 1 / sqrt(1 - beta2^s) }  (double)
//   2. multi_adam_k        chunk b: g += wd * p;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
//                                   p -= scal[t][0] * m / (sqrt(v) * scal[t][1] + eps)
// Step counts are per tensor (torch keeps one per parameter: a parameter that misses a gradient lags behind) and, like lr, live in
// device memory: a captured step advances its own bias correction on replay and follows a learning-rate schedule.
#include "common.hpp"
#include "../../include/mrgnas.h"

namespace mrg {

constexpr int OPT_CHUNK = 4096;          // elements per chunk (256 threads x 16)

__global__ __launch_bounds__(256) void multi_sqnorm_k(const float* const* __restrict__ grads, const int32_t* __restrict__ chunk_tensor,
                                                       const int64_t* __restrict__ chunk_off, const int32_t* __restrict__ chunk_len,
                                                       double* __restrict__ partial) {
  __shared__ double red[256];
  const int b = blockIdx.x;
  const float* g = grads[chunk_tensor[b]];
  double acc = 0.0;
  if (g) {
    g += chunk_off[b];
    const int n = chunk_len[b];
    for (int i = threadIdx.x; i < n; i += 256) { const double v = g[i]; acc += v * v; }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[b] = red[0];
}

__global__ __launch_bounds__(256) void multi_norm_final_k(const double* __restrict__ partial, int nb, float max_norm, float* __restrict__ out2) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    float coef = max_norm / (norm + 1e-6f);                 // torch.nn.utils.clip_grad_norm_: clip_coef clamped to 1
    if (!(coef < 1.0f)) coef = 1.0f;
    out2[0] = norm;
    out2[1] = max_norm > 0.f ? coef : 1.0f;
  }
}

__global__ __launch_bounds__(256) void multi_sgd_k(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                    float* const* __restrict__ bufs, const int32_t* __restrict__ chunk_tensor,
                                                    const int64_t* __restrict__ chunk_off, const int32_t* __restrict__ chunk_len,
                                                    const float* __restrict__ norm_coef, float lr, float momentum, float weight_decay) {
  const int b = blockIdx.x, t = chunk_tensor[b];
  const float* g = grads[t];
  if (!g) return;
  const int64_t off = chunk_off[b];
  g += off;
  float* p = params[t] + off;
  float* m = bufs[t] + off;
  const int n = chunk_len[b];
  const float coef = norm_coef[1];
  for (int i = threadIdx.x; i < n; i += 256) {
    float gi = g[i] * coef;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    const float mi = momentum * m[i] + gi;
    m[i] = mi;
    p[i] = pi - lr * mi;
  }
}

__global__ __launch_bounds__(256) void multi_adam_tick_k(const float* const* __restrict__ grads, int n_tensors, float* __restrict__ step,
                                                          float* __restrict__ scal, const float* __restrict__ lr, double beta1, double beta2) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tensors || !grads[t]) return;
  const float s = step[t] + 1.0f;                             // (float32 like torch's state['step']: exact up to 2^24 steps)
  step[t] = s;
  scal[2 * t] = (float)((double)lr[0] / (1.0 - pow(beta1, (double)s)));
  scal[2 * t + 1] = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)s)));
}

struct AdamCoef { float b1, c1, b2, c2, eps, wd, step_size, rsqrt_bc2; };

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamCoef& k) {
  if (k.wd != 0.f) g += k.wd * p;
  m = k.b1 * m + k.c1 * g;
  v = k.b2 * v + k.c2 * g * g;
  p -= k.step_size * (m / (sqrtf(v) * k.rsqrt_bc2 + k.eps));
}

__global__ __launch_bounds__(256) void multi_adam_k(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                     float* const* __restrict__ exp_avg, float* const* __restrict__ exp_avg_sq,
                                                     const int32_t* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off,
                                                     const int32_t* __restrict__ chunk_len, const float* __restrict__ scal, float beta1,
                                                     float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float weight_decay) {
  const int b = blockIdx.x, t = chunk_tensor[b];
  const float* g = grads[t];
  if (!g) return;
  const int64_t off = chunk_off[b];
  g += off;
  float* p = params[t] + off;
  float* m = exp_avg[t] + off;
  float* v = exp_avg_sq[t] + off;
  const int n = chunk_len[b];
  const AdamCoef k = {beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, scal[2 * t], scal[2 * t + 1]};
  int done = 0;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {            // block-uniform: 16-byte accesses
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      float4 pi = reinterpret_cast<float4*>(p)[i], mi = reinterpret_cast<float4*>(m)[i], vi = reinterpret_cast<float4*>(v)[i];
      const float4 gi = reinterpret_cast<const float4*>(g)[i];
      adam_one(pi.x, gi.x, mi.x, vi.x, k);
      adam_one(pi.y, gi.y, mi.y, vi.y, k);
      adam_one(pi.z, gi.z, mi.z, vi.z, k);
      adam_one(pi.w, gi.w, mi.w, vi.w, k);
      reinterpret_cast<float4*>(m)[i] = mi;
      reinterpret_cast<float4*>(v)[i] = vi;
      reinterpret_cast<float4*>(p)[i] = pi;
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += 256) {                                        // unaligned chunks, and the tail
    float pi = p[i], mi = m[i], vi = v[i];
    adam_one(pi, g[i], mi, vi, k);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// The parameter passes of the second-order (unrolled) DARTS architect step (reference models/architect_lp.py:26-35,88-103) over the
// same tables.  Memory-bound sweeps: the grid is capped at UNROLLED_GRID workgroups, which stride over the chunks.
//   multi_virtual_sgd_k     backup = p;  p = p - eta * (momentum * buf + (g + wd * p))             (eta from device memory)
//   multi_radius_final_k    one workgroup: partial[0..nb) in fixed order -> scal = { |v|, R = r / |v|, 1 / (2 R) }  (0, 0 when |v| = 0)
//   multi_shift_k           p = backup + sign * R * v  (sign 0: p = backup, a copy)
//   multi_alpha_combine_k   ig = (gp - gn) * (1 / (2 R));  out = dalpha - eta * ig
// A chunk whose addresses are all 16-byte aligned moves 16 bytes per lane (workgroup-uniform test), any other chunk and every tail
// 4 bytes per lane: a gradient may be a contiguous view that starts anywhere inside a larger buffer.
constexpr int UNROLLED_GRID = 2048;

__device__ __forceinline__ float virtual_one(float p, float g, float mb, float eta, float wd) {
  if (wd != 0.f) g += wd * p;
  return p - eta * (mb + g);
}

__global__ __launch_bounds__(256) void multi_virtual_sgd_k(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                            const float* const* __restrict__ bufs, float* const* __restrict__ backup,
                                                            const int32_t* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off,
                                                            const int32_t* __restrict__ chunk_len, int n_chunks,
                                                            const float* __restrict__ eta_p, float momentum, float weight_decay) {
  const float eta = eta_p[0];
  for (int b = blockIdx.x; b < n_chunks; b += gridDim.x) {
    const int t = chunk_tensor[b];
    const int64_t off = chunk_off[b];
    const int n = chunk_len[b];
    float* p = params[t] + off;
    float* k = backup[t] + off;
    const float* g = grads[t] ? grads[t] + off : nullptr;                                      // no gradient: a zero one
    const float* m = (bufs && bufs[t] && momentum != 0.f) ? bufs[t] + off : nullptr;           // no buffer: a zero moment
    int done = 0;
    if (g && (((uintptr_t)p | (uintptr_t)k | (uintptr_t)g | (uintptr_t)m) & 15) == 0) {        // (a null m passes the test)
      const int n4 = n >> 2;
      for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 pi = reinterpret_cast<const float4*>(p)[i], gi = reinterpret_cast<const float4*>(g)[i];
        float4 mi = {0.f, 0.f, 0.f, 0.f};
        if (m) {
          mi = reinterpret_cast<const float4*>(m)[i];
          mi.x *= momentum; mi.y *= momentum; mi.z *= momentum; mi.w *= momentum;
        }
        reinterpret_cast<float4*>(k)[i] = pi;
        float4 o;
        o.x = virtual_one(pi.x, gi.x, mi.x, eta, weight_decay);
        o.y = virtual_one(pi.y, gi.y, mi.y, eta, weight_decay);
        o.z = virtual_one(pi.z, gi.z, mi.z, eta, weight_decay);
        o.w = virtual_one(pi.w, gi.w, mi.w, eta, weight_decay);
        reinterpret_cast<float4*>(p)[i] = o;
      }
      done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += 256) {
      const float pi = p[i];
      k[i] = pi;
      p[i] = virtual_one(pi, g ? g[i] : 0.f, m ? momentum * m[i] : 0.f, eta, weight_decay);
    }
  }
}

__global__ __launch_bounds__(256) void multi_radius_final_k(const double* __restrict__ partial, int nb, float r, float* __restrict__ scal) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double norm = sqrt(red[0]);
    const float R = norm > 0.0 ? (float)((double)r / norm) : 0.f;
    scal[0] = (float)norm;
    scal[1] = R;
    scal[2] = R > 0.f ? (float)(1.0 / (2.0 * (double)R)) : 0.f;       // from the float32 R the shifts use: the distance really moved
  }
}

__global__ __launch_bounds__(256) void multi_shift_k(float* const* __restrict__ params, const float* const* __restrict__ backup,
                                                      const float* const* __restrict__ vecs, const int32_t* __restrict__ chunk_tensor,
                                                      const int64_t* __restrict__ chunk_off, const int32_t* __restrict__ chunk_len,
                                                      int n_chunks, const float* __restrict__ scal, int sign) {
  const float s = sign == 0 ? 0.f : (sign > 0 ? scal[1] : -scal[1]);
  for (int b = blockIdx.x; b < n_chunks; b += gridDim.x) {
    const int t = chunk_tensor[b];
    const int64_t off = chunk_off[b];
    const int n = chunk_len[b];
    float* p = params[t] + off;
    const float* k = backup[t] + off;
    const float* v = (sign != 0 && vecs && vecs[t]) ? vecs[t] + off : nullptr;                 // no vector: a zero one, p = backup
    int done = 0;
    if ((((uintptr_t)p | (uintptr_t)k | (uintptr_t)v) & 15) == 0) {
      const int n4 = n >> 2;
      for (int i = threadIdx.x; i < n4; i += 256) {
        float4 o = reinterpret_cast<const float4*>(k)[i];
        if (v) {
          const float4 vi = reinterpret_cast<const float4*>(v)[i];
          o.x += s * vi.x; o.y += s * vi.y; o.z += s * vi.z; o.w += s * vi.w;
        }
        reinterpret_cast<float4*>(p)[i] = o;
      }
      done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += 256) p[i] = v ? k[i] + s * v[i] : k[i];
  }
}

__global__ __launch_bounds__(256) void multi_alpha_combine_k(float* const* __restrict__ out, float* const* __restrict__ ig,
                                                              const float* const* __restrict__ dalpha, const float* const* __restrict__ gp,
                                                              const float* const* __restrict__ gn, const int32_t* __restrict__ chunk_tensor,
                                                              const int64_t* __restrict__ chunk_off, const int32_t* __restrict__ chunk_len,
                                                              int n_chunks, const float* __restrict__ eta_p, const float* __restrict__ scal) {
  const float eta = eta_p[0], inv2r = scal[2];
  for (int b = blockIdx.x; b < n_chunks; b += gridDim.x) {
    const int t = chunk_tensor[b];
    if (!gp[t] || !gn[t]) continue;                                                            // an alpha without a gradient: untouched
    const int64_t off = chunk_off[b];
    const int n = chunk_len[b];
    const float* a = gp[t] + off;
    const float* c = gn[t] + off;
    const float* d = dalpha[t] ? dalpha[t] + off : nullptr;
    float* o = out[t] + off;
    float* g = (ig && ig[t]) ? ig[t] + off : nullptr;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float gi = (a[i] - c[i]) * inv2r;
      if (g) g[i] = gi;
      o[i] = (d ? d[i] : 0.f) - eta * gi;
    }
  }
}

}  // namespace mrg

extern "C" int mrg_optim_chunk(void) { return mrg::OPT_CHUNK; }

extern "C" int mrg_clip_sgd_step(void* const* params, const void* const* grads, void* const* bufs, const int32_t* chunk_tensor,
                                 const int64_t* chunk_off, const int32_t* chunk_len, int64_t n_chunks, double* partial, float* norm_coef,
                                 float max_norm, float lr, float momentum, float weight_decay, void* stream) {
  using namespace mrg;
  if (n_chunks <= 0) return MRG_OK;
  if (!params || !grads || !bufs || !chunk_tensor || !chunk_off || !chunk_len || !partial || !norm_coef) return MRG_E_NULLPTR;
  if (n_chunks > (int64_t)2147483647) return MRG_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)n_chunks);
  hipLaunchKernelGGL(multi_sqnorm_k, grid, dim3(256), 0, st, (const float* const*)grads, chunk_tensor, chunk_off, chunk_len, partial);
  hipLaunchKernelGGL(multi_norm_final_k, dim3(1), dim3(256), 0, st, (const double*)partial, (int)n_chunks, max_norm, norm_coef);
  hipLaunchKernelGGL(multi_sgd_k, grid, dim3(256), 0, st, (float* const*)params, (const float* const*)grads, (float* const*)bufs, chunk_tensor,
                     chunk_off, chunk_len, (const float*)norm_coef, lr, momentum, weight_decay);
  return (int)hipGetLastError();
}

extern "C" int mrg_adam_step(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, int64_t n_tensors,
                             const int32_t* chunk_tensor, const int64_t* chunk_off, const int32_t* chunk_len, int64_t n_chunks, float* step,
                             float* scal, const float* lr, double beta1, double beta2, float eps, float weight_decay, void* stream) {
  using namespace mrg;
  if (n_chunks <= 0 || n_tensors <= 0) return MRG_OK;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !chunk_tensor || !chunk_off || !chunk_len || !step || !scal || !lr) return MRG_E_NULLPTR;
  if (n_chunks > (int64_t)2147483647 || n_tensors > (int64_t)2147483647) return MRG_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(multi_adam_tick_k, dim3((unsigned)((n_tensors + 255) / 256)), dim3(256), 0, st, (const float* const*)grads, (int)n_tensors,
                     step, scal, lr, beta1, beta2);
  hipLaunchKernelGGL(multi_adam_k, dim3((unsigned)n_chunks), dim3(256), 0, st, (float* const*)params, (const float* const*)grads,
                     (float* const*)exp_avg, (float* const*)exp_avg_sq, chunk_tensor, chunk_off, chunk_len, (const float*)scal, (float)beta1,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, weight_decay);
  return (int)hipGetLastError();
}

static inline unsigned unrolled_grid(int64_t n_chunks) {
  return (unsigned)(n_chunks < (int64_t)mrg::UNROLLED_GRID ? n_chunks : (int64_t)mrg::UNROLLED_GRID);
}

extern "C" int mrg_unrolled_virtual_step(void* const* params, const void* const* grads, const void* const* bufs, void* const* backup,
                                         const int32_t* chunk_tensor, const int64_t* chunk_off, const int32_t* chunk_len, int64_t n_chunks,
                                         const float* eta, float momentum, float weight_decay, void* stream) {
  using namespace mrg;
  if (n_chunks <= 0) return MRG_OK;
  if (!params || !grads || !backup || !chunk_tensor || !chunk_off || !chunk_len || !eta) return MRG_E_NULLPTR;       // (bufs may be null)
  if (n_chunks > (int64_t)2147483647) return MRG_E_SHAPE;
  hipLaunchKernelGGL(multi_virtual_sgd_k, dim3(unrolled_grid(n_chunks)), dim3(256), 0, (hipStream_t)stream, (float* const*)params,
                     (const float* const*)grads, (const float* const*)bufs, (float* const*)backup, chunk_tensor, chunk_off, chunk_len,
                     (int)n_chunks, eta, momentum, weight_decay);
  return (int)hipGetLastError();
}

extern "C" int mrg_unrolled_radius(const void* const* vecs, const int32_t* chunk_tensor, const int64_t* chunk_off, const int32_t* chunk_len,
                                   int64_t n_chunks, double* partial, float r, float* scal, void* stream) {
  using namespace mrg;
  if (!scal) return MRG_E_NULLPTR;
  if (n_chunks > 0 && (!vecs || !chunk_tensor || !chunk_off || !chunk_len || !partial)) return MRG_E_NULLPTR;
  if (n_chunks > (int64_t)2147483647 || !(r > 0.f)) return MRG_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (n_chunks > 0)
    hipLaunchKernelGGL(multi_sqnorm_k, dim3((unsigned)n_chunks), dim3(256), 0, st, (const float* const*)vecs, chunk_tensor, chunk_off, chunk_len,
                       partial);
  hipLaunchKernelGGL(multi_radius_final_k, dim3(1), dim3(256), 0, st, (const double*)partial, (int)(n_chunks > 0 ? n_chunks : 0), r, scal);
  return (int)hipGetLastError();
}

extern "C" int mrg_unrolled_shift(void* const* params, const void* const* backup, const void* const* vecs, const int32_t* chunk_tensor,
                                  const int64_t* chunk_off, const int32_t* chunk_len, int64_t n_chunks, const float* scal, int sign,
                                  void* stream) {
  using namespace mrg;
  if (sign < -1 || sign > 1) return MRG_E_ENUM;
  if (n_chunks <= 0) return MRG_OK;
  if (!params || !backup || !chunk_tensor || !chunk_off || !chunk_len || (sign != 0 && (!vecs || !scal))) return MRG_E_NULLPTR;
  if (n_chunks > (int64_t)2147483647) return MRG_E_SHAPE;
  hipLaunchKernelGGL(multi_shift_k, dim3(unrolled_grid(n_chunks)), dim3(256), 0, (hipStream_t)stream, (float* const*)params,
                     (const float* const*)backup, (const float* const*)vecs, chunk_tensor, chunk_off, chunk_len, (int)n_chunks, scal, sign);
  return (int)hipGetLastError();
}

extern "C" int mrg_unrolled_alpha_grad(void* const* out, void* const* ig, const void* const* dalpha, const void* const* gp,
                                       const void* const* gn, const int32_t* chunk_tensor, const int64_t* chunk_off,
                                       const int32_t* chunk_len, int64_t n_chunks, const float* eta, const float* scal, void* stream) {
  using namespace mrg;
  if (n_chunks <= 0) return MRG_OK;
  if (!out || !dalpha || !gp || !gn || !chunk_tensor || !chunk_off || !chunk_len || !eta || !scal) return MRG_E_NULLPTR;      // (ig may be null)
  if (n_chunks > (int64_t)2147483647) return MRG_E_SHAPE;
  hipLaunchKernelGGL(multi_alpha_combine_k, dim3(unrolled_grid(n_chunks)), dim3(256), 0, (hipStream_t)stream, (float* const*)out,
                     (float* const*)ig, (const float* const*)dalpha, (const float* const*)gp, (const float* const*)gn, chunk_tensor, chunk_off,
                     chunk_len, (int)n_chunks, eta, scal);
  return (int)hipGetLastError();
}
