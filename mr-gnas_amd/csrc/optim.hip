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
