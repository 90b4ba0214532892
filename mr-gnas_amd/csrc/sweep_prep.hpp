// The small kernels around the [queries, entities] sweeps that keep no [B, N] tensor: the per-query list lookup in front of a sweep and
// the fixed-order finish behind it.  Shared by the DistMult sweeps on the row GEMM (bce.hip, rank.hip) and the L1 sweeps of TransE
// (transe_1n.hip).  `static`: every translation unit that includes this header gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// qlist[i] = {begin, end} of the object list of qkey[i] (empty when the key is unknown)
static __global__ void bce_prep_k(const int64_t* __restrict__ qkey, const int64_t* __restrict__ keys, const int32_t* __restrict__ rowptr, int64_t U,
                                  int64_t B, int32_t* __restrict__ qlist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int lo = 0, hi = 0;
  if (U > 0) {
    const int64_t key = qkey[i];
    int64_t b = 0, e = U;
    while (b < e) {
      const int64_t mid = b + ((e - b) >> 1);
      if (keys[mid] < key) b = mid + 1; else e = mid;
    }
    if (b < U && keys[b] == key) { lo = rowptr[b]; hi = rowptr[b + 1]; }
  }
  *reinterpret_cast<int2*>(qlist + i * 2) = make_int2(lo, hi);
}

// loss = scale * (the n partials added in a fixed order: thread t adds partial[t], partial[t + 256], ..., then a tree over the threads)
static __global__ __launch_bounds__(256) void bce_finish_k(const double* __restrict__ partial, int64_t n, double scale, float* __restrict__ loss) {
  __shared__ double s[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(s[0] * scale);
}

// {begin, end} of the filter list of query i's key (empty when there is no index, or the key is -1 or unknown)
__device__ __forceinline__ int2 sweep_filter_list(const int64_t* __restrict__ qkey, const int64_t* __restrict__ keys,
                                                  const int32_t* __restrict__ rowptr, int64_t U, int64_t i) {
  int lo = 0, hi = 0;
  const int64_t key = (qkey && U > 0) ? qkey[i] : -1;
  if (key >= 0) {
    int64_t b = 0, e = U;
    while (b < e) {
      const int64_t mid = b + ((e - b) >> 1);
      if (keys[mid] < key) b = mid + 1; else e = mid;
    }
    if (b < U && keys[b] == key) { lo = rowptr[b]; hi = rowptr[b + 1]; }
  }
  return make_int2(lo, hi);
}

// qinfo[i] = {target, begin, end of the list of qkey[i] (empty when the key is -1 or unknown), when}; counts[i] = 0
static __global__ void rank_prep_k(const int32_t* __restrict__ t_idx, const int64_t* __restrict__ qkey, const int32_t* __restrict__ when,
                                   const int64_t* __restrict__ keys, const int32_t* __restrict__ rowptr, int64_t U, int64_t Q,
                                   int32_t* __restrict__ qinfo, unsigned* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const int2 l = sweep_filter_list(qkey, keys, rowptr, U, i);
  *reinterpret_cast<int4*>(qinfo + i * 4) = make_int4(t_idx[i], l.x, l.y, when ? when[i] : -1);
  counts[i] = 0;
}

// The top-k sweeps' form of rank_prep_k: there is no target (qinfo[i].x = -1, an id no candidate has), and instead of a count the
// query's running list ids / vals [Q][k] starts empty: id -1, value `pad`.
static __global__ void topk_prep_k(const int64_t* __restrict__ qkey, const int32_t* __restrict__ when, const int64_t* __restrict__ keys,
                                   const int32_t* __restrict__ rowptr, int64_t U, int64_t Q, int k, float pad, int32_t* __restrict__ qinfo,
                                   int32_t* __restrict__ ids, float* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const int2 l = sweep_filter_list(qkey, keys, rowptr, U, i);
  *reinterpret_cast<int4*>(qinfo + i * 4) = make_int4(-1, l.x, l.y, when ? when[i] : -1);
  for (int t = 0; t < k; ++t) { ids[i * k + t] = -1; vals[i * k + t] = pad; }
}

static __global__ void rank_finish_k(const unsigned* __restrict__ counts, int64_t* __restrict__ ranks, int64_t Q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Q) ranks[i] = 1 + (int64_t)counts[i];
}

}  // namespace mrg
