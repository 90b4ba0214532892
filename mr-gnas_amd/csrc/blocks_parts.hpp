// Parts shared by the block builders (blocks.hip: one fan-out over all in-edges; blocks_rel.hip: one fan-out per edge type).
#pragma once
#include <climits>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "common.hpp"

namespace mrg {

constexpr int BLOCKS_MAX_FANOUT = 64;       // one lane of a wave per pick

static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Temporary storage of an int32 scan over n items as the workspace queries size it: a HOST formula (the queries answer without a
// device), 16 bytes per 64 items + 4 KiB -- several times what rocprim's look-back scan takes (8 bytes of state per workgroup of
// >= 256 items, and a fixed part).  scan_into checks it against rocprim's own figure before it launches.
static size_t scan_temp_bound(int64_t n) { return up256(4096 + 16 * (size_t)((n + 63) / 64)); }

template <typename It>
static int scan_into(void* temp, It in, int32_t* out, int64_t n, hipStream_t st) {
  size_t need = 0, have = scan_temp_bound(n);
  hipError_t e = rocprim::exclusive_scan(nullptr, need, in, out, 0, (size_t)n, rocprim::plus<int32_t>(), st);
  if (e != hipSuccess) return (int)e;
  if (need > have) return MRG_E_WORKSPACE;
  e = rocprim::exclusive_scan(temp, have, in, out, 0, (size_t)n, rocprim::plus<int32_t>(), st);
  return e != hipSuccess ? (int)e : MRG_OK;
}

// One step of Floyd's algorithm as every formulation of the sampler computes it: the candidate of step s for a list of d entries
// and k picks, j = d - k + s, t = min(floor(u (j + 1)), j).  One float64 product: the same IEEE operation in torch and in Python.
__device__ __forceinline__ int32_t floyd_candidate(double us, int32_t j) {
  long long t = (long long)(us * (double)((int64_t)j + 1));   // floor: the product is >= 0
  if (!(t >= 0)) t = 0;
  if (t > j) t = j;
  return (int32_t)t;
}

}  // namespace mrg
