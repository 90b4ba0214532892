// What the MixedOp epilogue (mixedop.hip) and cell zero (cell_zero.hip) share: pointer packs, the device row count,
// grid sizing and the BatchNorm argument packs.
#pragma once
#include "common.hpp"

#define MRG_MIX_MAXK 8
static_assert(MRG_MIX_MAXK == MRG_MIX_MAX_CANDIDATES, "mrg_gated_branch.given is sized by the header's constant");

namespace mrg {

struct PtrPack { const float* p[MRG_MIX_MAXK]; };
struct MutPack { float* p[MRG_MIX_MAXK]; };

// rows that count: min(rows, *vrows) when the launch was given a device row count, else rows
__device__ __forceinline__ int64_t valid_rows(const int32_t* vrows, int64_t rows) {
  if (vrows == nullptr) return rows;
  const int64_t v = (int64_t)*vrows;
  return v < rows ? (v < 0 ? 0 : v) : rows;
}

// FEW ROWS (round 5: a sampled step graph, a rank's node chunk): a wave walks its rows one dependent memory round trip at a time, so
// with `trips` rows per wave a launch over 900 rows is ~30 blocks of 8 trips = a 15 us latency chain on an idle chip.  Until there
// is a block per CU, a block gets ONE row per wave: rows / (rows per trip) blocks, at most 256.
static int64_t row_blocks(int64_t rows, int lpr, int trips) {
  const int64_t per_trip = MRG_BLOCK / lpr;
  int64_t b = (rows + per_trip * trips - 1) / (per_trip * trips);
  if (b < 256) {
    const int64_t b1 = (rows + per_trip - 1) / per_trip;
    b = b1 < 256 ? b1 : 256;
  }
  return b < 1 ? 1 : b;
}
static int capped(int64_t blocks, int cap) { return (int)(blocks < cap ? blocks : cap); }

// gamma / beta / running mean / running variance: host arrays of K device pointers (entries may be NULL; the running statistics
// may be absent as a whole) -> kernel arguments.  MRG_E_NULLPTR when a candidate has one running statistic without the other.
struct BnPacks { PtrPack gamma, beta; MutPack rmean, rvar; };
static int bn_packs(BnPacks* bn, const float* const* gamma_host, const float* const* beta_host, float* const* rmean_host,
                    float* const* rvar_host, int K) {
  *bn = BnPacks{};
  for (int k = 0; k < K; ++k) {
    bn->gamma.p[k] = gamma_host[k]; bn->beta.p[k] = beta_host[k];
    bn->rmean.p[k] = rmean_host ? rmean_host[k] : nullptr;
    bn->rvar.p[k] = rvar_host ? rvar_host[k] : nullptr;
    if ((bn->rmean.p[k] == nullptr) != (bn->rvar.p[k] == nullptr)) return MRG_E_NULLPTR;
  }
  return MRG_OK;
}

// launches mix_reduce_finalize_fwd_k (mixedop.hip; the kernel lives in that translation unit only) over the nb per-block partial
// sums [nb][K][2][D] in ws: coefficients and running statistics of K candidates
int launch_reduce_finalize_fwd(const void* ws, int nb, const BnPacks& bn, int K, double total_rows, int D, float eps, float momentum,
                               float* coef, const int32_t* vrows, hipStream_t st);

}  // namespace mrg
