// a_std: destination-segmented standard deviation over in-edges, the aggregator of the node-classification task
// (reference models/operations.py:168-190):  out[v] = sqrt(relu(mean(x^2) - mean(x)^2) + 1e-5) over v's in-edge messages,
// 0 for a node without in-edges (DGL's UDF reducers leave such rows at 0).
// Forward: the chunk plan of mrg_seg_reduce_fwd (graph.plan()): one LPR-lane group sums x and x^2 over one chunk of one
// destination's in-edge list in float64; a chunk that is its node's whole list finalises the row, the chunks of a split (hub)
// list leave their two partial rows in a workspace slot and one workgroup per hub adds the slots in list order.  No atomics, a
// fixed association: bitwise reproducible.  Besides out, the forward writes what the backward needs per (node, column): the mean
// m and coef = [u > 0] / (deg * out) (u = the variance before the ReLU; the mask is the ReLU's derivative).
// Backward: gmsg[e] = g[v] * coef[v] * (x[e] - m[v]), v = dst[e] -- independent per edge row; the edges may be walked in
// destination order (the plan's eid list) so that the gathered [N, D] tables are re-used from cache.
// Algorithmic bytes: fwd 4*D*E read + 12*D*N write (+ 4*E indices); bwd 4*D*(2*E + 3*N) (+ 4*E indices).
#include "common.hpp"
#include <math.h>

namespace mrg {

constexpr double STD_EPS = 1e-5;

template <int VEC, int KMAX>
struct StdAcc {
  double s[KMAX][VEC], q[KMAX][VEC];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[k][j] = q[k][j] = 0.0;
  }
};

// out / mean / coef of the columns c * VEC .. c * VEC + VEC - 1 of row v from the sums s, q over deg messages
template <int VEC>
__device__ __forceinline__ void std_finalize(const double* s, const double* q, int64_t v, int c, int deg, float* __restrict__ out,
                                             float* __restrict__ mean, float* __restrict__ coef, int D) {
  Vec<VEC> o = Vec<VEC>::fill(0.f), m = Vec<VEC>::fill(0.f), k = Vec<VEC>::fill(0.f);
  if (deg > 0) {
    const double dd = (double)deg;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const double mu = s[j] / dd;                          // divisions, not a reciprocal: equal messages give u == 0 exactly
      const double u = q[j] / dd - mu * mu;
      const double sd = sqrt((u > 0.0 ? u : 0.0) + STD_EPS);
      o[j] = (float)sd;
      m[j] = (float)mu;
      k[j] = u > 0.0 ? (float)(1.0 / (dd * sd)) : 0.f;
    }
  }
  o.store(out + v * D + c * VEC);
  m.store(mean + v * D + c * VEC);
  k.store(coef + v * D + c * VEC);
}

template <int VEC, int LPR, int KMAX>
__global__ __launch_bounds__(MRG_BLOCK) void segstd_chunk_k(const float* __restrict__ msg, const int32_t* __restrict__ eid,
                                                            const int32_t* __restrict__ chunk_node, const int32_t* __restrict__ chunk_start,
                                                            const int32_t* __restrict__ chunk_end, const int32_t* __restrict__ chunk_slot,
                                                            int64_t n_chunks, const int32_t* __restrict__ in_degree,
                                                            float* __restrict__ out, float* __restrict__ mean, float* __restrict__ coef,
                                                            double* __restrict__ ws, int D) {
  constexpr int RPB = MRG_BLOCK / LPR;
  constexpr int U = KMAX == 1 ? 8 : 4;                      // rows in flight per lane group
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dv = D / VEC;
  for (int64_t ch = (int64_t)blockIdx.x * RPB + rw; ch < n_chunks; ch += (int64_t)gridDim.x * RPB) {
    const int v = chunk_node[ch];
    if (v < 0) continue;                                    // padding beyond the plan's real chunks (capacity-sized launch)
    const int j0 = chunk_start[ch], j1 = chunk_end[ch];
    const int slot = chunk_slot[ch];
    StdAcc<VEC, KMAX> acc;
    acc.init();
    for (int j = j0; j < j1; j += U) {
      int e[U];
#pragma unroll
      for (int u = 0; u < U; ++u) e[u] = (j + u < j1) ? eid[j + u] : -1;
      Vec<VEC> x[U][KMAX];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          const int c = sl + k * LPR;
          if (e[u] >= 0 && c < dv) x[u][k] = Vec<VEC>::load(msg + (int64_t)e[u] * D + c * VEC);
        }
#pragma unroll
      for (int u = 0; u < U; ++u)                           // list order: the association is fixed
        if (e[u] >= 0) {
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (sl + k * LPR < dv) {
#pragma unroll
              for (int i = 0; i < VEC; ++i) {
                const double xd = (double)x[u][k][i];
                acc.s[k][i] += xd;
                acc.q[k][i] += xd * xd;
              }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = sl + k * LPR;
      if (c >= dv) continue;
      if (slot < 0) {
        std_finalize<VEC>(acc.s[k], acc.q[k], v, c, in_degree[v], out, mean, coef, D);
      } else {
        double* w = ws + (int64_t)slot * 2 * D;            // slot layout: D sums of x, then D sums of x^2
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          w[c * VEC + i] = acc.s[k][i];
          w[D + c * VEC + i] = acc.q[k][i];
        }
      }
    }
  }
}

// one workgroup per hub: every thread owns columns and adds the hub's partial slots in list order (eight loads in flight)
__global__ __launch_bounds__(MRG_BLOCK) void segstd_hub_k(const int32_t* __restrict__ hub_node, const int32_t* __restrict__ hub_first,
                                                          const int32_t* __restrict__ hub_count, int64_t n_hubs,
                                                          const int32_t* __restrict__ in_degree, const double* __restrict__ ws,
                                                          float* __restrict__ out, float* __restrict__ mean, float* __restrict__ coef, int D) {
  constexpr int U = 8;
  for (int64_t h = blockIdx.x; h < n_hubs; h += gridDim.x) {
    const int v = hub_node[h];
    if (v < 0) continue;                                    // block-uniform: padding beyond the plan's real hubs
    const int s0 = hub_first[h], cnt = hub_count[h], deg = in_degree[v];
    for (int c = threadIdx.x; c < D; c += MRG_BLOCK) {
      double s = 0.0, q = 0.0;
      for (int b = 0; b < cnt; b += U) {
        double xs[U], xq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool ok = b + u < cnt;
          const double* w = ws + (int64_t)(s0 + (ok ? b + u : 0)) * 2 * D;
          xs[u] = ok ? w[c] : 0.0;
          xq[u] = ok ? w[D + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { s += xs[u]; q += xq[u]; }
      }
      std_finalize<1>(&s, &q, v, c, deg, out, mean, coef, D);
    }
  }
}

template <int VEC, int LPR, int KMAX>
__global__ __launch_bounds__(MRG_BLOCK) void segstd_bwd_k(const float* __restrict__ gout, const float* __restrict__ msg,
                                                          const int32_t* __restrict__ dst, const float* __restrict__ mean,
                                                          const float* __restrict__ coef, const int32_t* __restrict__ order,
                                                          float* __restrict__ gmsg, int64_t E, int D) {
  constexpr int RPB = MRG_BLOCK / LPR;
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dv = D / VEC;
  for (int64_t pos = (int64_t)blockIdx.x * RPB + rw; pos < E; pos += (int64_t)gridDim.x * RPB) {
    const int64_t r = order ? (int64_t)order[pos] : pos;
    const int64_t v = dst[r];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = sl + k * LPR;
      if (c < dv) {
        const Vec<VEC> g = Vec<VEC>::load(gout + v * D + c * VEC);
        const Vec<VEC> m = Vec<VEC>::load(mean + v * D + c * VEC);
        const Vec<VEC> w = Vec<VEC>::load(coef + v * D + c * VEC);
        const Vec<VEC> x = Vec<VEC>::load(msg + r * D + c * VEC);
        Vec<VEC> o;
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = g[j] * w[j] * (x[j] - m[j]);
        o.store(gmsg + r * D + c * VEC);
      }
    }
  }
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_seg_std_workspace_bytes(int64_t n_slots, int D) {
  if (n_slots < 0 || D <= 0) return 0;
  return (n_slots + 1) * (int64_t)D * 16 + 64;            // two float64 rows (sum of x, sum of x^2) per partial slot
}

extern "C" int mrg_seg_std_fwd(const float* msg, const int32_t* eid, const int32_t* chunk_node, const int32_t* chunk_start,
                               const int32_t* chunk_end, const int32_t* chunk_slot, int64_t n_chunks, const int32_t* hub_node,
                               const int32_t* hub_first, const int32_t* hub_count, int64_t n_hubs, int64_t n_slots,
                               const int32_t* in_degree, float* out, float* mean, float* coef, void* ws, int64_t N, int D,
                               void* stream) {
  if (N < 0 || D <= 0 || n_chunks < N || n_hubs < 0 || n_slots < 0) return MRG_E_SHAPE;
  if (N == 0) return MRG_OK;
  if (!out || !mean || !coef || !chunk_node || !chunk_start || !chunk_end || !chunk_slot || !in_degree) return MRG_E_NULLPTR;
  if (n_hubs > 0 && (!hub_node || !hub_first || !hub_count)) return MRG_E_NULLPTR;
  if (n_slots > 0 && !ws) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  RowGeom g = row_geom(D, aligned16(msg) && aligned16(out) && aligned16(mean) && aligned16(coef));
  if (!g.ok) return MRG_E_SHAPE;
  double* wsd = (double*)ws;
#define CALL(V, L, K)                                                                                                             \
  do {                                                                                                                            \
    hipLaunchKernelGGL((segstd_chunk_k<V, L, K>), dim3(grid_for(n_chunks, MRG_BLOCK / L)), dim3(MRG_BLOCK), 0, st, msg, eid,        \
                       chunk_node, chunk_start, chunk_end, chunk_slot, n_chunks, in_degree, out, mean, coef, wsd, D);           \
  } while (0)
  MRG_DISPATCH_GEOM(g, CALL);
#undef CALL
  if (n_hubs > 0) {
    const int gh = n_hubs < 4096 ? (int)n_hubs : 4096;
    hipLaunchKernelGGL(segstd_hub_k, dim3(gh), dim3(MRG_BLOCK), 0, st, hub_node, hub_first, hub_count, n_hubs, in_degree, wsd, out, mean,
                       coef, D);
  }
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_seg_std_bwd(const float* gout, const float* msg, const int32_t* dst, const float* mean, const float* coef,
                               const int32_t* order, float* gmsg, int64_t E, int64_t N, int D, void* stream) {
  if (E < 0 || N < 0 || D <= 0) return MRG_E_SHAPE;
  if (E == 0) return MRG_OK;
  if (!gout || !msg || !dst || !mean || !coef || !gmsg) return MRG_E_NULLPTR;
  hipStream_t st = (hipStream_t)stream;
  RowGeom g = row_geom(D, aligned16(gout) && aligned16(msg) && aligned16(mean) && aligned16(coef) && aligned16(gmsg));
  if (!g.ok) return MRG_E_SHAPE;
#define CALL(V, L, K)                                                                                                             \
  do {                                                                                                                            \
    hipLaunchKernelGGL((segstd_bwd_k<V, L, K>), dim3(grid_for(E, (MRG_BLOCK / L) * 4)), dim3(MRG_BLOCK), 0, st, gout, msg, dst, mean, \
                       coef, order, gmsg, E, D);                                                                                  \
  } while (0)
  MRG_DISPATCH_GEOM(g, CALL);
#undef CALL
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}
