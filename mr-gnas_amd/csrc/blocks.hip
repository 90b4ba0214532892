// Node-classification minibatch blocks with per-layer fan-outs (sampler.NeighborSampler), built from a RESIDENT
// in-edge index: rowptr [N + 1] over destinations, and the edge ids / global sources / types of the graph in stable destination
// order.  One layer of one minibatch is three entry points, none of whose work grows with N or with the graph's edge count:
//   mrg_block_sizes     first[i] = exclusive sum of cnt[i] = min(deg(dst_nodes[i]), k) (deg when k == 0); first[n_dst] = E
//   mrg_block_emit      the block's edge list: per destination its whole in-list, or the k positions Floyd's algorithm picks from
//                       the destination's row of uniforms, ascending; also enters the layer into the two [N] tables
//   mrg_block_relabel   local source indices in first-appearance order, the source-node list, and the tables restored
// The two tables (local: -1 everywhere, firstpos: INT32_MAX everywhere between calls) are only ever touched at the block's own
// nodes.  Integer atomics only (atomicMin: order-independent); every output is a pure function of the inputs.
#include "blocks_parts.hpp"

namespace mrg {

// cnt[i] as the scan reads it; index n_dst (one past the end) is 0, so that the exclusive scan leaves the total in first[n_dst].
// A destination id outside [0, N) has no edges (and is never used as an index).
struct block_count_fn {
  const int64_t* dst_nodes;
  const int32_t* rowptr;
  int64_t n_dst, N;
  int k;
  __device__ int32_t operator()(int32_t i) const {
    if (i >= n_dst) return 0;
    const int64_t v = dst_nodes[i];
    if ((uint64_t)v >= (uint64_t)N) return 0;
    const int32_t d = rowptr[v + 1] - rowptr[v];
    return (k > 0 && d > k) ? k : d;
  }
};

// edge e brings a NEW source (one that is no destination) and is the first edge of the block that does
struct block_fresh_fn {
  const int32_t* gsrc;
  const int32_t* local;
  const int32_t* firstpos;
  __device__ int32_t operator()(int32_t e) const {
    const int32_t s = gsrc[e];
    return (local[s] < 0 && firstpos[s] == e) ? 1 : 0;
  }
};

typedef rocprim::transform_iterator<rocprim::counting_iterator<int32_t>, block_count_fn, int32_t> count_iter;
typedef rocprim::transform_iterator<rocprim::counting_iterator<int32_t>, block_fresh_fn, int32_t> fresh_iter;

struct EmitOut {
  int64_t* eid;        // [E] edge ids in the graph
  int64_t* etype;      // [E] or NULL
  int64_t* ldst;       // [E] local destination
  int32_t* gsrc;       // [E] global source
  int32_t* firstpos;   // [N] table
};

__device__ __forceinline__ void emit_edge(const EmitOut& o, const int32_t* __restrict__ in_eid, const int32_t* __restrict__ in_src,
                                          const int32_t* __restrict__ in_type, int32_t e, int32_t i, int64_t p) {
  const int32_t s = in_src[p];
  o.eid[e] = in_eid[p];
  if (o.etype) o.etype[e] = in_type[p];
  o.ldst[e] = i;
  o.gsrc[e] = s;
  atomicMin(&o.firstpos[s], e);
}

// Workgroups [0, copy_blocks): local[dst_nodes[i]] = i, and ONE LANE PER BLOCK EDGE for the destinations that keep their whole
// in-list (k == 0 or deg <= k) -- the lane finds its destination by bisection of first[], so a hub of millions of in-edges is
// spread over the grid like any other range of edges.  Workgroups [copy_blocks, gridDim.x) (k > 0 only): ONE WAVE PER DESTINATION
// with deg > k -- Floyd's k picks are sequential by nature, each step is one broadcast + one ballot over the picks so far (lane s
// holds pick s), then every lane ranks its pick among the k (ascending positions = ascending edge ids) and writes one edge.
__global__ __launch_bounds__(MRG_BLOCK) void block_emit_k(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ in_eid,
                                                          const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_type,
                                                          const int64_t* __restrict__ dst_nodes, const int32_t* __restrict__ first,
                                                          int32_t n_dst, int64_t N, int k, const double* __restrict__ u, int32_t E,
                                                          int copy_blocks, EmitOut o, int32_t* __restrict__ local) {
  if ((int)blockIdx.x < copy_blocks) {
    const int32_t stride = copy_blocks * MRG_BLOCK, gid = blockIdx.x * MRG_BLOCK + threadIdx.x;
    for (int32_t i = gid; i < n_dst; i += stride) {
      const int64_t v = dst_nodes[i];
      if ((uint64_t)v < (uint64_t)N) local[v] = i;
    }
    for (int64_t e64 = gid; e64 < E; e64 += stride) {
      const int32_t e = (int32_t)e64;
      int32_t lo = 0, hi = n_dst;                              // the destination i with first[i] <= e < first[i + 1]
      while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (first[mid] <= e) lo = mid; else hi = mid;
      }
      const int64_t v = dst_nodes[lo];                         // it has edges, so it is a valid id
      const int32_t r0 = rowptr[v], d = rowptr[v + 1] - r0;
      if (k == 0 || d <= k) emit_edge(o, in_eid, in_src, in_type, e, lo, (int64_t)r0 + (e - first[lo]));
    }
    return;
  }
  const int lane = threadIdx.x & (MRG_WAVE - 1);
  const int32_t wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x - copy_blocks) * (MRG_BLOCK / MRG_WAVE) + threadIdx.x / MRG_WAVE));
  const int32_t n_waves = (gridDim.x - copy_blocks) * (MRG_BLOCK / MRG_WAVE);
  for (int64_t i64 = wave; i64 < n_dst; i64 += n_waves) {
    const int32_t i = (int32_t)i64;
    const int64_t v = dst_nodes[i];
    if ((uint64_t)v >= (uint64_t)N) continue;
    const int32_t r0 = rowptr[v], d = rowptr[v + 1] - r0;
    if (d <= k) continue;                                       // kept whole: the copy lanes wrote it
    const double ul = lane < k ? u[(int64_t)i * k + lane] : 0.0;
    int32_t pick = INT_MAX;
    for (int s = 0; s < k; ++s) {
      const double us = __shfl(ul, s, MRG_WAVE);
      const int32_t j = d - k + s;
      const int32_t t = floyd_candidate(us, j);
      const bool taken = __ballot(lane < s && pick == t) != 0;
      if (lane == s) pick = taken ? j : t;
    }
    int32_t rank = 0;
    for (int m = 0; m < k; ++m) rank += __shfl(pick, m, MRG_WAVE) < pick ? 1 : 0;
    if (lane < k) emit_edge(o, in_eid, in_src, in_type, first[i] + rank, i, (int64_t)r0 + pick);
  }
}

// src_nodes = dst_nodes, then the new sources at their ranks; lsrc[e] = the destination's index when the source is one, else
// n_dst + the rank of the source's first edge.  Reads the tables only.
__global__ __launch_bounds__(MRG_BLOCK) void block_assign_k(const int32_t* __restrict__ gsrc, const int32_t* __restrict__ rank,
                                                            const int32_t* __restrict__ local, const int32_t* __restrict__ firstpos,
                                                            const int64_t* __restrict__ dst_nodes, int32_t n_dst, int32_t E,
                                                            int64_t* __restrict__ src_nodes, int64_t* __restrict__ lsrc,
                                                            int32_t* __restrict__ n_new) {
  const int32_t stride = gridDim.x * MRG_BLOCK, gid = blockIdx.x * MRG_BLOCK + threadIdx.x;
  for (int64_t i = gid; i < n_dst; i += stride) src_nodes[i] = dst_nodes[i];
  for (int64_t e64 = gid; e64 < E; e64 += stride) {
    const int32_t e = (int32_t)e64;
    const int32_t s = gsrc[e], l = local[s], fp = firstpos[s], r = rank[e];
    const bool fresh = l < 0 && fp == e;
    if (fresh) src_nodes[(int64_t)n_dst + r] = s;
    lsrc[e] = l >= 0 ? l : n_dst + rank[fp];
    if (e == E - 1) *n_new = r + (fresh ? 1 : 0);
  }
}

// both tables back to their resting values at the entries this layer touched
__global__ __launch_bounds__(MRG_BLOCK) void block_restore_k(const int32_t* __restrict__ gsrc, const int64_t* __restrict__ dst_nodes,
                                                             int32_t n_dst, int64_t N, int32_t E, int32_t* __restrict__ local,
                                                             int32_t* __restrict__ firstpos) {
  const int32_t stride = gridDim.x * MRG_BLOCK, gid = blockIdx.x * MRG_BLOCK + threadIdx.x;
  for (int64_t e = gid; e < E; e += stride) firstpos[gsrc[e]] = INT_MAX;
  for (int64_t i = gid; i < n_dst; i += stride) {
    const int64_t v = dst_nodes[i];
    if ((uint64_t)v < (uint64_t)N) local[v] = -1;
  }
}

}  // namespace mrg

using namespace mrg;

static bool block_sizes_ok(int64_t n_dst, int64_t N, int k) { return n_dst >= 0 && n_dst < INT_MAX && N >= 0 && k >= 0 && k <= BLOCKS_MAX_FANOUT; }

extern "C" int64_t mrg_block_sizes_workspace_bytes(int64_t n_dst) {
  if (n_dst < 0 || n_dst >= INT_MAX) return 0;
  return (int64_t)scan_temp_bound(n_dst + 1);
}

extern "C" int mrg_block_sizes(const int32_t* rowptr, const int64_t* dst_nodes, int64_t n_dst, int64_t N, int k, int32_t* first, void* ws,
                               int64_t ws_bytes, void* stream) {
  if (!block_sizes_ok(n_dst, N, k)) return MRG_E_SHAPE;
  if (n_dst == 0) return MRG_OK;
  if (!rowptr || !dst_nodes || !first) return MRG_E_NULLPTR;
  if (!ws || ws_bytes < mrg_block_sizes_workspace_bytes(n_dst)) return MRG_E_WORKSPACE;
  count_iter in(rocprim::counting_iterator<int32_t>(0), block_count_fn{dst_nodes, rowptr, n_dst, N, k});
  const int code = scan_into(ws, in, first, n_dst + 1, (hipStream_t)stream);
  if (code != MRG_OK) return code;
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_block_emit(const int32_t* rowptr, const int32_t* in_eid, const int32_t* in_src, const int32_t* in_type,
                              const int64_t* dst_nodes, const int32_t* first, int64_t n_dst, int64_t N, int k, const double* u, int64_t E,
                              int64_t* eid, int64_t* etype, int64_t* ldst, int32_t* gsrc, int32_t* local, int32_t* firstpos, void* stream) {
  if (!block_sizes_ok(n_dst, N, k) || E < 0 || E >= INT_MAX) return MRG_E_SHAPE;
  if (n_dst == 0 || E == 0) return MRG_OK;
  if (!rowptr || !in_eid || !in_src || !dst_nodes || !first || !eid || !ldst || !gsrc || !local || !firstpos) return MRG_E_NULLPTR;
  if ((etype && !in_type) || (k > 0 && !u)) return MRG_E_NULLPTR;
  const int copy_blocks = grid_for(E > n_dst ? E : n_dst, MRG_BLOCK);
  const int pick_blocks = k > 0 ? grid_for(n_dst, MRG_BLOCK / MRG_WAVE) : 0;
  EmitOut o{eid, etype, ldst, gsrc, firstpos};
  hipLaunchKernelGGL(block_emit_k, dim3(copy_blocks + pick_blocks), dim3(MRG_BLOCK), 0, (hipStream_t)stream, rowptr, in_eid, in_src, in_type,
                     dst_nodes, first, (int32_t)n_dst, N, k, u, (int32_t)E, copy_blocks, o, local);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

// Workspace: the scan's temporary storage, then rank int32 [E].
extern "C" int64_t mrg_block_relabel_workspace_bytes(int64_t E) {
  if (E < 0 || E >= INT_MAX) return 0;
  return (int64_t)(scan_temp_bound(E) + up256((size_t)E * 4));
}

extern "C" int mrg_block_relabel(const int32_t* gsrc, const int64_t* dst_nodes, int64_t n_dst, int64_t N, int64_t E, int32_t* local,
                                 int32_t* firstpos, int64_t* src_nodes, int64_t* lsrc, int32_t* n_new, void* ws, int64_t ws_bytes,
                                 void* stream) {
  if (n_dst < 0 || N < 0 || E < 0 || E >= INT_MAX || n_dst + E >= INT_MAX) return MRG_E_SHAPE;
  if (n_dst == 0 || E == 0) return MRG_OK;
  if (!gsrc || !dst_nodes || !local || !firstpos || !src_nodes || !lsrc || !n_new) return MRG_E_NULLPTR;
  if (!ws || ws_bytes < mrg_block_relabel_workspace_bytes(E)) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t* rank = (int32_t*)((char*)ws + scan_temp_bound(E));
  fresh_iter in(rocprim::counting_iterator<int32_t>(0), block_fresh_fn{gsrc, local, firstpos});
  const int code = scan_into(ws, in, rank, E, st);
  if (code != MRG_OK) return code;
  const int grid = grid_for(E > n_dst ? E : n_dst, MRG_BLOCK);
  hipLaunchKernelGGL(block_assign_k, dim3(grid), dim3(MRG_BLOCK), 0, st, gsrc, rank, local, firstpos, dst_nodes, (int32_t)n_dst, (int32_t)E,
                     src_nodes, lsrc, n_new);
  hipLaunchKernelGGL(block_restore_k, dim3(grid), dim3(MRG_BLOCK), 0, st, gsrc, dst_nodes, (int32_t)n_dst, N, (int32_t)E, local, firstpos);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}
