// Top-k link prediction without a [Q, N] tensor: the parts the "dot" sweep on the row GEMM (topk.hip, EPI_TOPK) and the "l1" sweep
// (transe_1n.hip, L1_TOPK) share -- the order, the per-tile selection, the merge kernel and the sizing of the partial lists.
//
// Order.  Candidate a comes before candidate b iff its value is better (DESC: greater, a logit; else smaller, a distance) or equal at
// the lower entity id: the rule of mrg_rank_filtered and gemm_epilogue_rank, so position j + 1 of a list is the rank the rank sweeps
// give its entry.  A filtered or absent candidate is (pad, TOPK_NONE): pad is the worst value and TOPK_NONE is above every entity id,
// so it comes after every real candidate, one with the value pad included.  A NaN compares false both ways and is never selected.
//
// Selection (topk_select).  A sweep holds a query row's tile columns spread over W consecutive lanes, E values per lane in registers
// (the row GEMM's accumulator layout: W = 32, E = column tiles; the L1 micro-tiles: W = 16, E = 4).  Round t finds the best candidate
// that comes strictly after round t - 1's pick: every lane scans its E registers, a butterfly over the W lanes agrees on the winner.
// Nothing is marked or moved, so the registers are indexed by constants only (no scratch) and no LDS is used; the cost is
// k * (E compares + log2 W exchanges) per row and tile, paid once per tile at inference.  The group's first lane stores the pairs of
// the row's tile list at part[(row * tiles + tile) * k + t], up to and including the first padding pair: nothing behind it is read.
// Pruning: a candidate that does not come before the k-th entry of the query's running list (the k best of the column blocks swept
// so far; empty in the first block) cannot enter the result, so it is dropped before the rounds, and the rounds end as soon as no
// row of the wave has a candidate left.  From the second block on that is after a round or two.  The test is the order itself, so
// the result is the one an unpruned sweep gives.
//
// Merge (topk_merge_k).  After each column block one wave per query folds the block's tile lists and the query's running list
// ids / vals [k] -- all sorted -- into the new running list: lane l holds the heads of lists l, l + 64, ..., a butterfly picks the
// best head, its owner steps that list's cursor, lane t keeps pick t, and the k lanes store once every read is done.  Entity ids
// are distinct across tiles and blocks, so the order is total and the result does not depend on how N was cut.  No atomics.
#pragma once
#include <limits>
#include "sweep_host.hpp"

namespace mrg {

constexpr int TOPK_MAX_K = 64;                         // one lane per pick in the merge; a tile has at least as many columns
constexpr int TOPK_NONE = 0x7fffffff;                  // the id of a filtered / absent candidate inside the kernels (stored as -1)
constexpr int TOPK_MERGE_LISTS = 8;                    // list heads per lane of the merge: 8 * 64 lists
constexpr int64_t TOPK_PART_BYTES = 16ll << 20;        // budget of the per-(row, tile) partial lists of one launch

struct __attribute__((aligned(8))) TopkEnt { float v; int id; };

template <bool DESC>
__host__ __device__ constexpr float topk_pad() { return DESC ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity(); }

template <bool DESC>
__device__ __forceinline__ bool topk_before(float av, int aid, float bv, int bid) {
  return (DESC ? av > bv : av < bv) || (av == bv && aid < bid);
}

// v / id: this lane's E candidates of the row (id = TOPK_NONE, v = pad for a filtered or absent one); (kv, kid): the k-th entry of the
// row's running list, (pad, -1) while it has fewer than k.  Every lane of the wave calls it; `store`: the row exists.
template <bool DESC, int W, int E>
__device__ __forceinline__ void topk_select(float (&v)[E], int (&id)[E], float kv, int kid, int k, TopkEnt* __restrict__ out, bool store) {
  kid = kid < 0 ? TOPK_NONE : kid;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const bool keep = topk_before<DESC>(v[e], id[e], kv, kid);
    v[e] = keep ? v[e] : topk_pad<DESC>();
    id[e] = keep ? id[e] : TOPK_NONE;
  }
  float pv = topk_pad<!DESC>();                        // "before everything": the best value at an id below every entity's
  int pid = -1;
  const bool lead = store && (threadIdx.x & (W - 1)) == 0;
  for (int t = 0; t < k; ++t) {
    float bv = topk_pad<DESC>();
    int bid = TOPK_NONE;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const bool take = topk_before<DESC>(pv, pid, v[e], id[e]) && topk_before<DESC>(v[e], id[e], bv, bid);
      bv = take ? v[e] : bv;
      bid = take ? id[e] : bid;
    }
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oid = __shfl_xor(bid, off);
      const bool take = topk_before<DESC>(ov, oid, bv, bid);
      bv = take ? ov : bv;
      bid = take ? oid : bid;
    }
    pv = bv; pid = bid;
    if (lead) out[t] = TopkEnt{bv, bid == TOPK_NONE ? -1 : bid};
    if (!__any(bid != TOPK_NONE)) break;               // wave-uniform: every row's list has its closing padding pair
  }
}

// One wave per query row; 256 threads = 4 rows.  part: [rows][ntile][k]; ids / vals: the rows' running lists [rows][k].
template <bool DESC>
static __global__ __launch_bounds__(256) void topk_merge_k(const TopkEnt* __restrict__ part, int ntile, int k, int64_t rows, int32_t* ids,
                                                           float* vals) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                             // wave-uniform
  const TopkEnt* __restrict__ prow = part + row * ntile * k;
  int32_t* rid = ids + row * k;
  float* rv = vals + row * k;
  const int nlists = ntile + 1;                        // list 0: the running list
  auto head = [&](int list, int c) {
    TopkEnt h{topk_pad<DESC>(), TOPK_NONE};
    if (list < nlists && c < k) {
      const TopkEnt g = list == 0 ? TopkEnt{rv[c], rid[c]} : prow[(int64_t)(list - 1) * k + c];
      if (g.id >= 0) h = g;
    }
    return h;
  };
  TopkEnt h[TOPK_MERGE_LISTS];
  int cur[TOPK_MERGE_LISTS];
#pragma unroll
  for (int j = 0; j < TOPK_MERGE_LISTS; ++j) { cur[j] = 0; h[j] = head(lane + 64 * j, 0); }
  float resv = topk_pad<DESC>();
  int resid = TOPK_NONE;
  for (int t = 0; t < k; ++t) {
    float bv = topk_pad<DESC>();
    int bid = TOPK_NONE, bl = 0;
#pragma unroll
    for (int j = 0; j < TOPK_MERGE_LISTS; ++j) {
      const bool take = topk_before<DESC>(h[j].v, h[j].id, bv, bid);
      bv = take ? h[j].v : bv;
      bid = take ? h[j].id : bid;
      bl = take ? lane + 64 * j : bl;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oid = __shfl_xor(bid, off), ol = __shfl_xor(bl, off);
      const bool take = topk_before<DESC>(ov, oid, bv, bid);
      bv = take ? ov : bv;
      bid = take ? oid : bid;
      bl = take ? ol : bl;
    }
    if (lane == t) { resv = bv; resid = bid; }
    if (bid != TOPK_NONE && (bl & 63) == lane) {       // the owner steps the winning list
#pragma unroll
      for (int j = 0; j < TOPK_MERGE_LISTS; ++j)
        if (j == (bl >> 6)) { cur[j] += 1; h[j] = head(bl, cur[j]); }
    }
  }
  // every read of the running list fed a comparison above: the stores below follow them in program order
  if (lane < k) {
    rid[lane] = resid == TOPK_NONE ? -1 : resid;
    rv[lane] = resid == TOPK_NONE ? topk_pad<DESC>() : resv;
  }
}

template <bool DESC>
static inline int topk_merge_launch(const TopkEnt* part, int ntile, int k, int64_t rows, int32_t* ids, float* vals, hipStream_t st) {
  hipLaunchKernelGGL(topk_merge_k<DESC>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, part, ntile, k, rows, ids, vals);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

inline bool topk_k_ok(int k) { return k >= 1 && k <= TOPK_MAX_K; }

// bytes of one row's partial lists in a launch: one list of k pairs per column tile of a block of at most BCE_COLS columns
inline int64_t topk_row_bytes(int64_t N, int k, int tile_cols) {
  const int64_t nc = N < BCE_COLS ? N : BCE_COLS;
  return (nc + tile_cols - 1) / tile_cols * k * (int64_t)sizeof(TopkEnt);
}
// rows per launch: whole row tiles, as many as keep the launch's partial lists within TOPK_PART_BYTES, at most RANK_CHUNK
inline int64_t topk_row_chunk(int64_t N, int k, int tile_rows, int tile_cols) {
  int64_t rows = TOPK_PART_BYTES / topk_row_bytes(N, k, tile_cols) / tile_rows * tile_rows;
  rows = rows < tile_rows ? tile_rows : rows;
  return rows < RANK_CHUNK ? rows : RANK_CHUNK;
}
// what topk_row_chunk relies on: one row tile of the largest lists fits the budget, and the merge holds every list of a block
template <int TILE_ROWS, int TILE_COLS>
struct TopkTileCheck {
  static_assert(TILE_COLS >= TOPK_MAX_K, "a tile list has k entries");
  static_assert((BCE_COLS + TILE_COLS - 1) / TILE_COLS + 1 <= TOPK_MERGE_LISTS * 64, "list heads of the merge");
  static_assert((BCE_COLS + TILE_COLS - 1) / TILE_COLS * TOPK_MAX_K * (int64_t)sizeof(TopkEnt) * TILE_ROWS <= TOPK_PART_BYTES, "partial budget");
  static constexpr bool ok = true;
};

struct TopkPlan { size_t ent_split, qinfo, part, total; int64_t chunk; };
// split_bytes: the row GEMM's split table of one column block (0 for the L1 sweep and the exact core)
inline TopkPlan topk_plan(int64_t Q, int64_t N, int k, int tile_rows, int tile_cols, size_t split_bytes) {
  TopkPlan p{};
  p.chunk = topk_row_chunk(N, k, tile_rows, tile_cols);
  const int64_t rows = Q < p.chunk ? Q : p.chunk;
  size_t off = 256;                                          // slack: the workspace pointer is rounded up to 256 bytes
  p.ent_split = off; off += sweep_up(split_bytes);
  p.qinfo = off; off += sweep_up((size_t)Q * 4 * sizeof(int32_t));
  p.part = off; off += sweep_up((size_t)rows * (size_t)topk_row_bytes(N, k, tile_cols));
  p.total = off;
  return p;
}

}  // namespace mrg
