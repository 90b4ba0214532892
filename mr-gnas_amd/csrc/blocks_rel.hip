// Node-classification minibatch blocks with one fan-out PER EDGE TYPE (sampler.NeighborSampler with a per-relation layer; DESIGN
// section 9.9.1), next to blocks.hip's one fan-out over all in-edges.  A RUN (v, r) is the in-edges of destination v with type r in
// ascending edge id; the resident index holds the in-edges in stable (destination, type, edge id) order and the run table:
//   run_ptr [N + 1]        runs before destination v (the runs of v are run_ptr[v] .. run_ptr[v + 1] - 1, types ascending)
//   run_start [n_runs + 1] first position of every run in rel_eid, and the edge count at the end
//   run_type [n_runs]      the run's type
//   rel_eid [E_graph]      edge ids in (destination, type, edge id) order;  src_of / type_of [E_graph]: the graph's own arrays
// A layer's specification is fan[r] per type: -1 every in-edge of the type, 0 none, 1..64 that many (Floyd's picks of blocks.hip with
// d = the run's length).  It comes twice: fan_host [R] for the checks before any launch, spec [2 R] on the device = fan, then the
// column offset of every type in the rows of u [n_dst][K] (K = the sum of the entries >= 1).  One layer is
//   mrg_block_rel_sizes   first[i] = exclusive sum over the destinations of the kept edges of all their runs; first[n_dst] = E
//   mrg_block_rel_emit    keys (local destination, edge id), type by type inside a destination as the runs come; a radix sort of the
//                         keys (the destination bits are in order already: it is the segmented sort by edge id); then every column
//                         of the block from the sorted keys, and the layer entered into the two [N] tables
//   mrg_block_relabel     blocks.hip's, unchanged
// Nothing grows with N or the graph's edge count; integer atomics only (atomicMin); every output is a pure function of the inputs.
#include <rocprim/device/device_radix_sort.hpp>
#include "blocks_parts.hpp"

namespace mrg {

// the specification entry of type r as the kernels read it: a type outside [0, R) keeps nothing, an entry is never above the limit
__device__ __forceinline__ int32_t rel_fan(const int32_t* __restrict__ spec, int R, int32_t r) {
  if ((uint32_t)r >= (uint32_t)R) return 0;
  const int32_t f = spec[r];
  return f > BLOCKS_MAX_FANOUT ? BLOCKS_MAX_FANOUT : f;
}

__device__ __forceinline__ int32_t rel_kept(int32_t d, int32_t f) { return (f < 0 || d <= f) ? d : f; }

struct RelIndex {
  const int32_t* run_ptr;
  const int32_t* run_start;
  const int32_t* run_type;
};

// cnt[i] = the kept edges over the runs of destination i, formed on the fly like block_count_fn of blocks.hip; index n_dst is 0, so
// that the exclusive scan leaves the total in first[n_dst].  ONE WAVE PER DESTINATION, a lane per run: a destination has up to R
// runs and every run costs two dependent loads (its type, then the type's entry), which one lane of the scan's transform iterator
// would walk one after the other (measured: 39 us per layer at 133 types, against 17 us at 45).
__global__ __launch_bounds__(MRG_BLOCK) void block_rel_count_k(RelIndex ix, const int64_t* __restrict__ dst_nodes, int32_t n_dst, int64_t N,
                                                               const int32_t* __restrict__ spec, int R, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & (MRG_WAVE - 1);
  const int32_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (MRG_BLOCK / MRG_WAVE) + threadIdx.x / MRG_WAVE));
  const int32_t n_waves = gridDim.x * (MRG_BLOCK / MRG_WAVE);
  for (int64_t i64 = wave; i64 <= n_dst; i64 += n_waves) {
    const int32_t i = (int32_t)i64;
    const int64_t v = i < n_dst ? dst_nodes[i] : -1;
    int32_t c = 0;
    if ((uint64_t)v < (uint64_t)N)
      for (int32_t q = ix.run_ptr[v] + lane, q1 = ix.run_ptr[v + 1]; q < q1; q += MRG_WAVE)
        c += rel_kept(ix.run_start[q + 1] - ix.run_start[q], rel_fan(spec, R, ix.run_type[q]));
#pragma unroll
    for (int off = MRG_WAVE / 2; off > 0; off >>= 1) c += __shfl_xor(c, off, MRG_WAVE);
    if (lane == 0) cnt[i] = c;
  }
}

__device__ __forceinline__ uint64_t rel_key(int32_t i, int eid_bits, int32_t eid) { return ((uint64_t)(uint32_t)i << eid_bits) | (uint32_t)eid; }

// Workgroups [0, pick_blocks): ONE WAVE PER DESTINATION.  Lane l takes run l of the destination (64 runs at a time, a carry between
// the rounds: a destination may have more runs than a wave has lanes), a wave scan of the kept counts gives every run its place
// inside the destination; then the runs with an integer fan-out share the wave, a lane per kept edge: a run with d <= f is copied,
// one with d > f gets Floyd's f picks in the wave form of block_emit_k (lane s of the run holds pick s, a ballot per step) and
// every lane ranks its pick among its run's and writes one key.  Lane 0 enters the destination into `local`.
// Workgroups [pick_blocks, gridDim.x) (launched only when some type keeps every in-edge; such a run can be millions long): ONE LANE
// PER BLOCK EDGE.  The lane finds its destination by bisection of first[] and its run by walking the destination's runs (at most R
// steps); it writes the key when the run is one that keeps everything and leaves the others to the waves.
__global__ __launch_bounds__(MRG_BLOCK) void block_rel_pick_k(RelIndex ix, const int32_t* __restrict__ rel_eid,
                                                              const int64_t* __restrict__ dst_nodes, const int32_t* __restrict__ first,
                                                              int32_t n_dst, int64_t N, const int32_t* __restrict__ spec, int R,
                                                              const double* __restrict__ u, int K, int32_t E, int eid_bits, int pick_blocks,
                                                              uint64_t* __restrict__ keys, int32_t* __restrict__ local) {
  if ((int)blockIdx.x >= pick_blocks) {
    const int32_t stride = (gridDim.x - pick_blocks) * MRG_BLOCK, gid = (blockIdx.x - pick_blocks) * MRG_BLOCK + threadIdx.x;
    for (int64_t e64 = gid; e64 < E; e64 += stride) {
      const int32_t e = (int32_t)e64;
      int32_t lo = 0, hi = n_dst;                              // the destination i with first[i] <= e < first[i + 1]
      while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (first[mid] <= e) lo = mid; else hi = mid;
      }
      const int64_t v = dst_nodes[lo];                         // it has edges, so it is a valid id
      int32_t o = e - first[lo];
      for (int32_t q = ix.run_ptr[v], q1 = ix.run_ptr[v + 1]; q < q1; ++q) {
        const int32_t s0 = ix.run_start[q], d = ix.run_start[q + 1] - s0, f = rel_fan(spec, R, ix.run_type[q]);
        const int32_t kept = rel_kept(d, f);
        if (o < kept) {
          if (f < 0) keys[e] = rel_key(lo, eid_bits, rel_eid[(int64_t)s0 + o]);
          break;
        }
        o -= kept;
      }
    }
    return;
  }
  const int lane = threadIdx.x & (MRG_WAVE - 1);
  const int32_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (MRG_BLOCK / MRG_WAVE) + threadIdx.x / MRG_WAVE));
  const int32_t n_waves = pick_blocks * (MRG_BLOCK / MRG_WAVE);
  for (int64_t i64 = wave; i64 < n_dst; i64 += n_waves) {
    const int32_t i = (int32_t)i64;
    const int64_t v = dst_nodes[i];
    if ((uint64_t)v >= (uint64_t)N) continue;
    if (lane == 0) local[v] = i;
    const int32_t q0 = ix.run_ptr[v], q1 = ix.run_ptr[v + 1];
    int32_t base = first[i];                                   // where the next run of this destination starts in the block
    for (int32_t qb = q0; qb < q1; qb += MRG_WAVE) {
      const int32_t q = qb + lane;
      const bool valid = q < q1;
      const int32_t s0 = valid ? ix.run_start[q] : 0, d = valid ? ix.run_start[q + 1] - s0 : 0, r = valid ? ix.run_type[q] : -1;
      const int32_t f = rel_fan(spec, R, r), kept = rel_kept(d, f);
      int32_t incl = kept;
#pragma unroll
      for (int off = 1; off < MRG_WAVE; off <<= 1) {
        const int32_t y = __shfl_up(incl, off, MRG_WAVE);
        if (lane >= off) incl += y;
      }
      const int32_t excl = base + incl - kept;
      base += __shfl(incl, MRG_WAVE - 1, MRG_WAVE);
      // A run with an integer fan-out takes need = min(d, f) <= 64 lanes, one per kept edge.  The runs stand SIDE BY SIDE in rounds
      // of 64 lanes, none across a round's end (a destination's many short runs -- 68 of 133 types at [1] * R -- are then one
      // round, not 68 trips of dependent loads): start / end = the run's slots, end nondecreasing over the lanes.
      const int32_t need = f >= 1 ? kept : 0;
      if (__ballot(need > 0) == 0) continue;
      int32_t start = 0, end = 0, cur = 0;
#pragma nounroll
      for (int l = 0; l < MRG_WAVE; ++l) {                     // scalar arithmetic on a wave-uniform counter
        const int32_t n = __builtin_amdgcn_readlane(need, l);
        if ((cur & (MRG_WAVE - 1)) + n > MRG_WAVE) cur = (cur + MRG_WAVE - 1) & ~(MRG_WAVE - 1);
        if (lane == l) start = cur;
        cur += n;
        if (lane == l) end = cur;
      }
      for (int32_t t0 = 0; t0 < cur; t0 += MRG_WAVE) {
        const int32_t t = t0 + lane;
        int o = 0;                                             // the slot's run: the first lane whose end lies beyond t
#pragma unroll
        for (int step = MRG_WAVE / 2; step > 0; step >>= 1)
          if (__shfl(end, o + step - 1, MRG_WAVE) <= t) o += step;
        // every cross-lane read below stands in wave-uniform control flow: a lane that owns a run need not own a slot of this round,
        // and a read from a lane that sits out a branch returns 0
        const int32_t o_end = __shfl(end, o, MRG_WAVE), o_start = __shfl(start, o, MRG_WAVE), o_f = __shfl(f, o, MRG_WAVE);
        const int32_t od = __shfl(d, o, MRG_WAVE), at = __shfl(excl, o, MRG_WAVE), ss = __shfl(s0, o, MRG_WAVE), orr = __shfl(r, o, MRG_WAVE);
        const bool mine = o_end > t && o_start <= t;           // else a padding slot
        const int32_t seg0 = mine ? o_start - t0 : 0;          // the run's first lane in this round
        const int32_t of = mine ? o_f : 0, s = lane - seg0;
        // Floyd's picks of the runs with d > f in the wave form of block_emit_k: lane seg0 + s holds pick s of its run, one ballot
        // per step, read through the mask of the run's lanes
        const bool cut = mine && od > of;
        const int32_t col = cut ? spec[R + orr] : -1;          // of >= 1, so the type is inside [0, R)
        const double ul = (cut && col >= 0 && col + of <= K) ? u[(int64_t)i * K + col + s] : 0.0;
        const unsigned long long run_lanes = (of >= MRG_WAVE ? ~0ull : ((1ull << of) - 1)) << seg0;
        int32_t pick = INT_MAX;
        for (int s2 = 0; __ballot(cut && s2 < of) != 0; ++s2) {
          const double us = __shfl(ul, (seg0 + s2) & (MRG_WAVE - 1), MRG_WAVE);
          const int32_t j = od - of + s2;
          const int32_t c = floyd_candidate(us, j);
          const bool taken = (__ballot(cut && s < s2 && pick == c) & run_lanes) != 0;
          if (cut && s == s2) pick = taken ? j : c;
        }
        int32_t rank = 0;
        for (int m = 0; __ballot(cut && m < of) != 0; ++m) {
          const int32_t other = __shfl(pick, (seg0 + m) & (MRG_WAVE - 1), MRG_WAVE);
          if (cut && m < of && other < pick) ++rank;
        }
        // a run kept whole (d <= f) copies position s to place s; a position outside the run is never used as an index
        const int32_t pos = cut ? pick : s;
        if (mine && (uint32_t)pos < (uint32_t)od) keys[at + (cut ? rank : s)] = rel_key(i, eid_bits, rel_eid[(int64_t)ss + pos]);
      }
    }
  }
}

// every column of the block from the sorted keys: one lane per block edge
__global__ __launch_bounds__(MRG_BLOCK) void block_rel_fill_k(const uint64_t* __restrict__ keys, const int32_t* __restrict__ src_of,
                                                              const int32_t* __restrict__ type_of, int32_t E_graph, int32_t E,
                                                              int eid_bits, int64_t* __restrict__ eid, int64_t* __restrict__ etype,
                                                              int64_t* __restrict__ ldst, int32_t* __restrict__ gsrc,
                                                              int32_t* __restrict__ firstpos) {
  const int32_t stride = gridDim.x * MRG_BLOCK, gid = blockIdx.x * MRG_BLOCK + threadIdx.x;
  const uint64_t mask = ((uint64_t)1 << eid_bits) - 1;
  for (int64_t e64 = gid; e64 < E; e64 += stride) {
    const int32_t e = (int32_t)e64;
    const uint64_t key = keys[e];
    int32_t id = (int32_t)(key & mask);
    if ((uint32_t)id >= (uint32_t)E_graph) id = 0;             // an id outside the graph is never used as an index
    const int32_t s = src_of[id];
    eid[e] = id;
    if (etype) etype[e] = type_of[id];
    ldst[e] = (int64_t)(key >> eid_bits);
    gsrc[e] = s;
    atomicMin(&firstpos[s], e);
  }
}

// Temporary storage of the key sort as the workspace query sizes it: a HOST formula like scan_temp_bound, 64 KiB + 32 bytes per key
// (rocprim takes a second key buffer of 8 bytes per key, digit counters of a few KiB, and per workgroup of >= 1 024 keys a few hundred
// look-back states of 4 bytes or merge bounds).  sort_temp_check holds it against rocprim's own figure before anything is launched.
static size_t sort_temp_bound(int64_t n) { return up256(65536 + 32 * (size_t)n); }

static int sort_temp_check(int64_t n, int bits, hipStream_t st) {
  size_t need = 0;
  const hipError_t e = rocprim::radix_sort_keys(nullptr, need, (const uint64_t*)nullptr, (uint64_t*)nullptr, (unsigned int)n, 0u, (unsigned int)bits, st);
  if (e != hipSuccess) return (int)e;
  return need > sort_temp_bound(n) ? MRG_E_WORKSPACE : MRG_OK;
}

static int sort_keys(void* temp, const uint64_t* in, uint64_t* out, int64_t n, int bits, hipStream_t st) {
  size_t have = sort_temp_bound(n);
  const hipError_t e = rocprim::radix_sort_keys(temp, have, in, out, (unsigned int)n, 0u, (unsigned int)bits, st);
  return e != hipSuccess ? (int)e : MRG_OK;
}

static int bit_length(int64_t x) {
  int b = 0;
  while (x > 0) { ++b; x >>= 1; }
  return b;
}

// the specification on the host: every entry -1..64; *K = the sum of the entries >= 1, *whole = some type keeps every in-edge
static bool rel_spec_ok(const int32_t* fan_host, int R, int64_t* K, bool* whole) {
  *K = 0;
  *whole = false;
  for (int r = 0; r < R; ++r) {
    const int32_t f = fan_host[r];
    if (f < -1 || f > BLOCKS_MAX_FANOUT) return false;
    if (f > 0) *K += f;
    if (f < 0) *whole = true;
  }
  return true;
}

}  // namespace mrg

using namespace mrg;

static bool rel_sizes_ok(int64_t n_dst, int64_t N, int R) { return n_dst >= 0 && n_dst < INT_MAX && N >= 0 && R >= 1 && R <= (INT_MAX >> 7); }

// Workspace: the scan's temporary storage, then cnt int32 [n_dst + 1].
extern "C" int64_t mrg_block_rel_sizes_workspace_bytes(int64_t n_dst) {
  if (n_dst < 0 || n_dst >= INT_MAX) return 0;
  return (int64_t)(scan_temp_bound(n_dst + 1) + up256((size_t)(n_dst + 1) * 4));
}

extern "C" int mrg_block_rel_sizes(const int32_t* run_ptr, const int32_t* run_start, const int32_t* run_type, const int64_t* dst_nodes,
                                   int64_t n_dst, int64_t N, const int32_t* fan_host, const int32_t* spec, int R, int32_t* first, void* ws,
                                   int64_t ws_bytes, void* stream) {
  if (!rel_sizes_ok(n_dst, N, R)) return MRG_E_SHAPE;
  if (!fan_host) return MRG_E_NULLPTR;
  int64_t K;
  bool whole;
  if (!rel_spec_ok(fan_host, R, &K, &whole)) return MRG_E_SHAPE;
  if (n_dst == 0) return MRG_OK;
  if (!run_ptr || !run_start || !run_type || !dst_nodes || !spec || !first) return MRG_E_NULLPTR;
  if (!ws || ws_bytes < mrg_block_rel_sizes_workspace_bytes(n_dst)) return MRG_E_WORKSPACE;
  int32_t* cnt = (int32_t*)((char*)ws + scan_temp_bound(n_dst + 1));
  hipLaunchKernelGGL(block_rel_count_k, dim3(grid_for(n_dst + 1, MRG_BLOCK / MRG_WAVE)), dim3(MRG_BLOCK), 0, (hipStream_t)stream,
                     RelIndex{run_ptr, run_start, run_type}, dst_nodes, (int32_t)n_dst, N, spec, R, cnt);
  const int code = scan_into(ws, (const int32_t*)cnt, first, n_dst + 1, (hipStream_t)stream);
  if (code != MRG_OK) return code;
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

// Workspace: the unsorted keys uint64 [E], the sorted keys uint64 [E], then the sort's temporary storage.
extern "C" int64_t mrg_block_rel_emit_workspace_bytes(int64_t E) {
  if (E < 0 || E >= INT_MAX) return 0;
  return (int64_t)(2 * up256((size_t)E * 8) + sort_temp_bound(E));
}

extern "C" int mrg_block_rel_emit(const int32_t* run_ptr, const int32_t* run_start, const int32_t* run_type, const int32_t* rel_eid,
                                  const int32_t* src_of, const int32_t* type_of, int64_t E_graph, const int64_t* dst_nodes,
                                  const int32_t* first, int64_t n_dst, int64_t N, const int32_t* fan_host, const int32_t* spec, int R,
                                  const double* u, int64_t K, int64_t E, int64_t* eid, int64_t* etype, int64_t* ldst, int32_t* gsrc,
                                  int32_t* local, int32_t* firstpos, void* ws, int64_t ws_bytes, void* stream) {
  if (!rel_sizes_ok(n_dst, N, R) || E < 0 || E >= INT_MAX || E_graph < 0 || E_graph >= INT_MAX) return MRG_E_SHAPE;
  if (!fan_host) return MRG_E_NULLPTR;
  int64_t k_sum;
  bool whole;
  if (!rel_spec_ok(fan_host, R, &k_sum, &whole) || K != k_sum) return MRG_E_SHAPE;
  if (n_dst == 0 || E == 0) return MRG_OK;
  if (!run_ptr || !run_start || !run_type || !rel_eid || !src_of || !dst_nodes || !first || !spec || !eid || !ldst || !gsrc || !local ||
      !firstpos)
    return MRG_E_NULLPTR;
  if ((etype && !type_of) || (K > 0 && !u)) return MRG_E_NULLPTR;
  if (!ws || ws_bytes < mrg_block_rel_emit_workspace_bytes(E)) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint64_t* keys = (uint64_t*)ws;
  uint64_t* sorted = (uint64_t*)((char*)ws + up256((size_t)E * 8));
  void* temp = (char*)ws + 2 * up256((size_t)E * 8);
  const int eid_bits = bit_length(E_graph > 1 ? E_graph - 1 : 1), dst_bits = bit_length(n_dst - 1);
  const int pick_blocks = grid_for(n_dst, MRG_BLOCK / MRG_WAVE), copy_blocks = whole ? grid_for(E, MRG_BLOCK) : 0;
  int code = sort_temp_check(E, eid_bits + dst_bits, st);
  if (code != MRG_OK) return code;
  hipLaunchKernelGGL(block_rel_pick_k, dim3(pick_blocks + copy_blocks), dim3(MRG_BLOCK), 0, st, RelIndex{run_ptr, run_start, run_type},
                     rel_eid, dst_nodes, first, (int32_t)n_dst, N, spec, R, u, (int)K, (int32_t)E, eid_bits, pick_blocks, keys, local);
  code = sort_keys(temp, keys, sorted, E, eid_bits + dst_bits, st);
  if (code != MRG_OK) return code;
  hipLaunchKernelGGL(block_rel_fill_k, dim3(grid_for(E, MRG_BLOCK)), dim3(MRG_BLOCK), 0, st, sorted, src_of, type_of, (int32_t)E_graph, (int32_t)E,
                     eid_bits, eid, etype, ldst, gsrc, firstpos);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}
