// The parts the register-tiled [queries, entities] sweeps share: l1_sweep_k (transe_1n.hip) and mix_sweep_k<NS> (sf_mix_1n.hip).  256
// threads own a tile of SWT_T queries x SWT_T entities as a 16 x 16 grid of 4 x 4 micro-tiles (tx = tid & 15 the entity side, ty =
// tid >> 4 the query side); operands travel through LDS in slices of SWT_C columns laid out [c][row].  Each part is written ONCE
// because the kernels are only correct where they agree bit for bit: a sweep with its target kernel, the three-way sweep at w2 = 0
// with the two-way one, every dist with transe_fwd_k's.  What is fixed here:
//   staging    thread (r = tid & 63, part = tid >> 6) carries row r of an operand, 8 of a slice's 32 columns; a column at or beyond D
//              and a row beyond the launch's are staged as exact zeros (|o - e| and q * e add nothing to a chain).  mix_sweep_k's;
//              l1_sweep_k keeps the same two loops written out for its two operands
//   mask       the labels (LOSS / GRAD: qlist) or filtered members (RANK / TOPK: qinfo, gone_at > when) of a tile row among the
//              tile's 64 entities as bits: binary search for the first member >= the tile's first entity, then the walk
//   rank count hits per row over the 16 lanes tx, one integer atomic per (row, workgroup); the tie rule is
//              beats(v, t) || (v == t && id < target), the lower id first
//   partials   float64: lane sums in register order (the caller's loop), butterfly per wave, the four waves added in order, NSUM
//              values per workgroup laid out [workgroup][NSUM].  No float atomics anywhere.
#pragma once
#include "common.hpp"

namespace mrg {

constexpr int SWT_T = 64;           // tile: 64 queries x 64 entities
constexpr int SWT_C = 32;           // columns per LDS slice

// 8 of the 32 columns [c0, c0 + 32) of row p into v.  VEC4 (D % 4 == 0, 16-byte aligned rows): columns c .. c + 3 twice
template <bool VEC4>
__device__ __forceinline__ void sweep_fetch(const float* __restrict__ p, bool ok, int c0, int part, int D, float (&v)[8]) {
  if constexpr (VEC4) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = c0 + (part + 4 * h) * 4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < D && ok) x = *reinterpret_cast<const float4*>(p + c);
      v[h * 4] = x.x; v[h * 4 + 1] = x.y; v[h * 4 + 2] = x.z; v[h * 4 + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c0 + part + 4 * k;
      v[k] = (ok && c < D) ? p[c] : 0.f;
    }
  }
}

// v into column r of the slice: the lanes of a wave write 64 consecutive floats of one [c] row, conflict free
template <bool VEC4>
__device__ __forceinline__ void sweep_stash(float (&s)[SWT_C][SWT_T], int r, int part, const float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) s[VEC4 ? (part + 4 * (k >> 2)) * 4 + (k & 3) : part + 4 * k][r] = v[k];
}

// The mask of tile row `row` of launch `a` over the 64 entities from column col0 of the launch; 0 for a row beyond the launch.  ARGS: the kernel's
// argument struct (rows, list, and qinfo / gone_at or qlist).  FILTERS: a.qinfo [rows][4] (target, begin, end, when) and a member
// counts iff gone_at > when; else a.qlist [rows][2] (begin, end) and every member counts.
template <bool FILTERS, class ARGS>
__device__ __forceinline__ unsigned long long sweep_tile_mask(const ARGS& a, int64_t row, int col0) {
  unsigned long long m = 0ull;
  if (row < a.rows) {
    int lo, hi, when = 0;
    if constexpr (FILTERS) {
      const int4 qi = *reinterpret_cast<const int4*>(a.qinfo + row * 4);
      lo = qi.y; hi = qi.z; when = qi.w;
    } else {
      const int2 q = *reinterpret_cast<const int2*>(a.qlist + row * 2);
      lo = q.x; hi = q.y;
    }
    if (lo < hi) {
      const int cbeg = a.e0 + col0, cend = cbeg + SWT_T;
      int b = lo, e = hi;
      while (b < e) {                                        // first member >= cbeg
        const int mid = b + ((e - b) >> 1);
        if (a.list[mid] < cbeg) b = mid + 1; else e = mid;
      }
      for (; b < hi; ++b) {
        const int id = a.list[b];
        if (id >= cend) break;
        if constexpr (FILTERS) { if (a.gone_at[b] > when) m |= 1ull << (id - cbeg); }
        else m |= 1ull << (id - cbeg);
      }
    }
  }
  return m;
}

// What an epilogue knows of the thread's 4 x 4 elements: element (i, j) is (row0 + ty * 4 + i, col0 + tx * 4 + j); (mrow[i] >> j) & 1
// is its mask bit, rok[i] / cok[j] say whether its row / column is inside the launch.  (Three plain arrays of the kernel, not a struct:
// l1_sweep_k's instructions stay where they were.)
__device__ __forceinline__ void sweep_edges(const unsigned long long* smask, int tx, int ty, int64_t row0, int col0, int64_t rows, int ncols,
                                            unsigned long long (&mrow)[4], bool (&rok)[4], bool (&cok)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mrow[i] = smask[ty * 4 + i] >> (tx * 4);
    rok[i] = row0 + ty * 4 + i < rows;
    cok[i] = col0 + tx * 4 + i < ncols;
  }
}

// counts[row] += #{unfiltered e != target of the tile : value(i, j) beats the target's, or ties with it at a lower id}.  LESS: the
// smaller value wins (a distance); else the larger (a probability).  tval [rows]: the targets' values from the target kernel, which
// runs the sweep's chains; qinfo[row * 4] the target's id.  scnt: SWT_T counters in LDS.  id0: the entity id of the tile's column 0.
template <bool LESS, class VALUE>
__device__ __forceinline__ void sweep_rank_count(const unsigned long long (&mrow)[4], const bool (&rok)[4], const bool (&cok)[4], int tid, int64_t row0, int64_t rows, int id0, const float* __restrict__ tval,
                                                 const int32_t* __restrict__ qinfo, unsigned* scnt, unsigned* __restrict__ counts, VALUE&& value) {
  const int tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = row0 + ty * 4 + i;
    const int64_t rc = rok[i] ? row : rows - 1;
    const float vt = tval[rc];
    const int tg = qinfo[rc * 4];
    unsigned n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int id = id0 + tx * 4 + j;
      const float v = value(i, j);
      const bool hit = rok[i] && cok[j] && id != tg && !((mrow[i] >> j) & 1ull) && ((LESS ? v < vt : v > vt) || (v == vt && id < tg));
      n += hit ? 1u : 0u;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) n += __shfl_xor(n, off);         // the 16 lanes tx of micro-tile row ty are consecutive
    if (tx == 0) scnt[ty * 4 + i] = n;
  }
  __syncthreads();
  if (tid < SWT_T && row0 + tid < rows && scnt[tid]) atomicAdd(counts + row0 + tid, scnt[tid]);
}

// partial[NSUM] of this workgroup = the workgroup's sums of the threads' s[NSUM]: butterfly per wave, the four waves added in order
template <int NSUM>
__device__ __forceinline__ void sweep_partials(double (&s)[NSUM], double (&sred)[NSUM][4], int tid, double* __restrict__ partial) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < NSUM; ++k) s[k] += __shfl_xor(s[k], off);
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < NSUM; ++k) sred[k][tid >> 6] = s[k];
  __syncthreads();
  if (tid < NSUM) partial[tid] = ((sred[tid][0] + sred[tid][1]) + sred[tid][2]) + sred[tid][3];
}

// one (query, entity) term of the loss on a probability p and its label value y (EPI_BCE's term, gemm.hpp)
__device__ __forceinline__ float sweep_bce_term(float p, float y) {
  const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
  return (y - 1.f) * lq - y * lp;
}

}  // namespace mrg
