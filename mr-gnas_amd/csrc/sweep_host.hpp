// Host code the [queries, entities] sweeps that keep no [B, N] tensor share (bce.hip, rank.hip on the row GEMM; transe_1n.hip): the launch
// bounds, the workspace's rounding and base, the argument checks, the launch grid of a blocked sweep and the launch of sweep_prep.hpp's
// kernels.  Which core a shape takes (rank_split_core, the aligned16 conditions, VEC4) stays in the file that owns the core.
#pragma once
#include "common.hpp"
#include "sweep_prep.hpp"

namespace mrg {

constexpr int64_t RANK_CHUNK = 8192;          // queries per sweep launch: bounds the [chunk, D] operands of the workspace and grid.x
constexpr int RANK_NT = 7;                    // column tiles per block of the row GEMM's sweep
constexpr int64_t RANK_MAX_N = 65535LL * RANK_NT * 32;     // grid.y
constexpr int64_t BCE_COLS = (int64_t)RANK_NT * 32 * 128;      // entity columns per sweep launch (28 672): bounds the split table

inline size_t sweep_up(size_t x) { return (x + 255) & ~(size_t)255; }

// The base the plans' offsets count from.  They start at 256: the slack that lets the workspace pointer be rounded up to 256 bytes.
inline char* sweep_ws_base(void* ws) { return (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255) - 256; }

// row_gemm: the row GEMM's cores take D <= 256, or beyond it a multiple of 4
inline bool sweep_shape_ok(int64_t rows, int64_t N, int D, bool row_gemm) {
  return rows >= 0 && N >= 1 && N <= RANK_MAX_N && D >= 1 && D <= 1024 && (!row_gemm || D <= 256 || D % 4 == 0);
}

// the label (filter) pointers may be NULL only when there is no list at all
template <class... P>
inline bool sweep_labels_ok(int64_t U, const P*... p) { return U <= 0 || (... && (p != nullptr)); }

// The launch grid of a blocked sweep over the columns [c0, c1) of rows_all rows in workgroup tiles of tile_rows x tile_cols: column blocks
// of BCE_COLS outermost (the row GEMM splits the entity rows once per block), row chunks of row_chunk inside.  The ONE definition of
// it: a sweep launches through each(), a plan sizes the per-workgroup partials with workgroups(), which walks the same loop.
struct SweepGrid {
  int64_t rows_all, c0, c1;
  int tile_rows, tile_cols;
  int64_t row_chunk = RANK_CHUNK;     // rows per launch; a sweep that keeps per-(row, tile) partials sets less (topk_parts.hpp)
  unsigned row_tiles(int64_t rows) const { return (unsigned)((rows + tile_rows - 1) / tile_rows); }
  unsigned col_tiles(int64_t nc) const { return (unsigned)((nc + tile_cols - 1) / tile_cols); }
  // launch(q0, rows, c, nc, wg0): rows [q0, q0 + rows) x columns [c, c + nc) on a grid of row_tiles(rows) x col_tiles(nc) workgroups;
  // wg0 counts the workgroups of the launches before it (where a launch appends its partials).  An error ends the walk and is returned.
  template <class F>
  int each(F&& launch, int64_t* total = nullptr) const {
    int64_t wg = 0;
    for (int64_t c = c0; c < c1; c += BCE_COLS) {
      const int64_t nc = c1 - c < BCE_COLS ? c1 - c : BCE_COLS;
      for (int64_t q0 = 0; q0 < rows_all; q0 += row_chunk) {
        const int64_t rows = rows_all - q0 < row_chunk ? rows_all - q0 : row_chunk;
        const int rc = launch(q0, rows, c, nc, wg);
        if (rc != MRG_OK) return rc;
        wg += (int64_t)row_tiles(rows) * col_tiles(nc);
      }
    }
    if (total) *total = wg;
    return MRG_OK;
  }
  int64_t workgroups() const {
    int64_t n = 0;
    each([](int64_t, int64_t, int64_t, int64_t, int64_t) { return (int)MRG_OK; }, &n);
    return n;
  }
};

// The workspace of a 1-N loss / gradient call of the register-tiled sweeps (transe_1n.hip, sf_mix_1n.hip): the queries' label lists
// qlist [B][2] and nsums float64 partials per workgroup of the sweep's grid.
struct SweepBcePlan { size_t qlist, partial, total; int64_t nparts; };
inline SweepBcePlan sweep_bce_plan(const SweepGrid& grid, int64_t B, int nsums) {
  SweepBcePlan p{};
  p.nparts = grid.workgroups();
  size_t off = 256;                                          // slack: the workspace pointer is rounded up to 256 bytes
  p.qlist = off; off += sweep_up((size_t)B * 2 * sizeof(int32_t));
  p.partial = off; off += sweep_up((size_t)p.nparts * nsums * sizeof(double));
  p.total = off;
  return p;
}

// ... of a rank call: qinfo [Q][4], the targets' values tval [Q] (a distance or a probability) and the counts [Q]
struct SweepRankPlan { size_t qinfo, tval, counts, total; };
inline SweepRankPlan sweep_rank_plan(int64_t Q) {
  SweepRankPlan p{};
  size_t off = 256;
  p.qinfo = off; off += sweep_up((size_t)Q * 4 * sizeof(int32_t));
  p.tval = off; off += sweep_up((size_t)Q * sizeof(float));
  p.counts = off; off += sweep_up((size_t)Q * sizeof(unsigned));
  p.total = off;
  return p;
}

// kernel<<<ceil(n / 256), 256>>>(args...): the launch of sweep_prep.hpp's kernels, one thread per row (bce_finish_k: n = 1, its one
// workgroup).  The kernels are `static`, so each translation unit launches its own copy.  MRG_OK or the HIP error.
template <class... KARGS, class... ARGS>
static inline int sweep_launch_rows(void (*kernel)(KARGS...), int64_t n, hipStream_t st, ARGS... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<KARGS>(args)...);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

}  // namespace mrg
