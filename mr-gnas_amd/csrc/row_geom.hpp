// Row-tile geometry of the row-streaming kernels (compose, gate, dense, accum, segreduce, segstd, mixedop, cell_zero, fused_gcs):
// which template instance <VEC, LPR, KMAX> a row width D and the alignment of its pointers select.  Host code only (no HIP
// include): tools/row_geom_check.cpp walks it on the CPU.
#pragma once
#include <stdint.h>

namespace mrg {

// ---- row-tile geometry ---------------------------------------------------------
// A row of D floats is covered by LPR lanes x KMAX steps x VEC floats.
struct RowGeom {
  int vec;    // 4 (D % 4 == 0 and 16-B aligned pointers) or 1
  int lpr;    // lanes per row: 16 / 32 / 64
  int kmax;   // 1 / 2 / 4
  bool ok;
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline RowGeom row_geom(int D, bool all_aligned) {
  RowGeom g{};
  g.vec = (D % 4 == 0 && all_aligned) ? 4 : 1;
  int dv = D / g.vec;
  g.lpr = dv <= 16 ? 16 : (dv <= 32 ? 32 : 64);
  int k = (dv + g.lpr - 1) / g.lpr;
  g.kmax = k <= 1 ? 1 : (k <= 2 ? 2 : 4);
  g.ok = D > 0 && k <= 4;
  return g;
}

}  // namespace mrg
