// The launch plan of the exact-f32 weight-gradient kernels (wgrad.hip: wgrad_k, wgrad_dma_k) and the list of their instances.
// Plain C++17 without HIP, so that a host program can walk the plan over every shape and check that it lands on an instance
// that exists and that every instance is reached (tools/wgrad_plan_check.cpp, tests/test_wgrad_plan_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mrg {

constexpr int WBR = 16;              // rows per LDS tile
constexpr int WGRAD_BLOCK = 256;     // threads of wgrad_k / wgrad_dma_k (MRG_BLOCK; wgrad.hip asserts the two agree)

struct WgradPlan {
  int TM, TN, TNB, tpw, npf, G;
  int64_t rows_per_block;
  size_t lds;
  bool ok;
};

// How many row ranges share one weight-gradient launch (the three direction segments of a dense filter: mrg_linear_bwd_weight3), so
// that the ranges TOGETHER, not each of them, get about one workgroup per CU: with 15 000-row ranges (the 30 000-edge search step) three
// ranges of 59 row blocks x 2 column blocks were 354 workgroups = 1.4 rounds of the chip, 46 us where one round of 23-tile blocks
// takes 33.  A caller that launches the ranges one by one passes their number as mrg_linear_bwd_weight_share's `share`, to keep the
// same partial sums.
constexpr int WGRAD_SHARE_MAX_BLOCKS = 400;   // largest range (row blocks of 16 tiles) that shares the chip; see wgrad_plan

inline WgradPlan wgrad_plan(int64_t rows, int K, int Nout, bool dma = false, int share = 1) {
  WgradPlan p{};
  p.TM = (Nout + 31) / 32;
  p.TN = (K + 1 + 31) / 32;
  const int opts[] = {1, 2, 4, 7};                       // p.tpw stays 0 where none fits
  if (dma && p.TM <= 7) {
    // DMA kernel: wave w owns column tile w of the block (<= 4 per block) and all TM row tiles
    p.TNB = p.TN < 4 ? p.TN : 4;
    for (int o : opts) if (p.TM <= o) { p.tpw = o; break; }
  } else {
    // at most 28 accumulator tiles (7 per wave, 112 registers) per workgroup so that two workgroups
    // share a CU; wider outputs split the X' column tiles over grid.y (gY is then re-read per split)
    p.TNB = p.TM * p.TN <= 28 ? p.TN : (28 / p.TM > 0 ? 28 / p.TM : 0);
    int per_wave = p.TNB > 0 ? (p.TM * p.TNB + 3) / 4 : 99;      // 99 (more than 28 row tiles): no option matches, the plan is not ok
    for (int o : opts) if (per_wave <= o) { p.tpw = o; break; }
  }
  int nf4 = WBR * (p.TM + p.TNB) * 8;                    // float4 per staged tile
  p.npf = (nf4 + WGRAD_BLOCK - 1) / WGRAD_BLOCK;
  p.lds = (size_t)(dma ? 3 : 2) * WBR * (p.TM + p.TNB) * 32 * sizeof(float);
  p.ok = p.tpw > 0 && p.lds <= 160 * 1024 && p.npf <= 16;
  int64_t tiles = (rows + WBR - 1) / WBR;
  // >= 16 row tiles per workgroup: every extra workgroup costs a TM*32 x TN*32 partial tile (372 KB at 200 x 400)
  // that the ordered reduction has to read back
  // ... and about one workgroup per CU: 256 / (column blocks of the split-core kernel) row blocks (the figure depends on
  // the shape only, never on the kernel chosen: the workspace query and the launch must agree)
  const int ny = (p.TN + (p.TM <= 4 ? 16 : 8) - 1) / (p.TM <= 4 ? 16 : 8);
  // (only up to 400 row blocks of 16 tiles per range: measured -13 % at 15 000-row ranges,
  //  -10 % at 87 000-row ranges, but +20 % at 272 000-row ranges, where three rounds of 128 shorter workgroups per range beat one round of long ones)
  const bool shared = share > 1 && (tiles + 15) / 16 <= WGRAD_SHARE_MAX_BLOCKS;
  const int64_t gshare = 256 / (ny * share);
  const int64_t gmax = !shared ? (256 / ny > 32 ? 256 / ny : 32) : (gshare > 16 ? gshare : 16);
  int64_t G = (tiles + 15) / 16 < gmax ? (tiles + 15) / 16 : gmax;
  // few rows (a sampled step graph, a rank's node chunk): a workgroup walks its 16-row tiles one barrier at a time (~2 us each), so
  // one or two workgroups of 16 tiles are a 30 us latency chain on an idle chip -- up to eight workgroups of >= 4 tiles instead
  // (the extra partial tiles are a few MB for the ordered reduction)
  const int64_t gsmall = (tiles + 3) / 4 < 8 ? (tiles + 3) / 4 : 8;
  if (G < gsmall) G = gsmall;
  if (G < 1) G = 1;
  int64_t tpb = (tiles + G - 1) / G;
  if (tpb < 1) tpb = 1;
  p.rows_per_block = tpb * WBR;
  p.G = (int)((rows + p.rows_per_block - 1) / p.rows_per_block);
  if (p.G < 1) p.G = 1;
  return p;
}

// The prefetch depth a kernel is instantiated for: the plan's float4 per thread rounded up to 2, 4, 8 or 16.
inline int wgrad_npf_class(int npf) { return npf <= 2 ? 2 : (npf <= 4 ? 4 : (npf <= 8 ? 8 : 16)); }

// Every (tpw, npf class) an ok plan can produce, per kernel, and nothing else: wgrad.hip instantiates and dispatches exactly
// these.  (A wave owns at most 7 tiles: 28 per workgroup in the plain form, TM <= 7 in the DMA form.)
#define MRG_WGRAD_DMA_INSTANCES(X) X(1, 2) X(1, 4) X(2, 2) X(2, 4) X(4, 2) X(4, 4) X(7, 4) X(7, 8)
#define MRG_WGRAD_PLAIN_INSTANCES(X) X(1, 2) X(1, 4) X(2, 4) X(2, 8) X(4, 4) X(4, 8) X(4, 16) X(7, 8) X(7, 16)

inline bool wgrad_has_instance(bool dma, int tpw, int npf_class) {
#define MRG_WGRAD_IS(T, F) if (tpw == T && npf_class == F) return true;
  if (dma) { MRG_WGRAD_DMA_INSTANCES(MRG_WGRAD_IS) } else { MRG_WGRAD_PLAIN_INSTANCES(MRG_WGRAD_IS) }
#undef MRG_WGRAD_IS
  return false;
}

}  // namespace mrg
