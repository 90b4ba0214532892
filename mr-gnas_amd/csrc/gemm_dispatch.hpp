// Which kernel a row GEMM launch takes.  Two matrix cores:
//   gemm.hpp        exact f32 (v_mfma_f32_32x32x2_f32): rowgemm_dma_k / rowgemm_k.  Mode 1, operands the split core cannot take, no workspace.
//   split bf16      (arithmetic, weight split and every shared part: x3_parts.hpp), four kernels that agree bit for bit unless noted:
//     gemm_x3s.hpp   rowgemm_x3s_k   the default: weight slabs shared through LDS, 128-row workgroups, two per CU; grouped launches,
//                                    dual source, the fused aggregators' epilogues; outputs up to 7 column tiles per block
//     gemm_x3s8.hpp  rowgemm_x3s8_k  plain single-source launches of 225..256 columns (D = 256) as ONE block of eight tiles
//     gemm_x3q.hpp   rowgemm_x3q_k   16 x 16 x 32 tiles, 64-row workgroups, three per CU: 129..224 columns with K > X3Q_MIN_K
//                                    (sums 32 k at a time: agrees with the others to rounding, not bit for bit)
//     gemm_x3.hpp    rowgemm_x3_k    wave-autonomous, one wave per SIMD: few rows (<= X3N_MAX_ROWS, two-tile column blocks) and mode 2
// mrg_distmult_rank (rank.hip) launches rowgemm_x3s_k / rowgemm_k itself with the counting epilogues EPI_RANK / EPI_RANK_DIAG (gemm.hpp).
// The persistent transposed-accumulator kernel and the two-waves-per-SIMD kernel of rounds 2-3 live in tools/lab/ (tools/gemm_x3_lab.hip
// still times them).  The switches that move a launch off its default kernel are GemmSwitches (x3_parts.hpp).
#pragma once
#include "gemm_x3.hpp"
#include "gemm_x3s.hpp"
#include "gemm_x3s8.hpp"
#include "gemm_x3q.hpp"

namespace mrg {

// Since round 3 the default split-core kernel is gemm_x3s.hpp: bit-identical with gemm_x3.hpp; alone 0.191 vs 0.22-0.23 ms at rows
// 272 115, K = N = 200 and equal at 558 771 rows, but inside the supernet step every row-GEMM entry point gains 9-22 % (input
// gradients 10.3 -> 8.4 ms, fused a_max / a_mean 4.1 -> 3.2, dense-filter forward 6.5 -> 5.9; 68.2 -> 65.5 ms / step,
// profiles/r3_rowgemm_lds_weight.txt).
inline int gemm_mode() { return gemm_switches().mode; }

// Which launches take the 16 x 16 x 32 kernel of gemm_x3q.hpp (round 5): a pure function of the epilogue kind and of the product's
// shape, so that the code that prepares the weight split and the code that launches the GEMM agree without talking.  Its column
// block is 14 tiles of 16 (129..224 columns: narrower products keep the four-tile blocks of rowgemm_x3s_k, wider ones its eight-tile
// sibling); the fused aggregators' epilogues (EPI_SEGMAX / EPI_SEGSUM: run structure tied to the 32-row strip) stay on rowgemm_x3s_k.
// Measured (profiles/r5_rowgemm_q.txt, rows 558 771, interleaved rounds in one process): at K = 400 (the dense filters' forward on
// two operands, the paired input gradient) 0.552 vs 0.584 ms (-5 %), gate-only forward -7..-12 %; at K = 200 equal (0.986-1.017): the
// reduction dimension has to be long enough for the smaller tile's doubled weight traffic (L2 -> LDS 2.6 GB instead of 1.2 GB per
// launch) to be paid back, so switch q == 1 (default) takes only K > X3Q_MIN_K; 2 (lab, tests) takes every K > 48.
constexpr int X3Q_MIN_K = 224;
inline bool x3q_shape(int epi, int N, int K) {
  const int q = gemm_switches().q;
  return gemm_mode() == 0 && q != 0 && epi != EPI_SEGMAX && epi != EPI_SEGSUM && N > 128 && N <= X3Q_NT * 16 && K > (q == 2 ? 48 : X3Q_MIN_K);
}

// FEW ROWS (round 5: the sampled search step of graph_batch_size 300, a rank's node chunk).  A 128-row workgroup of rowgemm_x3s_k
// walks all seven column tiles of its rows: 546 matrix instructions per wave one behind the other, ~20 us however few rows there
// are, on an otherwise idle chip.  Up to X3N_MAX_ROWS rows the product runs on the wave-autonomous kernel of gemm_x3.hpp with column
// blocks of TWO tiles (grid.y = 4 for 200 columns): 3.5 x more waves, each with a 3.5 x shorter chain.  Same operands, same order of
// the k-sum per output element: bit-identical with rowgemm_x3s_k (tests/test_ops_gpu.py::test_few_rows_row_gemm_is_bit_exact), so a
// grouped launch and its per-range launches may fall on different sides of the bound.  Not for the shapes of rowgemm_x3q_k (another
// summation order: those keep one kernel for every row count).  mrg_gemm_set_small(0) switches it off.
constexpr int X3N_NT = 2;                   // (the default row bound X3N_MAX_ROWS is next to the switch: x3_parts.hpp)
inline bool x3n_shape(int epi, int64_t rows, int N, int K) {
  return gemm_mode() == 0 && rows > 0 && rows <= gemm_switches().small_rows && gemm_pick_nt(N) > X3N_NT && N <= 224 && !x3q_shape(epi, N, K);
}

// bytes of ONE pre-split weight in whichever layout a launch of this shape may use
inline size_t bsplit_bytes_any(int N, int K) {
  const size_t a = x3_bsplit_bytes(N, K, gemm_pick_nt(N));
  const size_t q = (N > 128 && N <= X3Q_NT * 16) ? x3q_bsplit_bytes(K) : 0;
  const size_t n = (gemm_pick_nt(N) > X3N_NT && N <= 224) ? x3_bsplit_bytes(N, K, X3N_NT) : 0;
  const size_t m = a > q ? a : q;
  return m > n ? m : n;
}

// the weight split of a launch of `rows` rows with epilogue `epi`: B(n, k) = B[n * sn + k * sk]
inline void launch_bsplit_any(int epi, int64_t rows, const float* B, int64_t sn, int64_t sk, int N, int K, void* Bp, hipStream_t st) {
  if (x3q_shape(epi, N, K)) {
    const float* Bs[1] = {B};
    void* outs[1] = {Bp};
    launch_bsplitq3(Bs, sn, sk, N, K, outs, 1, st);
  } else {
    launch_bsplit(B, sn, sk, N, K, x3n_shape(epi, rows, N, K) ? X3N_NT : gemm_pick_nt(N), Bp, st);
  }
}
inline void launch_bsplit3_any(int epi, int64_t rows, const float* const* B, int64_t sn, int64_t sk, int N, int K, void* const* out, hipStream_t st,
                               const float* const* B2 = nullptr, int ksplit = 0) {
  if (x3q_shape(epi, N, K)) launch_bsplitq3(B, sn, sk, N, K, out, 3, st, B2, ksplit);
  else launch_bsplit3(B, sn, sk, N, K, x3n_shape(epi, rows, N, K) ? X3N_NT : gemm_pick_nt(N), out, st, B2, ksplit);
}

// the split-core row GEMM of the current mode for launches that prepared their own weight split (grouped launches, fused aggregators)
// with launch_bsplit_any / launch_bsplit3_any
template <int EPI>
inline int launch_rowgemm_x3_mode(GemmArgs a, const void* Bp, hipStream_t st) {
  if (x3q_shape(EPI, a.N, a.K1 + a.K2)) {
    if (!x3q_eligible(a)) return MRG_E_SHAPE;              // the split was prepared in this kernel's layout: no other kernel can read it
    return launch_rowgemm_x3q<EPI>(a, Bp, st);
  }
  if (x3n_shape(EPI, a.rows, a.N, a.K1 + a.K2)) {
    if (!x3_eligible(a)) return MRG_E_SHAPE;               // the split was prepared with two-tile column blocks
    return launch_rowgemm_x3<EPI>(a, Bp, st, X3N_NT);
  }
  if (gemm_mode() != 2 && x3s_eligible(a)) {
    // eight column tiles (D = 256) as ONE block where the epilogue fits (gemm_x3s8.hpp): the activation operand is read once
    if constexpr (EPI != EPI_GATE) {
      if (x3s8_eligible<EPI>(a)) return launch_rowgemm_x3s8<EPI>(a, Bp, st);
    }
    return launch_rowgemm_x3s<EPI>(a, Bp, st);
  }
  return launch_rowgemm_x3<EPI>(a, Bp, st);
}

// ---- column sums of the output as a by-product (EPI_GATE / EPI_SCALE: the MixedOp epilogue's BatchNorm statistics) ---------------
// The workgroups (= [2][N] float64 partials) a launch of `a` would leave, or 0 when the kernel it would take has no such form: the
// exact-f32 core and mode 2, few-row launches on rowgemm_x3_k, and outputs that are not
// one seven-tile column block (129..224 columns, N % 4 == 0).  The caller then keeps the statistics pass.
inline int64_t gemm_colsum_blocks(int epi, GemmArgs a) {
  const int K = a.K1 + a.K2;
  if ((epi != EPI_GATE && epi != EPI_SCALE) || gemm_mode() != 0) return 0;
  if (a.N % 4 != 0 || a.N <= 128 || a.N > 224 || a.rows <= 0 || !x3_eligible(a)) return 0;
  int gbm = 128;
  if (x3q_shape(epi, a.N, K)) {
    if (!x3q_eligible(a)) return 0;
    gbm = X3Q_ROWS;
  } else if (x3n_shape(epi, a.rows, a.N, K)) {
    return 0;
  }
  return a.grp.n > 0 ? gemm_group_tiles(a.grp, gbm) : (a.rows + gbm - 1) / gbm;
}

// the launch itself (the weight split prepared by launch_bsplit_any / launch_bsplit3_any for the plain epilogue, as for
// launch_rowgemm_x3_mode); EPI = EPI_GATE_SUMS / EPI_SCALE_SUMS, gemm_set_colsum(a, .): gemm_colsum_blocks(epi_base(EPI), a) partials
template <int EPI>
inline int launch_rowgemm_x3_mode_colsum(GemmArgs a, const void* Bp, hipStream_t st) {
  if (!gemm_colsum(a) || gemm_colsum_blocks(epi_base(EPI), a) <= 0) return MRG_E_SHAPE;
  if (x3q_shape(epi_base(EPI), a.N, a.K1 + a.K2)) return launch_rowgemm_x3q<EPI>(a, Bp, st);
  return launch_rowgemm_x3s_colsum<EPI>(a, Bp, st);
}

// ---- queries x all entities (rank.hip, bce.hip): the sweeps that launch rowgemm_x3s_k / rowgemm_k themselves -------------------------
// (RANK_CHUNK, RANK_NT, RANK_MAX_N, BCE_COLS: sweep_host.hpp, shared with the L1 sweeps of transe_1n.hip)
inline bool rank_split_core(int D) { return gemm_mode() != 1 && D > 48 && D % 4 == 0; }

inline size_t gemm_workspace_bytes(int K, int N) {
  const size_t split = bsplit_bytes_any(N, K);
  const size_t transp = (size_t)K * N * sizeof(float);
  return split > transp ? split : transp;
}

// B(n, k) = a.B[n * b_sn + k * b_sk] (a.ldb is ignored).  ws: gemm_workspace_bytes(K, N) bytes, may be NULL
// when b_sk == 1 (then only the exact-f32 core is available).
template <int EPI>
inline int launch_gemm(GemmArgs a, int64_t b_sn, int64_t b_sk, void* ws, hipStream_t st) {
  if (a.rows <= 0) return MRG_OK;
  if (!a.A2 || a.K2 == 0) { a.A2 = a.A1; a.K2 = 0; }
  const int K = a.K1 + a.K2;
  if (ws && gemm_mode() != 1 && x3_eligible(a)) {
    launch_bsplit_any(EPI, a.rows, a.B, b_sn, b_sk, a.N, K, ws, st);
    return launch_rowgemm_x3_mode<EPI>(a, ws, st);
  }
  if (b_sk != 1) {                                   // present B^T row-major to the f32 core
    if (!ws) return MRG_E_WORKSPACE;
    launch_transpose(a.B, (float*)ws, (int)(K), a.N, (int)b_sk, st);
    a.B = (const float*)ws;
    a.ldb = K;
  } else {
    a.ldb = (int)b_sn;
  }
  return launch_rowgemm<EPI>(a, st);
}

}  // namespace mrg
