// mrg_distmult_bce_fwd / mrg_distmult_bce_dlogit: the fixed-genotype driver's 1-N training loss, BCELoss(sigmoid(q ent^T), labels), without
// a [B, N] tensor (reference train/mr_lp_train.py Network._loss, models/operations_lp.py:115-127, labels utils/data_set.py:21-33).
//   x[b, e] = sum_c q[b, c] * ent[e, c],  q = ent[subj] * rel_emb[rel] materialised by the caller;  p = sigmoid(x)
//   y[b, e] = v_one if e is in the object list of key qkey[b] (LabelIndex: keys / rowptr / objs), else v_zero
//   loss    = mean over b, e of  (y - 1) * max(log1p(-p), -100) - y * max(log p, -100)
//   dl      = gscale * (p - y) * (p (1 - p) / max(p (1 - p), 1e-12))         for the columns [c0, c1)
// The product runs as the row GEMM of mrg_distmult_rank (rows = queries, columns = entities) with the epilogues EPI_BCE / EPI_BCE_GRAD
// (gemm.hpp): the forward leaves one float64 partial per workgroup, which bce_finish_k adds in a fixed order -- no float atomics, the
// same bits on every call -- and the backward recomputes the tile and stores a [B, c1 - c0] slice of the logit gradient.
// Split-bf16 core (rowgemm_x3s_k) for D > 48 with D % 4 == 0, the entity rows pre-split per block of BCE_COLS columns (so the split
// table is O(BCE_COLS * D) whatever N is); every other D on the exact-f32 core (rowgemm_k).  Rows go in chunks of RANK_CHUNK.
// mrg_rows_bias_bce_fwd / mrg_rows_bias_bce_dlogit are the same two sweeps under a per-entity score bias, x[b, e] = q . ent[e] + bias[e]
// (reference models/compgcn.py:188-269, CompGCN_ConvE): EPI_BCE_BIAS / EPI_BCE_GRAD_BIAS add the bias to the accumulators and run the
// same epilogues (gemm.hpp: gemm_add_col_bias); a column block that starts at entity c gets bias + c.  mrg_cols_sum forms the bias
// gradient from a slice of the logit gradient: column sums in float64 in a fixed order.
#include "gemm_dispatch.hpp"
#include "sweep_host.hpp"      // the launch bounds, SweepGrid, the workspace's rounding and base, the checks; bce_prep_k, bce_finish_k

namespace mrg {

inline SweepGrid bce_grid(int64_t B, int64_t c0, int64_t c1) { return SweepGrid{B, c0, c1, 128, RANK_NT * 32}; }

struct BcePlan { size_t ent_split, qlist, partial, total; int64_t nparts; };
// ncols: the columns a call sweeps (N for the forward, c1 - c0 for the logit gradient)
inline BcePlan bce_plan(int64_t B, int64_t ncols, int D) {
  BcePlan p{};
  const bool split = D > 48 && D % 4 == 0;                   // (sized for the split core whatever mrg_gemm_set_mode says)
  const int64_t cc = ncols < BCE_COLS ? ncols : BCE_COLS;
  p.nparts = bce_grid(B, 0, ncols).workgroups();             // one float64 partial per workgroup of the sweep
  size_t off = 256;                                          // slack: the workspace pointer is rounded up to 256 bytes
  p.ent_split = off; off += sweep_up(split ? x3_bsplit_bytes((int)cc, D, RANK_NT) : 0);
  p.qlist = off; off += sweep_up((size_t)B * 2 * sizeof(int32_t));
  p.partial = off; off += sweep_up((size_t)p.nparts * sizeof(double));
  p.total = off;
  return p;
}

// one launch: g.A1 / rows, the columns' count g.N and the epilogue's values are set; ent_c points at the first column's entity row
template <int EPI>
static int bce_launch(GemmArgs g, dim3 grid, const float* ent_c, int D, bool split, bool vec, void* ent_split, hipStream_t st) {
  if (split) {
    launch_bsplit(ent_c, D, 1, g.N, D, RANK_NT, ent_split, st);
    return launch_kernel(rowgemm_x3s_k<RANK_NT, EPI, false>, grid, dim3(256), (size_t)3 * RANK_NT * 3 * 1024, st, g, (const char*)ent_split,
                         x3_tiles(g.N, RANK_NT));
  }
  g.B = ent_c; g.ldb = D;
  if (vec) return launch_kernel(rowgemm_k<RANK_NT, 1, 16, EPI, true>, grid, dim3(MRG_BLOCK), gemm_lds_bytes(RANK_NT, 1, 16), st, g);
  return launch_kernel(rowgemm_k<RANK_NT, 1, 16, EPI, false>, grid, dim3(MRG_BLOCK), gemm_lds_bytes(RANK_NT, 1, 16), st, g);
}

// The sweep over the columns [c0, c1) of all B rows on bce_grid: column blocks outermost (one split per block), row chunks inside.
// EPI_BCE appends its launches' partials at `partial`; EPI_BCE_GRAD stores into dl [B][c1 - c0].  The _BIAS kinds: bias [N], else unused.
template <int EPI>
static int bce_sweep(const float* q, const float* ent, const float* bias, const int32_t* qlist, const int32_t* objs, float v_zero, float v_one, int64_t B, int D,
                     int64_t c0, int64_t c1, double* partial, const float* gscale, float* dl, void* ent_split, hipStream_t st) {
  const bool split = rank_split_core(D) && aligned16(q);
  const bool vec = D % 4 == 0 && aligned16(ent) && aligned16(q);
  const SweepGrid sg = bce_grid(B, c0, c1);
  return sg.each([&](int64_t q0, int64_t rows, int64_t c, int64_t nc, int64_t wg0) {
    GemmArgs g{};
    g.A1 = q + q0 * D; g.A2 = g.A1; g.K1 = D; g.K2 = 0; g.rows = rows; g.N = (int)nc;
    if (epi_unbiased(EPI) == EPI_BCE_GRAD) { g.C = dl + q0 * (c1 - c0) + (c - c0); g.ldc = (int)(c1 - c0); }
    if (epi_col_bias(EPI)) g.bias = bias + c;
    gemm_set_bce(g, BceEpi{qlist + q0 * 2, objs, v_zero, v_one, (int)c, epi_unbiased(EPI) == EPI_BCE ? partial + wg0 : partial, gscale});
    // (the split of a column block is redone per row chunk only when B > RANK_CHUNK: the launches of one block share the buffer in stream order)
    return bce_launch<EPI>(g, dim3(sg.row_tiles(rows), sg.col_tiles(nc)), ent + c * D, D, split, vec, ent_split, st);
  });
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_distmult_bce_workspace_bytes(int64_t B, int64_t N, int D) {
  if (!sweep_shape_ok(B, N, D, true)) return MRG_E_SHAPE;
  return (int64_t)bce_plan(B, N, D).total;
}

// The body of the four entry points from the label pointers on.  dl == NULL: the loss over the columns [0, N) = [c0, c1)
// (mrg_distmult_bce_fwd); else the logit gradient of the columns [c0, c1) (mrg_distmult_bce_dlogit).  bias != NULL: their biased twins.
static int bce_run(const float* q, const float* ent, const float* bias, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr, const int32_t* objs,
                   int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D, int64_t c0, int64_t c1, float* loss,
                   const float* gscale, float* dl, void* ws, int64_t ws_bytes, void* stream) {
  if (!sweep_labels_ok(U, qkey, keys, rowptr, objs)) return MRG_E_NULLPTR;
  const BcePlan p = bce_plan(B, c1 - c0, D);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = sweep_ws_base(ws);
  int32_t* qlist = (int32_t*)(w + p.qlist);
  double* partial = (double*)(w + p.partial);
  int rc = sweep_launch_rows(bce_prep_k, B, st, qkey, keys, rowptr, U, B, qlist);
  if (rc != MRG_OK) return rc;
  if (dl && bias) return bce_sweep<EPI_BCE_GRAD_BIAS>(q, ent, bias, qlist, objs, v_zero, v_one, B, D, c0, c1, nullptr, gscale, dl, w + p.ent_split, st);
  if (dl) return bce_sweep<EPI_BCE_GRAD>(q, ent, nullptr, qlist, objs, v_zero, v_one, B, D, c0, c1, nullptr, gscale, dl, w + p.ent_split, st);
  if (bias) rc = bce_sweep<EPI_BCE_BIAS>(q, ent, bias, qlist, objs, v_zero, v_one, B, D, c0, c1, partial, nullptr, nullptr, w + p.ent_split, st);
  else rc = bce_sweep<EPI_BCE>(q, ent, nullptr, qlist, objs, v_zero, v_one, B, D, c0, c1, partial, nullptr, nullptr, w + p.ent_split, st);
  if (rc != MRG_OK) return rc;
  return sweep_launch_rows(bce_finish_k, 1, st, partial, p.nparts, 1.0 / ((double)B * (double)N), loss);
}

extern "C" int mrg_distmult_bce_fwd(const float* q, const float* ent, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr,
                                    const int32_t* objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D, float* loss,
                                    void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, true)) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!q || !ent || !loss) return MRG_E_NULLPTR;
  return bce_run(q, ent, nullptr, qkey, keys, rowptr, objs, U, v_zero, v_one, B, N, D, 0, N, loss, nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int mrg_distmult_bce_dlogit(const float* q, const float* ent, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr,
                                       const int32_t* objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D, int64_t c0,
                                       int64_t c1, const float* gscale, float* dl, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, true) || c0 < 0 || c1 <= c0 || c1 > N) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!q || !ent || !gscale || !dl) return MRG_E_NULLPTR;
  return bce_run(q, ent, nullptr, qkey, keys, rowptr, objs, U, v_zero, v_one, B, N, D, c0, c1, nullptr, gscale, dl, ws, ws_bytes, stream);
}

extern "C" int mrg_rows_bias_bce_fwd(const float* q, const float* ent, const float* bias, const int64_t* qkey, const int64_t* keys,
                                     const int32_t* rowptr, const int32_t* objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N,
                                     int D, float* loss, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, true)) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!q || !ent || !bias || !loss) return MRG_E_NULLPTR;
  return bce_run(q, ent, bias, qkey, keys, rowptr, objs, U, v_zero, v_one, B, N, D, 0, N, loss, nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int mrg_rows_bias_bce_dlogit(const float* q, const float* ent, const float* bias, const int64_t* qkey, const int64_t* keys,
                                        const int32_t* rowptr, const int32_t* objs, int64_t U, float v_zero, float v_one, int64_t B,
                                        int64_t N, int D, int64_t c0, int64_t c1, const float* gscale, float* dl, void* ws,
                                        int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, true) || c0 < 0 || c1 <= c0 || c1 > N) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!q || !ent || !bias || !gscale || !dl) return MRG_E_NULLPTR;
  return bce_run(q, ent, bias, qkey, keys, rowptr, objs, U, v_zero, v_one, B, N, D, c0, c1, nullptr, gscale, dl, ws, ws_bytes, stream);
}

// out[c] = sum over r of x[r][c], float64 accumulation in a fixed order: a workgroup of COLS_SUM_WAVES waves owns 64 columns, lane l of
// every wave column l (coalesced rows); wave w adds the rows w, w + COLS_SUM_WAVES, ... in ascending order, the waves' sums meet in LDS
// and are added in wave order.  No atomics: the same bits on every call.
constexpr int COLS_SUM_WAVES = 8;
static __global__ __launch_bounds__(64 * COLS_SUM_WAVES) void cols_sum_k(const float* __restrict__ x, int64_t rows, int64_t cols, int64_t ld,
                                                                         float* __restrict__ out) {
  __shared__ double part[COLS_SUM_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + lane;
  double s = 0.0;
  if (col < cols)
    for (int64_t r = wave; r < rows; r += COLS_SUM_WAVES) s += (double)x[r * ld + col];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && col < cols) {
    double t = part[0][lane];
#pragma unroll
    for (int w = 1; w < COLS_SUM_WAVES; ++w) t += part[w][lane];
    out[col] = (float)t;
  }
}

extern "C" int mrg_cols_sum(const float* x, int64_t rows, int64_t cols, int64_t ld, float* out, void* stream) {
  if (rows < 0 || cols < 0 || ld < cols || (cols + 63) / 64 > 0x7fffffffLL) return MRG_E_SHAPE;
  if (cols == 0) return MRG_OK;
  if (!out || (rows > 0 && !x)) return MRG_E_NULLPTR;
  hipLaunchKernelGGL(cols_sum_k, dim3((unsigned)((cols + 63) / 64)), dim3(64 * COLS_SUM_WAVES), 0, (hipStream_t)stream, x, rows, cols, ld, out);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}
