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
#include "gemm_dispatch.hpp"
#include "sweep_prep.hpp"      // bce_prep_k, bce_finish_k

namespace mrg {

struct BcePlan { size_t ent_split, qlist, partial, total; int64_t nrb, ncb; };
inline size_t bce_up(size_t x) { return (x + 255) & ~(size_t)255; }
// ncols: the columns a call sweeps (N for the forward, c1 - c0 for the logit gradient)
inline BcePlan bce_plan(int64_t B, int64_t ncols, int D) {
  BcePlan p{};
  const bool split = D > 48 && D % 4 == 0;                   // (sized for the split core whatever mrg_gemm_set_mode says)
  const int64_t cc = ncols < BCE_COLS ? ncols : BCE_COLS;
  p.nrb = (B / RANK_CHUNK) * (RANK_CHUNK / 128) + (B % RANK_CHUNK + 127) / 128;                        // workgroups along the rows ...
  p.ncb = (ncols / BCE_COLS) * (BCE_COLS / (RANK_NT * 32)) + (ncols % BCE_COLS + RANK_NT * 32 - 1) / (RANK_NT * 32);   // ... and the columns
  size_t off = 256;                                          // slack: the workspace pointer is rounded up to 256 bytes
  p.ent_split = off; off += bce_up(split ? x3_bsplit_bytes((int)cc, D, RANK_NT) : 0);
  p.qlist = off; off += bce_up((size_t)B * 2 * sizeof(int32_t));
  p.partial = off; off += bce_up((size_t)p.nrb * p.ncb * sizeof(double));
  p.total = off;
  return p;
}

// one launch: g.A1 / rows, the columns' count g.N and the epilogue's values are set; ent_c points at the first column's entity row
template <int EPI>
inline int bce_launch(GemmArgs g, const float* ent_c, int D, bool split, bool vec, void* ent_split, hipStream_t st) {
  const dim3 grid((unsigned)((g.rows + 127) / 128), (unsigned)((g.N + RANK_NT * 32 - 1) / (RANK_NT * 32)));
  if (split) {
    launch_bsplit(ent_c, D, 1, g.N, D, RANK_NT, ent_split, st);
    return launch_kernel(rowgemm_x3s_k<RANK_NT, EPI, false>, grid, dim3(256), (size_t)3 * RANK_NT * 3 * 1024, st, g, (const char*)ent_split,
                         x3_tiles(g.N, RANK_NT));
  }
  g.B = ent_c; g.ldb = D;
  if (vec) return launch_kernel(rowgemm_k<RANK_NT, 1, 16, EPI, true>, grid, dim3(MRG_BLOCK), gemm_lds_bytes(RANK_NT, 1, 16), st, g);
  return launch_kernel(rowgemm_k<RANK_NT, 1, 16, EPI, false>, grid, dim3(MRG_BLOCK), gemm_lds_bytes(RANK_NT, 1, 16), st, g);
}

// The sweep over the columns [c0, c1) of all B rows: column blocks outermost (one split per block), row chunks inside.  EPI_BCE appends
// its launches' partials at `partial`; EPI_BCE_GRAD stores into dl [B][c1 - c0].
template <int EPI>
inline int bce_sweep(const float* q, const float* ent, const int32_t* qlist, const int32_t* objs, float v_zero, float v_one, int64_t B, int D,
                     int64_t c0, int64_t c1, double* partial, const float* gscale, float* dl, void* ent_split, hipStream_t st) {
  const bool split = rank_split_core(D) && aligned16(q);
  const bool vec = D % 4 == 0 && aligned16(ent) && aligned16(q);
  for (int64_t c = c0; c < c1; c += BCE_COLS) {
    const int64_t nc = c1 - c < BCE_COLS ? c1 - c : BCE_COLS;
    for (int64_t q0 = 0; q0 < B; q0 += RANK_CHUNK) {
      const int64_t rows = B - q0 < RANK_CHUNK ? B - q0 : RANK_CHUNK;
      GemmArgs g{};
      g.A1 = q + q0 * D; g.A2 = g.A1; g.K1 = D; g.K2 = 0; g.rows = rows; g.N = (int)nc;
      if (EPI == EPI_BCE_GRAD) { g.C = dl + q0 * (c1 - c0) + (c - c0); g.ldc = (int)(c1 - c0); }
      gemm_set_bce(g, BceEpi{qlist + q0 * 2, objs, v_zero, v_one, (int)c, partial, gscale});
      // (the split of a column block is redone per row chunk only when B > RANK_CHUNK: the launches of one block share the buffer in stream order)
      const int rc = bce_launch<EPI>(g, ent + c * D, D, split, vec, ent_split, st);
      if (rc != MRG_OK) return rc;
      if (EPI == EPI_BCE) partial += ((rows + 127) / 128) * ((nc + RANK_NT * 32 - 1) / (RANK_NT * 32));
    }
  }
  return MRG_OK;
}

}  // namespace mrg

using namespace mrg;

static bool bce_shape_ok(int64_t B, int64_t N, int D) { return B >= 0 && N >= 1 && N <= RANK_MAX_N && D >= 1 && D <= 1024 && (D <= 256 || D % 4 == 0); }

extern "C" int64_t mrg_distmult_bce_workspace_bytes(int64_t B, int64_t N, int D) {
  if (!bce_shape_ok(B, N, D)) return MRG_E_SHAPE;
  return (int64_t)bce_plan(B, N, D).total;
}

extern "C" int mrg_distmult_bce_fwd(const float* q, const float* ent, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr,
                                    const int32_t* objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D, float* loss,
                                    void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !bce_shape_ok(B, N, D)) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!q || !ent || !loss) return MRG_E_NULLPTR;
  if (U > 0 && (!qkey || !keys || !rowptr || !objs)) return MRG_E_NULLPTR;
  const BcePlan p = bce_plan(B, N, D);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255) - 256;        // the plan's offsets start at 256
  int32_t* qlist = (int32_t*)(w + p.qlist);
  double* partial = (double*)(w + p.partial);
  hipLaunchKernelGGL(bce_prep_k, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, qkey, keys, rowptr, U, B, qlist);
  MRG_LAUNCH_CHECK();
  const int rc = bce_sweep<EPI_BCE>(q, ent, qlist, objs, v_zero, v_one, B, D, 0, N, partial, nullptr, nullptr, w + p.ent_split, st);
  if (rc != MRG_OK) return rc;
  hipLaunchKernelGGL(bce_finish_k, dim3(1), dim3(256), 0, st, partial, p.nrb * p.ncb, 1.0 / ((double)B * (double)N), loss);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_distmult_bce_dlogit(const float* q, const float* ent, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr,
                                       const int32_t* objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D, int64_t c0,
                                       int64_t c1, const float* gscale, float* dl, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !bce_shape_ok(B, N, D) || c0 < 0 || c1 <= c0 || c1 > N) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!q || !ent || !gscale || !dl) return MRG_E_NULLPTR;
  if (U > 0 && (!qkey || !keys || !rowptr || !objs)) return MRG_E_NULLPTR;
  const BcePlan p = bce_plan(B, c1 - c0, D);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255) - 256;
  int32_t* qlist = (int32_t*)(w + p.qlist);
  hipLaunchKernelGGL(bce_prep_k, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, qkey, keys, rowptr, U, B, qlist);
  MRG_LAUNCH_CHECK();
  return bce_sweep<EPI_BCE_GRAD>(q, ent, qlist, objs, v_zero, v_one, B, D, c0, c1, nullptr, gscale, dl, w + p.ent_split, st);
}
