// mrg_distmult_rank: raw / filtered ranks of DistMult link prediction without a [Q, N] tensor (reference utils/utils_rgcn.py:212-380,
// search/mr_lp_search.py:258-278).
//   score of candidate e for query i:  x = sum_c ent[a_i, c] * rel[r_i, c] * ent[e, c]
//   ranks[i] = 1 + #{e != t_i, not filtered : x_e > x_t  or  (x_e == x_t and e < t_i)}
// The product [Q, D] x [N, D]^T runs as a row GEMM (rows = queries, columns = entities, grid.y over the column blocks) whose
// epilogue counts instead of storing (gemm.hpp: gemm_epilogue_rank).  Per chunk of RANK_CHUNK queries:
//   1. the operand ent[a] * rel[r] and the gathered target rows ent[t] are materialised (mrg_gather_compose_fwd),
//   2. EPI_RANK_DIAG forms every query's target score on the tile routine of the sweep (row block x against its own 128 gathered
//      targets, diagonal kept): bit-identical with what the sweep computes for a column that holds the same entity row,
//   3. EPI_RANK sweeps all entities and adds, per (row, workgroup), the number of unfiltered candidates that beat the target.
// Split-bf16 core (rowgemm_x3s_k, the entity table pre-split once per call) where it takes the shape, D > 48 and D % 4 == 0;
// every other D runs the same two epilogues on the exact-f32 core (rowgemm_k).
// mrg_rows_rank is the same body for query rows the caller already holds (ConvE's hidden vector, any "dot" scorer): step 1 gathers
// the target rows only.  rank_prep_k / rank_finish_k live in sweep_prep.hpp and the host code around them in
// sweep_host.hpp, shared with the L1 sweeps of transe_1n.hip.
// mrg_rows_bias_rank is mrg_rows_rank under a per-entity score bias, x_e = q . ent[e] + bias[e] (CompGCN_ConvE): the sweep runs as
// EPI_RANK_BIAS (gemm.hpp: the bias joins the accumulators, then EPI_RANK's epilogue), and between steps 2 and 3 rank_bias_tscore_k
// adds bias[t_i] to the target scores -- the float32 add on the same two values that the sweep forms for the target's column, so a
// duplicate entity row with an equal bias still ties bit for bit.
#include "gemm_dispatch.hpp"
#include "sweep_host.hpp"      // the launch bounds, the workspace's rounding and base, the checks; rank_prep_k, rank_finish_k

namespace mrg {

struct RankPlan { size_t ent_split, a, t, t_split, qinfo, tscore, counts, total; };
inline RankPlan rank_plan(int64_t Q, int64_t N, int D) {
  RankPlan p{};
  const int64_t qc = Q < RANK_CHUNK ? Q : RANK_CHUNK;
  const bool split = D > 48 && D % 4 == 0;                  // (sized for the split core whatever mrg_gemm_set_mode says)
  size_t off = 256;                                          // slack: the workspace pointer is rounded up to 256 bytes
  p.ent_split = off; off += sweep_up(split ? x3_bsplit_bytes((int)N, D, RANK_NT) : 0);
  p.a = off; off += sweep_up((size_t)qc * D * sizeof(float));
  p.t = off; off += sweep_up((size_t)qc * D * sizeof(float));
  p.t_split = off; off += sweep_up(split ? x3_bsplit_bytes((int)qc, D, 4) : 0);
  p.qinfo = off; off += sweep_up((size_t)Q * 4 * sizeof(int32_t));
  p.tscore = off; off += sweep_up((size_t)Q * sizeof(float));
  p.counts = off; off += sweep_up((size_t)Q * sizeof(unsigned));
  p.total = off;
  return p;
}

// tscore[i] += bias[target of query i] (qinfo[i][0]): the target's logit under a score bias, after EPI_RANK_DIAG and before the sweep
static __global__ void rank_bias_tscore_k(const float* __restrict__ bias, const int32_t* __restrict__ qinfo, float* __restrict__ tscore, int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) tscore[i] = tscore[i] + bias[qinfo[i * 4]];
}
// g: a chunk's arguments, gemm_set_rank done (qinfo travels in row_seg, tscore_out in aux).  g.bias == NULL: nothing to do
static int rank_bias_tscore(const GemmArgs& g, hipStream_t st) {
  if (!g.bias) return MRG_OK;
  return sweep_launch_rows(rank_bias_tscore_k, g.rows, st, g.bias, g.row_seg, g.aux, g.rows);
}

// one chunk: target scores, then the sweep.  g: A1 / K1 / rows and the rank pointers of the chunk are set; g.bias: [N] or NULL
template <int EPI>
inline int rank_chunk_split(GemmArgs g, const float* T, void* t_split, const void* ent_split, int64_t N, int D, hipStream_t st) {
  GemmArgs d = g;
  d.N = (int)g.rows;
  launch_bsplit(T, D, 1, d.N, D, 4, t_split, st);
  int rc = launch_kernel(rowgemm_x3s_k<4, EPI_RANK_DIAG, false>, dim3((unsigned)((g.rows + 127) / 128), 1), dim3(256), (size_t)3 * 4 * 3 * 1024, st,
                         d, (const char*)t_split, x3_tiles(d.N, 4));
  if (rc != MRG_OK) return rc;
  rc = rank_bias_tscore(g, st);
  if (rc != MRG_OK) return rc;
  g.N = (int)N;
  const int ntile = x3_tiles(g.N, RANK_NT);
  return launch_kernel(rowgemm_x3s_k<RANK_NT, EPI, false>, dim3((unsigned)((g.rows + 127) / 128), (unsigned)(ntile / RANK_NT)), dim3(256),
                       (size_t)3 * RANK_NT * 3 * 1024, st, g, (const char*)ent_split, ntile);
}

template <int EPI, bool VEC4>
inline int rank_chunk_exact(GemmArgs g, const float* T, const float* ent, int64_t N, int D, hipStream_t st) {
  GemmArgs d = g;
  d.N = (int)g.rows; d.B = T; d.ldb = D;
  int rc = launch_kernel(rowgemm_k<4, 1, 16, EPI_RANK_DIAG, VEC4>, dim3((unsigned)((g.rows + 127) / 128), 1), dim3(MRG_BLOCK), gemm_lds_bytes(4, 1, 16), st, d);
  if (rc != MRG_OK) return rc;
  rc = rank_bias_tscore(g, st);
  if (rc != MRG_OK) return rc;
  g.N = (int)N; g.B = ent; g.ldb = D;
  return launch_kernel(rowgemm_k<RANK_NT, 1, 16, EPI, VEC4>, dim3((unsigned)((g.rows + 127) / 128), (unsigned)((N + RANK_NT * 32 - 1) / (RANK_NT * 32))),
                       dim3(MRG_BLOCK), gemm_lds_bytes(RANK_NT, 1, 16), st, g);
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_distmult_rank_workspace_bytes(int64_t Q, int64_t N, int D) {
  if (!sweep_shape_ok(Q, N, D, true)) return MRG_E_SHAPE;
  return (int64_t)rank_plan(Q, N, D).total;
}

// The body of the three entry points.  rows_q == NULL: the chunk's query rows are ent[a] * rel[r] (mrg_distmult_rank); else they are the
// caller's rows_q + q0 * D (mrg_rows_rank; bias != NULL: mrg_rows_bias_rank).  The target rows are gathered in all.
static int rank_run(const float* rows_q, const float* ent, const float* bias, const float* rel, const int32_t* a_idx, const int32_t* r_idx, const int32_t* t_idx,
                    const int64_t* qkey, const int32_t* when, const int64_t* keys, const int32_t* rowptr, const int32_t* members,
                    const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t* ranks, void* ws, int64_t ws_bytes, void* stream) {
  if (!sweep_labels_ok(U, qkey, when, keys, rowptr, members, gone_at)) return MRG_E_NULLPTR;
  const RankPlan p = rank_plan(Q, N, D);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = sweep_ws_base(ws);
  float* A = (float*)(w + p.a);
  float* T = (float*)(w + p.t);
  int32_t* qinfo = (int32_t*)(w + p.qinfo);
  float* tscore = (float*)(w + p.tscore);
  unsigned* counts = (unsigned*)(w + p.counts);
  const bool qal = !rows_q || aligned16(rows_q);                            // the workspace's rows are aligned; a caller's may not be
  const bool split = rank_split_core(D) && qal;
  const bool vec = D % 4 == 0 && aligned16(ent) && qal;

  int rc = sweep_launch_rows(rank_prep_k, Q, st, t_idx, qkey, when, keys, rowptr, U, Q, qinfo, counts);
  if (rc != MRG_OK) return rc;
  if (split) launch_bsplit(ent, D, 1, (int)N, D, RANK_NT, w + p.ent_split, st);
  for (int64_t q0 = 0; q0 < Q; q0 += RANK_CHUNK) {
    const int64_t rows = Q - q0 < RANK_CHUNK ? Q - q0 : RANK_CHUNK;
    const float* Aq = A;
    if (rows_q) Aq = rows_q + q0 * D;
    else rc = mrg_gather_compose_fwd(MRG_COMPOSE_MULT, ent, rel, a_idx + q0, r_idx + q0, A, rows, D, stream);
    if (rc != MRG_OK) return rc;
    rc = mrg_gather_compose_fwd(-1, ent, rel, t_idx + q0, rows_q ? nullptr : r_idx + q0, T, rows, D, stream);
    if (rc != MRG_OK) return rc;
    GemmArgs g{};
    g.A1 = Aq; g.A2 = Aq; g.K1 = D; g.K2 = 0; g.rows = rows; g.bias = bias;      // (the sweep covers all N columns: column 0 is entity 0)
    gemm_set_rank(g, RankEpi{tscore + q0, tscore + q0, qinfo + q0 * 4, members, gone_at, counts + q0});
    if (bias) {
      if (split) rc = rank_chunk_split<EPI_RANK_BIAS>(g, T, w + p.t_split, w + p.ent_split, N, D, st);
      else if (vec) rc = rank_chunk_exact<EPI_RANK_BIAS, true>(g, T, ent, N, D, st);
      else rc = rank_chunk_exact<EPI_RANK_BIAS, false>(g, T, ent, N, D, st);
    }
    else if (split) rc = rank_chunk_split<EPI_RANK>(g, T, w + p.t_split, w + p.ent_split, N, D, st);
    else if (vec) rc = rank_chunk_exact<EPI_RANK, true>(g, T, ent, N, D, st);
    else rc = rank_chunk_exact<EPI_RANK, false>(g, T, ent, N, D, st);
    if (rc != MRG_OK) return rc;
  }
  return sweep_launch_rows(rank_finish_k, Q, st, counts, ranks, Q);
}

extern "C" int mrg_distmult_rank(const float* ent, const float* rel, const int32_t* a_idx, const int32_t* r_idx, const int32_t* t_idx,
                                 const int64_t* qkey, const int32_t* when, const int64_t* keys, const int32_t* rowptr, const int32_t* members,
                                 const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t* ranks, void* ws, int64_t ws_bytes,
                                 void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, true)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!ent || !rel || !a_idx || !r_idx || !t_idx || !ranks) return MRG_E_NULLPTR;
  return rank_run(nullptr, ent, nullptr, rel, a_idx, r_idx, t_idx, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, ranks, ws, ws_bytes, stream);
}

extern "C" int mrg_rows_rank(const float* q, const float* ent, const int32_t* t_idx, const int64_t* qkey, const int32_t* when, const int64_t* keys,
                             const int32_t* rowptr, const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D,
                             int64_t* ranks, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, true)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!q || !ent || !t_idx || !ranks) return MRG_E_NULLPTR;
  return rank_run(q, ent, nullptr, nullptr, nullptr, nullptr, t_idx, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, ranks, ws, ws_bytes, stream);
}

extern "C" int mrg_rows_bias_rank(const float* q, const float* ent, const float* bias, const int32_t* t_idx, const int64_t* qkey,
                                  const int32_t* when, const int64_t* keys, const int32_t* rowptr, const int32_t* members,
                                  const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t* ranks, void* ws, int64_t ws_bytes,
                                  void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, true)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!q || !ent || !bias || !t_idx || !ranks) return MRG_E_NULLPTR;
  return rank_run(q, ent, bias, nullptr, nullptr, nullptr, t_idx, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, ranks, ws, ws_bytes, stream);
}
