// mrg_rows_topk: the k best unfiltered entities of every query row under the score x_e = sum_c q[i, c] * ent[e, c], without a [Q, N]
// tensor -- the consumer of the "dot" scorers (DistMult's ent[s] * rel[r], ConvE's hidden vector) that answers (s, r, ?).
// The product runs as the row GEMM of mrg_rows_rank / mrg_distmult_bce_fwd (rows = queries, columns = entities) with the epilogue
// EPI_TOPK: a wave holds 32 rows x RANK_NT * 32 columns in the MFMA accumulator layout, in which the columns of one row sit in the 32
// lanes of a half wave, RANK_NT per lane -- topk_select's layout (topk_parts.hpp), so the tile's k best pairs per row come straight
// out of the accumulators.  The filter bits come from gemm_epilogue_rank's walk of the row's member slice.  Column blocks of BCE_COLS
// outermost (the split table is per block), rows in chunks that keep the partial lists within TOPK_PART_BYTES, one merge per launch.
// Core selection is mrg_rows_rank's -- split-bf16 (rowgemm_x3s_k) for D > 48, D % 4 == 0 and 16-byte aligned rows, else exact f32
// (rowgemm_k) -- and a column's accumulator does not depend on how the columns are cut into blocks, so the values returned are the
// ones mrg_rows_rank compares, bit for bit.
// mrg_rows_bias_topk is the same sweep under a per-entity score bias, x_e = q . ent[e] + bias[e] (CompGCN_ConvE): EPI_TOPK_BIAS adds the
// bias to the accumulators (gemm.hpp: gemm_add_col_bias; a column block that starts at entity c gets bias + c) and selects on them,
// so the values are the ones mrg_rows_bias_rank compares.
#include "gemm_dispatch.hpp"
#include "topk_parts.hpp"

namespace mrg {

// EPI_TOPK: what the selecting epilogue reads and writes.  Like RankEpi the values travel in slots of GemmArgs that this kind does not
// otherwise use (row_seg, Cin, rowscale, seg_part, act, bits_ld, S, aux), so the argument block stays what it was.  row_index stays NULL.
struct TopkEpi {
  const int32_t* qinfo;       // [rows][4]: -1, begin and end of the query's filter list in members / gone_at, `when`
  const int32_t* members;     // filter lists: entity ids, ascending inside a list
  const int32_t* gone_at;     // per member: filtered iff gone_at > when
  TopkEnt* part;              // [rows][gridDim.y][k]: the (row, workgroup) lists
  int k;
  int c0;                     // entity id of the launch's column 0 (B points at that entity's row)
  const float* run_vals;      // [rows][k] the rows' running lists after the column blocks swept so far: their k-th entry prunes
  const int32_t* run_ids;
};
inline void gemm_set_topk(GemmArgs& a, const TopkEpi& t) {
  a.row_seg = t.qinfo; a.Cin = reinterpret_cast<const float*>(t.members); a.rowscale = reinterpret_cast<const float*>(t.gone_at);
  a.seg_part = reinterpret_cast<float*>(t.part); a.act = t.k; a.bits_ld = t.c0;
  a.S = t.run_vals; a.aux = reinterpret_cast<float*>(const_cast<int32_t*>(t.run_ids));
}
__device__ __forceinline__ TopkEpi gemm_topk(const GemmArgs& a) {
  return TopkEpi{a.row_seg, reinterpret_cast<const int32_t*>(a.Cin), reinterpret_cast<const int32_t*>(a.rowscale),
                 reinterpret_cast<TopkEnt*>(a.seg_part), a.act, a.bits_ld, a.S, reinterpret_cast<const int32_t*>(a.aux)};
}

// The filtered columns of a wave's 32 rows x NT * 32 columns as bits: lane l < 32 walks the slice of row (rowbase + l)'s ascending
// member list that falls into the workgroup's column range (binary search for its start, as gemm_epilogue_rank does) and sets the bit
// of every member still in force (gone_at > when); lanes 32-63 and rows beyond the launch leave zeros.
template <int NT>
__device__ __forceinline__ void gemm_topk_filter_words(const TopkEpi& k, int64_t rowbase, int64_t rows, int col0, int lane, unsigned (&word)[NT]) {
#pragma unroll
  for (int n = 0; n < NT; ++n) word[n] = 0u;
  const int64_t row = rowbase + lane;
  if (lane >= 32 || row >= rows) return;
  const int4 qi = *reinterpret_cast<const int4*>(k.qinfo + row * 4);
  const int hi = qi.z, when = qi.w;
  if (qi.y >= hi) return;
  const int cbeg = k.c0 + col0, cend = cbeg + NT * 32;
  int b = qi.y, e = hi;
  while (b < e) {                                            // first member >= cbeg
    const int mid = b + ((e - b) >> 1);
    if (k.members[mid] < cbeg) b = mid + 1; else e = mid;
  }
  for (; b < hi; ++b) {
    const int m = k.members[b];
    if (m >= cend) break;
    if (k.gone_at[b] > when) {
      const int d = m - cbeg;
#pragma unroll
      for (int n = 0; n < NT; ++n) word[n] |= (d >> 5) == n ? 1u << (d & 31) : 0u;
    }
  }
}

// Accumulator register r of a lane is row (r & 3) + 8 * (r >> 2) + 4 * lh of the strip, column n * 32 + li of tile n: per register the
// 32 lanes of a half wave hold one row's NT * 32 columns.  The row's filter word of tile n lives in lane `row within the strip`.
template <int NT>
__device__ __forceinline__ void gemm_epilogue_topk(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh) {
  if (rowbase >= a.rows) return;                             // wave-uniform
  const TopkEpi k = gemm_topk(a);
  unsigned word[NT];
  gemm_topk_filter_words<NT>(k, rowbase, a.rows, col0, lh * 32 + li, word);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rl = (r & 3) + 8 * (r >> 2);
    float v[NT];
    int id[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const unsigned w0 = (unsigned)__builtin_amdgcn_readlane((int)word[n], rl), w1 = (unsigned)__builtin_amdgcn_readlane((int)word[n], rl + 4);
      const int col = col0 + n * 32 + li;
      const bool ok = col < a.N && !(((lh ? w1 : w0) >> li) & 1u);
      v[n] = ok ? acc[n][r] : topk_pad<true>();
      id[n] = ok ? k.c0 + col : TOPK_NONE;
    }
    const int64_t row = rowbase + rl + 4 * lh;
    const int64_t kth = (row < a.rows ? row : a.rows - 1) * k.k + k.k - 1;
    topk_select<true, 32, NT>(v, id, k.run_vals[kth], k.run_ids[kth], k.k, k.part + (row * gridDim.y + blockIdx.y) * k.k, row < a.rows);
  }
}

static_assert(TopkTileCheck<128, RANK_NT * 32>::ok, "");
inline SweepGrid topk_grid(int64_t Q, int64_t N, int64_t chunk) { return SweepGrid{Q, 0, N, 128, RANK_NT * 32, chunk}; }

inline TopkPlan topk_rows_plan(int64_t Q, int64_t N, int D, int k) {
  const bool split = D > 48 && D % 4 == 0;                   // (sized for the split core whatever mrg_gemm_set_mode says)
  const int64_t cc = N < BCE_COLS ? N : BCE_COLS;
  return topk_plan(Q, N, k, 128, RANK_NT * 32, split ? x3_bsplit_bytes((int)cc, D, RANK_NT) : 0);
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_rows_topk_workspace_bytes(int64_t Q, int64_t N, int D, int k) {
  if (!sweep_shape_ok(Q, N, D, true) || !topk_k_ok(k)) return MRG_E_SHAPE;
  return (int64_t)topk_rows_plan(Q, N, D, k).total;
}

// The body of both entry points; bias == NULL: mrg_rows_topk, else mrg_rows_bias_topk.
template <int EPI>
static int topk_rows_run(const float* q, const float* ent, const float* bias, const int64_t* qkey, const int32_t* when, const int64_t* keys,
                         const int32_t* rowptr, const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D,
                         int k, int32_t* ids, float* vals, void* ws, int64_t ws_bytes, void* stream) {
  if (!sweep_labels_ok(U, qkey, when, keys, rowptr, members, gone_at)) return MRG_E_NULLPTR;
  const TopkPlan p = topk_rows_plan(Q, N, D, k);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = sweep_ws_base(ws);
  int32_t* qinfo = (int32_t*)(w + p.qinfo);
  TopkEnt* part = (TopkEnt*)(w + p.part);
  void* ent_split = w + p.ent_split;
  const bool split = rank_split_core(D) && aligned16(q);
  const bool vec = D % 4 == 0 && aligned16(ent) && aligned16(q);

  int rc = sweep_launch_rows(topk_prep_k, Q, st, qkey, when, keys, rowptr, U, Q, k, topk_pad<true>(), qinfo, ids, vals);
  if (rc != MRG_OK) return rc;
  const SweepGrid sg = topk_grid(Q, N, p.chunk);
  return sg.each([&](int64_t q0, int64_t rows, int64_t c, int64_t nc, int64_t) {
    GemmArgs g{};
    g.A1 = q + q0 * D; g.A2 = g.A1; g.K1 = D; g.K2 = 0; g.rows = rows; g.N = (int)nc;
    gemm_set_topk(g, TopkEpi{qinfo + q0 * 4, members, gone_at, part, k, (int)c, vals + q0 * k, ids + q0 * k});
    if (epi_col_bias(EPI)) g.bias = bias + c;
    const dim3 grid(sg.row_tiles(rows), sg.col_tiles(nc));
    const float* ent_c = ent + c * D;
    int rc2;
    // (the split of a column block is redone per row chunk: the launches of one block share the buffer in stream order)
    if (split) {
      launch_bsplit(ent_c, D, 1, g.N, D, RANK_NT, ent_split, st);
      rc2 = launch_kernel(rowgemm_x3s_k<RANK_NT, EPI, false>, grid, dim3(256), (size_t)3 * RANK_NT * 3 * 1024, st, g, (const char*)ent_split,
                          x3_tiles(g.N, RANK_NT));
    } else {
      g.B = ent_c; g.ldb = D;
      if (vec) rc2 = launch_kernel(rowgemm_k<RANK_NT, 1, 16, EPI, true>, grid, dim3(MRG_BLOCK), gemm_lds_bytes(RANK_NT, 1, 16), st, g);
      else rc2 = launch_kernel(rowgemm_k<RANK_NT, 1, 16, EPI, false>, grid, dim3(MRG_BLOCK), gemm_lds_bytes(RANK_NT, 1, 16), st, g);
    }
    if (rc2 != MRG_OK) return rc2;
    return topk_merge_launch<true>(part, (int)grid.y, k, rows, ids + q0 * k, vals + q0 * k, st);
  });
}

extern "C" int mrg_rows_topk(const float* q, const float* ent, const int64_t* qkey, const int32_t* when, const int64_t* keys,
                             const int32_t* rowptr, const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D,
                             int k, int32_t* ids, float* vals, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, true) || !topk_k_ok(k)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!q || !ent || !ids || !vals) return MRG_E_NULLPTR;
  return topk_rows_run<EPI_TOPK>(q, ent, nullptr, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, k, ids, vals, ws, ws_bytes, stream);
}

extern "C" int mrg_rows_bias_topk(const float* q, const float* ent, const float* bias, const int64_t* qkey, const int32_t* when,
                                  const int64_t* keys, const int32_t* rowptr, const int32_t* members, const int32_t* gone_at, int64_t U,
                                  int64_t Q, int64_t N, int D, int k, int32_t* ids, float* vals, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, true) || !topk_k_ok(k)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!q || !ent || !bias || !ids || !vals) return MRG_E_NULLPTR;
  return topk_rows_run<EPI_TOPK_BIAS>(q, ent, bias, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, k, ids, vals, ws, ws_bytes, stream);
}
