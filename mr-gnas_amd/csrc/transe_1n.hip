// The 1-N TransE loss, its logit gradient and the filtered ranks without a [B, N] tensor (reference models/operations_lp.py:101-112
// sf_TransE_op, train/mr_lp_train.py Network._loss and predict; labels utils/data_set.py:21-33).
//   dist[b, e] = sum_c |obj[b, c] - ent[e, c]|     obj = sub + rel, float32, formed by the caller
//   x[b, e]    = gamma - dist[b, e]                p = sigmoid(x) in float32 (sigmoidf_fast)
//   mrg_transe_bce_fwd     loss = mean over b, e of (y - 1) * max(log1p(-p), -100) - y * max(log p, -100)      (EPI_BCE's term, gemm.hpp)
//   mrg_transe_bce_dlogit  dl   = gscale * (p - y) * (p (1 - p) / max(p (1 - p), 1e-12)) for the entities [c0, c1)   (EPI_BCE_GRAD's)
//   mrg_transe_rank        rank = 1 + #{e != t, not filtered : dist_e < dist_t or (dist_e == dist_t and e < t)}
// An L1 distance has no matrix form (scoring.hip): this is VALU work.  The dense transe_fwd_k reads two LDS words per absolute
// difference and is bound by LDS; l1_sweep_k is register-tiled: 256 threads own a tile of 64 queries x 64 entities as a 16 x 16 grid of
// 4 x 4 micro-tiles, operands staged through LDS in slices of 32 columns laid out [c][row], so that a thread fetches its four query
// values and its four entity values of a column with two 16-byte LDS reads (the 16 lanes of a micro-tile row cover one 256-byte bank
// row, the four micro-tile rows of a wave read broadcasts) for 16 subtract / |.|-add pairs.
// Every distance is ONE float32 accumulator, acc += fabsf(o - e) over c ascending from 0, padding adding exact zeros: the chain of
// transe_fwd_k, so fused and dense agree bit for bit on dist, and so does l1_target_k (one thread per query, same chain), whose target
// distance therefore ties exactly with a duplicate of the target's entity row.  Ranks compare dist itself (gamma - dist and
// sigmoid(gamma - dist) are monotone non-increasing in dist and only merge values).
// No float atomics: the loss leaves one float64 partial per workgroup (lane sums in register order, butterfly per wave, the four waves
// added in order), bce_finish_k adds the partials in a fixed order; counts are integer atomics, one per (row, workgroup).
// Labels / filters of a tile: thread r < 64 walks the slice of tile row r's ascending list that falls into the tile's 64 entities
// (binary search for its start, as gemm_bce_label_words does) and leaves a 64-bit mask in LDS.  The mask, the epilogues' edge set-up, the
// rank count and the partial sums are sweep_tile.hpp's, shared with the mixed-score sweep (sf_mix_1n.hip); the two-operand staging
// stays written out here (through the header's per-operand helpers the compiler encoded this kernel's compares differently).
#include "sweep_host.hpp"      // the launch bounds, SweepGrid, the plans, the workspace's rounding and base, the checks; the prep / finish kernels
#include "sweep_tile.hpp"      // the tile's staging, mask, rank count and partial sums
#include "topk_parts.hpp"      // L1_TOPK: the order, the per-tile selection, the merge

namespace mrg {

constexpr int L1_T = SWT_T;         // tile: 64 queries x 64 entities
constexpr int L1_C = SWT_C;         // columns per LDS slice
enum { L1_LOSS = 0, L1_DLOGIT = 1, L1_RANK = 2, L1_TOPK = 3 };
constexpr bool l1_filters(int epi) { return epi == L1_RANK || epi == L1_TOPK; }      // the tile's mask: filtered members, read through qinfo

struct L1Args {
  const float* obj;           // [rows][D]: the launch's query rows
  const float* ent;           // the entity row of the launch's column 0
  int64_t rows;
  int ncols, D;
  int e0;                     // entity id of the launch's column 0
  float gamma;
  const int32_t* qlist;       // L1_LOSS / L1_DLOGIT: [rows][2] begin and end of the query's object list in `list`
  const int32_t* qinfo;       // L1_RANK / L1_TOPK: [rows][4] target (L1_TOPK: -1), begin and end of the filter list in `list` / gone_at, `when`
  const int32_t* list;        // entity ids, ascending inside a list
  const int32_t* gone_at;     // L1_RANK / L1_TOPK: per member, filtered iff gone_at > when
  float v_zero, v_one;
  double* partial;            // L1_LOSS: [gridDim.y][gridDim.x]
  const float* gscale;        // L1_DLOGIT: [1] on the device
  float* dl;                  // L1_DLOGIT: element (row 0, column 0) of the launch
  int64_t ld;
  const float* tdist;         // L1_RANK: [rows] the target's distance (l1_target_k)
  unsigned* counts;           // L1_RANK: [rows], zeroed
  TopkEnt* part;              // L1_TOPK: [rows][gridDim.x][k] the (row, tile) lists
  int k;
  const float* run_vals;      // L1_TOPK: [rows][k] the rows' running lists after the column blocks swept so far: their k-th entry prunes
  const int32_t* run_ids;
};

// tdist[i] = sum_c |obj[i, c] - ent[target_i, c]|, the sweep's chain
__global__ void l1_target_k(const float* __restrict__ obj, const float* __restrict__ ent, const int32_t* __restrict__ qinfo, int64_t Q, int D,
                            float* __restrict__ tdist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const float* __restrict__ o = obj + i * D;
  const float* __restrict__ e = ent + (int64_t)qinfo[i * 4] * D;
  float acc = 0.f;
  for (int c = 0; c < D; ++c) acc += fabsf(o[c] - e[c]);
  tdist[i] = acc;
}

template <int EPI, bool VEC4>
__global__ __launch_bounds__(256) void l1_sweep_k(const L1Args a) {
  __shared__ __attribute__((aligned(16))) float so[L1_C][L1_T];
  __shared__ __attribute__((aligned(16))) float se[L1_C][L1_T];
  __shared__ unsigned long long smask[L1_T];
  __shared__ unsigned scnt[L1_T];
  __shared__ double sred[1][4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int col0 = blockIdx.x * L1_T;
  const int64_t row0 = (int64_t)blockIdx.y * L1_T;
  const int D = a.D;

  // the tile row's labels (filtered members) as bits
  if (tid < L1_T) smask[tid] = sweep_tile_mask<l1_filters(EPI)>(a, row0 + tid, col0);

  // staging: thread (r = tid & 63, part = tid >> 6) carries row r of both operands; per slice 8 of its 32 columns
  const int r = tid & 63, part = tid >> 6;
  const bool qok = row0 + r < a.rows, eok = col0 + r < a.ncols;
  const float* __restrict__ qp = a.obj + (qok ? (row0 + r) * D : 0);
  const float* __restrict__ ep = a.ent + (eok ? (int64_t)(col0 + r) * D : 0);
  float pq[8], pe[8];
  auto fetch = [&](int c0) {
    if constexpr (VEC4) {                                    // D % 4 == 0, 16-byte aligned rows: columns c .. c + 3
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = c0 + (part + 4 * h) * 4;
        float4 vq = make_float4(0.f, 0.f, 0.f, 0.f), ve = vq;
        if (c < D) {
          if (qok) vq = *reinterpret_cast<const float4*>(qp + c);
          if (eok) ve = *reinterpret_cast<const float4*>(ep + c);
        }
        pq[h * 4] = vq.x; pq[h * 4 + 1] = vq.y; pq[h * 4 + 2] = vq.z; pq[h * 4 + 3] = vq.w;
        pe[h * 4] = ve.x; pe[h * 4 + 1] = ve.y; pe[h * 4 + 2] = ve.z; pe[h * 4 + 3] = ve.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = c0 + part + 4 * k;
        pq[k] = (qok && c < D) ? qp[c] : 0.f;
        pe[k] = (eok && c < D) ? ep[c] : 0.f;
      }
    }
  };
  auto stash = [&]() {                                       // lanes of a wave write 64 consecutive floats of one [c] row: conflict free
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = VEC4 ? (part + 4 * (k >> 2)) * 4 + (k & 3) : part + 4 * k;
      so[c][r] = pq[k];
      se[c][r] = pe[k];
    }
  };

  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  fetch(0);
  for (int c0 = 0; c0 < D; c0 += L1_C) {
    stash();
    __syncthreads();
    if (c0 + L1_C < D) fetch(c0 + L1_C);                     // the next slice travels while this one is consumed
    const int cn = D - c0 < L1_C ? D - c0 : L1_C;
#pragma unroll 8
    for (int c = 0; c < cn; ++c) {
      const float4 o = *reinterpret_cast<const float4*>(&so[c][ty * 4]);
      const float4 e = *reinterpret_cast<const float4*>(&se[c][tx * 4]);
      const float ov[4] = {o.x, o.y, o.z, o.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += fabsf(ov[i] - ev[j]);
    }
    __syncthreads();
  }

  // ---- epilogues: element (i, j) of the thread is (row0 + ty * 4 + i, col0 + tx * 4 + j) ----
  unsigned long long mrow[4];
  bool rok[4], cok[4];
  sweep_edges(smask, tx, ty, row0, col0, a.rows, a.ncols, mrow, rok, cok);

  if constexpr (EPI == L1_LOSS) {
    double s[1] = {0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = sweep_bce_term(sigmoidf_fast(a.gamma - acc[i][j]), ((mrow[i] >> j) & 1ull) ? a.v_one : a.v_zero);
        s[0] += (rok[i] && cok[j]) ? (double)t : 0.0;
      }
    sweep_partials<1>(s, sred, tid, a.partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x));
  } else if constexpr (EPI == L1_DLOGIT) {
    const float gs = a.gscale[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!rok[i]) continue;
      float* __restrict__ out = a.dl + (row0 + ty * 4 + i) * a.ld + col0 + tx * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float y = ((mrow[i] >> j) & 1ull) ? a.v_one : a.v_zero;
        const float p = sigmoidf_fast(a.gamma - acc[i][j]);
        const float pq1 = p * (1.f - p);
        if (cok[j]) out[j] = gs * (p - y) * (pq1 / fmaxf(pq1, 1e-12f));
      }
    }
  } else if constexpr (EPI == L1_TOPK) {
    // a row's 64 columns sit in the 16 consecutive lanes tx of micro-tile row ty, four per lane: topk_select's layout
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[4];
      int id[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = cok[j] && !((mrow[i] >> j) & 1ull);
        v[j] = ok ? acc[i][j] : topk_pad<false>();
        id[j] = ok ? a.e0 + col0 + tx * 4 + j : TOPK_NONE;
      }
      const int64_t row = row0 + ty * 4 + i;
      const int64_t kth = (rok[i] ? row : a.rows - 1) * a.k + a.k - 1;
      topk_select<false, 16, 4>(v, id, a.run_vals[kth], a.run_ids[kth], a.k, a.part + (row * gridDim.x + blockIdx.x) * a.k, rok[i]);
    }
  } else {
    sweep_rank_count<true>(mrow, rok, cok, tid, row0, a.rows, a.e0 + col0, a.tdist, a.qinfo, scnt, a.counts, [&](int i, int j) { return acc[i][j]; });
  }
}

inline SweepGrid l1_grid(int64_t rows_all, int64_t c0, int64_t c1, int64_t row_chunk = RANK_CHUNK) {
  return SweepGrid{rows_all, c0, c1, L1_T, L1_T, row_chunk};
}

// ncols: the columns a call sweeps (N for the forward, c1 - c0 for the logit gradient); one float64 partial per workgroup
inline SweepBcePlan l1_bce_plan(int64_t B, int64_t ncols) { return sweep_bce_plan(l1_grid(B, 0, ncols), B, 1); }

// The sweep over the columns [c0, c1) of all rows on l1_grid: column blocks of BCE_COLS outermost, row chunks of RANK_CHUNK inside.  `all`
// carries what does not change from launch to launch; L1_LOSS appends its launches' partials at all.partial.  L1_TOPK: every launch fills
// all.part, and after(q0, rows, column tiles) follows it (the merge into the running lists).
template <int EPI, class AFTER>
static int l1_sweep(const L1Args& all, const float* obj, const float* ent, int64_t rows_all, int64_t c0, int64_t c1, hipStream_t st,
                    int64_t row_chunk, AFTER&& after) {
  const bool vec = all.D % 4 == 0 && aligned16(obj) && aligned16(ent);
  const SweepGrid sg = l1_grid(rows_all, c0, c1, row_chunk);
  return sg.each([&](int64_t q0, int64_t rows, int64_t c, int64_t nc, int64_t wg0) {
    L1Args a = all;
    a.obj = obj + q0 * a.D; a.ent = ent + c * a.D; a.rows = rows; a.ncols = (int)nc; a.e0 = (int)c;
    if (EPI == L1_RANK) { a.qinfo = all.qinfo + q0 * 4; a.tdist = all.tdist + q0; a.counts = all.counts + q0; }
    else if (EPI == L1_TOPK) { a.qinfo = all.qinfo + q0 * 4; a.run_vals = all.run_vals + q0 * a.k; a.run_ids = all.run_ids + q0 * a.k; }
    else a.qlist = all.qlist + q0 * 2;
    if (EPI == L1_DLOGIT) a.dl = all.dl + q0 * a.ld + (c - c0);
    if (EPI == L1_LOSS) a.partial = all.partial + wg0;
    const dim3 grid(sg.col_tiles(nc), sg.row_tiles(rows));
    if (vec) hipLaunchKernelGGL((l1_sweep_k<EPI, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((l1_sweep_k<EPI, false>), grid, dim3(256), 0, st, a);
    MRG_LAUNCH_CHECK();
    return (int)after(q0, rows, (int)grid.x);
  });
}
template <int EPI>
static int l1_sweep(const L1Args& all, const float* obj, const float* ent, int64_t rows_all, int64_t c0, int64_t c1, hipStream_t st) {
  return l1_sweep<EPI>(all, obj, ent, rows_all, c0, c1, st, RANK_CHUNK, [](int64_t, int64_t, int) { return (int)MRG_OK; });
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_transe_bce_workspace_bytes(int64_t B, int64_t ncols, int D) {
  if (!sweep_shape_ok(B, ncols, D, false)) return MRG_E_SHAPE;
  return (int64_t)l1_bce_plan(B, ncols).total;
}

// The body of both entry points from the label pointers on.  dl == NULL: the loss over the columns [0, N) = [c0, c1)
// (mrg_transe_bce_fwd); else the logit gradient of the columns [c0, c1) (mrg_transe_bce_dlogit).
static int l1_bce_run(const float* obj, const float* ent, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr, const int32_t* objs,
                      int64_t U, float gamma, float v_zero, float v_one, int64_t B, int64_t N, int D, int64_t c0, int64_t c1, float* loss,
                      const float* gscale, float* dl, void* ws, int64_t ws_bytes, void* stream) {
  if (!sweep_labels_ok(U, qkey, keys, rowptr, objs)) return MRG_E_NULLPTR;
  const SweepBcePlan p = l1_bce_plan(B, c1 - c0);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = sweep_ws_base(ws);
  int32_t* qlist = (int32_t*)(w + p.qlist);
  double* partial = (double*)(w + p.partial);
  int rc = sweep_launch_rows(bce_prep_k, B, st, qkey, keys, rowptr, U, B, qlist);
  if (rc != MRG_OK) return rc;
  L1Args a{};
  a.D = D; a.gamma = gamma; a.qlist = qlist; a.list = objs; a.v_zero = v_zero; a.v_one = v_one;
  if (dl) {
    a.gscale = gscale; a.dl = dl; a.ld = c1 - c0;
    return l1_sweep<L1_DLOGIT>(a, obj, ent, B, c0, c1, st);
  }
  a.partial = partial;
  rc = l1_sweep<L1_LOSS>(a, obj, ent, B, c0, c1, st);
  if (rc != MRG_OK) return rc;
  return sweep_launch_rows(bce_finish_k, 1, st, partial, p.nparts, 1.0 / ((double)B * (double)N), loss);
}

extern "C" int mrg_transe_bce_fwd(const float* obj, const float* ent, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr,
                                  const int32_t* objs, int64_t U, float gamma, float v_zero, float v_one, int64_t B, int64_t N, int D, float* loss,
                                  void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, false)) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!obj || !ent || !loss) return MRG_E_NULLPTR;
  return l1_bce_run(obj, ent, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, 0, N, loss, nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int mrg_transe_bce_dlogit(const float* obj, const float* ent, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr,
                                     const int32_t* objs, int64_t U, float gamma, float v_zero, float v_one, int64_t B, int64_t N, int D,
                                     int64_t c0, int64_t c1, const float* gscale, float* dl, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, false) || c0 < 0 || c1 <= c0 || c1 > N) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!obj || !ent || !gscale || !dl) return MRG_E_NULLPTR;
  return l1_bce_run(obj, ent, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, c0, c1, nullptr, gscale, dl, ws, ws_bytes, stream);
}

extern "C" int64_t mrg_transe_rank_workspace_bytes(int64_t Q, int64_t N, int D) {
  if (!sweep_shape_ok(Q, N, D, false)) return MRG_E_SHAPE;
  return (int64_t)sweep_rank_plan(Q).total;
}

extern "C" int mrg_transe_rank(const float* obj, const float* ent, const int32_t* t_idx, const int64_t* qkey, const int32_t* when,
                               const int64_t* keys, const int32_t* rowptr, const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q,
                               int64_t N, int D, int64_t* ranks, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, false)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!obj || !ent || !t_idx || !ranks) return MRG_E_NULLPTR;
  if (!sweep_labels_ok(U, qkey, when, keys, rowptr, members, gone_at)) return MRG_E_NULLPTR;
  const SweepRankPlan p = sweep_rank_plan(Q);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = sweep_ws_base(ws);
  int32_t* qinfo = (int32_t*)(w + p.qinfo);
  float* tdist = (float*)(w + p.tval);
  unsigned* counts = (unsigned*)(w + p.counts);
  int rc = sweep_launch_rows(rank_prep_k, Q, st, t_idx, qkey, when, keys, rowptr, U, Q, qinfo, counts);
  if (rc != MRG_OK) return rc;
  rc = sweep_launch_rows(l1_target_k, Q, st, obj, ent, qinfo, Q, D, tdist);
  if (rc != MRG_OK) return rc;
  L1Args a{};
  a.D = D; a.qinfo = qinfo; a.list = members; a.gone_at = gone_at; a.tdist = tdist; a.counts = counts;
  rc = l1_sweep<L1_RANK>(a, obj, ent, Q, 0, N, st);
  if (rc != MRG_OK) return rc;
  return sweep_launch_rows(rank_finish_k, Q, st, counts, ranks, Q);
}

// mrg_rows_topk on the L1 distance: the k unfiltered entities nearest to every query row, nearest first (topk_parts.hpp).  The
// distances are l1_sweep_k's accumulators, the ones mrg_transe_rank compares.
static_assert(TopkTileCheck<L1_T, L1_T>::ok, "");

extern "C" int64_t mrg_transe_topk_workspace_bytes(int64_t Q, int64_t N, int D, int k) {
  if (!sweep_shape_ok(Q, N, D, false) || !topk_k_ok(k)) return MRG_E_SHAPE;
  return (int64_t)topk_plan(Q, N, k, L1_T, L1_T, 0).total;
}

extern "C" int mrg_transe_topk(const float* obj, const float* ent, const int64_t* qkey, const int32_t* when, const int64_t* keys,
                               const int32_t* rowptr, const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D,
                               int k, int32_t* ids, float* vals, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, false) || !topk_k_ok(k)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!obj || !ent || !ids || !vals) return MRG_E_NULLPTR;
  if (!sweep_labels_ok(U, qkey, when, keys, rowptr, members, gone_at)) return MRG_E_NULLPTR;
  const TopkPlan p = topk_plan(Q, N, k, L1_T, L1_T, 0);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* w = sweep_ws_base(ws);
  int32_t* qinfo = (int32_t*)(w + p.qinfo);
  TopkEnt* part = (TopkEnt*)(w + p.part);
  int rc = sweep_launch_rows(topk_prep_k, Q, st, qkey, when, keys, rowptr, U, Q, k, topk_pad<false>(), qinfo, ids, vals);
  if (rc != MRG_OK) return rc;
  L1Args a{};
  a.D = D; a.qinfo = qinfo; a.list = members; a.gone_at = gone_at; a.part = part; a.k = k; a.run_vals = vals; a.run_ids = ids;
  return l1_sweep<L1_TOPK>(a, obj, ent, Q, 0, N, st, p.chunk, [&](int64_t q0, int64_t rows, int ntile) {
    return topk_merge_launch<false>(part, ntile, k, rows, ids + q0 * k, vals + q0 * k, st);
  });
}
