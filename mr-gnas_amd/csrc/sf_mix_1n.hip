// The score-function search leg without a [B, N] tensor: the 1-N loss, its gradients and the filtered ranks under the MIXED score of
// MixedOp_SF over NS = 2 scorers, SF_OPS = ['sf_TransE', 'sf_DisMult'] (reference models/cell_lp.py:36-50, 71-86, 191-200; the supernet's
// score_f line, models/model_search_lp.py:160-161), or NS = 3, ['sf_TransE', 'sf_DisMult', 'sf_ConvE'] (models/operations_lp.py:26-30; the
// genotype the reference's training driver ships ends in sf_ConvE, train/mr_lp_train.py:380).  ONE template over NS.
//   dist[b, e]  = sum_c |obj[b, c] - ent[e, c]|      obj = sub + rel, float32, formed by the caller
//   dot_k[b, e] = sum_c q_k[b, c] * ent[e, c]        q_1 = qd = sub * rel;  q_2 = qh = ConvE's hidden row after BN2 + ReLU
//                                                    (sf_ConvE_op.query);  float32, formed by the caller
//   p0 = sigmoid(gamma - dist)   p_k = sigmoid(dot_k)   p = (w0 * p0 + w1 * p1) [+ w2 * p2]            (mix_prob: float32, no contraction)
//   mrg_sfmix[3]_bce_fwd   loss = mean over b, e of (y - 1) * max(log1p(-p), -100) - y * max(log p, -100)      (EPI_BCE's term on p)
//   mrg_sfmix[3]_bce_grad  G = gscale * (p - y) / max((1 - p) p, 1e-12);  dl_k = (G w_k) ((1 - p_k) p_k) for the entities [c0, c1);
//                          dw_k = sum over b, e of G p_k
//   mrg_sfmix[3]_rank      rank = 1 + #{e != t, not filtered : p_e > p_t or (p_e == p_t and e < t)}
// BCE(sum w_k p_k, y) is no function of the BCE(p_k, y): all probabilities are needed at the same (b, e), so neither the L1 sweep
// (transe_1n.hip) nor the row GEMM's (bce.hip) can form it.  mix_sweep_k is l1_sweep_k's tile (sweep_tile.hpp) with NS + 1 staged
// operands (obj, the q_k, the entity rows: 8 KiB each) and NS accumulator sets per thread.  Per (query, entity, column): a subtract, an
// |.|-add and NS - 1 fused multiply-adds on one entity value read once.
// LDS: every array is [32][64] floats, one 256-byte bank row per column c.  A wave's lanes are tx = 0 .. 15 and four values of ty: the
// 128-bit reads of the query arrays touch four slots of a bank row (the rest is broadcast), the entity read all sixteen; the 32-bit
// writes of a wave cover one bank row.  Every array is a whole number of bank rows, so none moves another's banks: conflict free at
// both NS.  NS = 3: 48 accumulators, 32 staging registers and 16 operand values put the kernel near 140 VGPRs, three waves per SIMD,
// against four or five at NS = 2 (about 100 VGPRs).  No scratch.
// The arithmetic, fixed (tests/test_sweep_bits_gpu.py holds every output to recorded bits):
//   * dist is ONE float32 accumulator, dist += fabsf(o - e), and every dot_k ONE, dot_k = __builtin_fmaf(q_k, e, dot_k) written out,
//     with c ascending from 0; padding adds exact zeros.  dist is l1_sweep_k's and transe_fwd_k's chain, the chains at NS = 3 are those
//     at NS = 2 and one more, and mix_target_k (one thread per query) runs the identical chains.
//   * mix_prob forms ((w0 p0 + w1 p1) + w2 p2) left to right, every product and every sum rounded on its own under
//     `#pragma clang fp contract(off)` inside it, for the sweep and the target kernel alike: a duplicate of the target's entity row
//     ties exactly, and w2 = 0 adds an exact zero to the two-way p.
//   * the gradient expressions are (G w_k) ((1 - p_k) p_k) and G p_k into float64, with the max(., 1e-12) / max(log, -100) guards.
//   * no float atomics: the loss and the NS weight-gradient sums leave float64 partials laid out [workgroup][NS] (sweep_tile.hpp's
//     order inside a workgroup); mix_dw_finish_k adds a component's partials as a 256-strided per-thread sum, then the halving tree,
//     and adds the result to dw when c0 > 0.
//   * the tie rule is p > pt || (p == pt && id < tg) (sweep_rank_count).
#include "sweep_host.hpp"      // the launch bounds, SweepGrid, the plans, the workspace's rounding and base, the checks; the prep / finish kernels
#include "sweep_tile.hpp"      // the tile's staging, mask, rank count and partial sums
#include <utility>

namespace mrg {

enum { MIX_LOSS = 0, MIX_GRAD = 1, MIX_RANK = 2 };

template <int NS>
struct MixArgs {
  const float* obj;           // [rows][D]: sub + rel of the launch's query rows
  const float* q[NS - 1];     // [rows][D] each: qd = sub * rel, then qh = ConvE's hidden rows, of the launch's query rows
  const float* ent;           // the entity row of the launch's column 0
  const float* w;             // [NS] on the device: TransE's, DistMult's, ConvE's weight (the order of SF_OPS)
  int64_t rows;
  int ncols, D;
  int e0;                     // entity id of the launch's column 0
  float gamma;
  const int32_t* qlist;       // MIX_LOSS / MIX_GRAD: [rows][2] begin and end of the query's object list in `list`
  const int32_t* qinfo;       // MIX_RANK: [rows][4] target, begin and end of the filter list in `list` / gone_at, `when`
  const int32_t* list;        // entity ids, ascending inside a list
  const int32_t* gone_at;     // MIX_RANK: per member, filtered iff gone_at > when
  float v_zero, v_one;
  double* partial;            // MIX_LOSS: [workgroups]; MIX_GRAD: [workgroups][NS] the weight-gradient sums
  const float* gscale;        // MIX_GRAD: [1] on the device
  float* dl[NS];              // MIX_GRAD: element (row 0, column 0) of the launch; gradient with respect to gamma - dist, then to dot_k
  int64_t ld;
  const float* tp;            // MIX_RANK: [rows] the target's mixed probability (mix_target_k)
  unsigned* counts;           // MIX_RANK: [rows], zeroed
};

// f(K) for K = 0 .. N - 1 as compile-time constants, expanded by the front end (a `#pragma unroll` loop is only unrolled after the
// passes that shape the epilogues' branches and addresses have run)
template <class F, int... K>
__device__ __forceinline__ void mix_each(F&& f, std::integer_sequence<int, K...>) { (f(std::integral_constant<int, K>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void mix_each(F&& f) { mix_each(f, std::make_integer_sequence<int, N>{}); }

template <int NS>
struct MixP { float pk[NS], p; };

// The mixed probability of one (query, entity) pair from its NS accumulators: the literal formulation's sum(w * op(...)), i.e.
// (w0 * p0 + w1 * p1) + w2 * p2 in float32, each product and each sum rounded on its own.  Contraction is switched off for the
// statements themselves: without OCML_BASIC_ROUNDED_OPERATIONS clang's __clang_hip_math.h defines __fmul_rn / __fadd_rn as plain
// `x * y` / `x + y`, which carry the translation unit's -ffp-contract=fast, and a product that is fused into the sum in the sweep but
// not in mix_target_k (or the other product of the two) would break the exact tie of a duplicated row.
// With sum w_k = 1 the float32 p can round one ulp above 1: then log1pf(-p) is NaN and fmaxf(NaN, -100) = -100 in the loss, and
// (1 - p) p < 0 is raised to 1e-12 in the gradient: finite values where torch's binary_cross_entropy, which takes inputs in [0, 1]
// only, rejects the dense formulation's p.
template <int NS>
__device__ __forceinline__ MixP<NS> mix_prob(float dist, const float (&dot)[NS - 1], float gamma, const float (&w)[NS]) {
#pragma clang fp contract(off)
  MixP<NS> r;
  float t[NS];
  r.pk[0] = sigmoidf_fast(gamma - dist);
#pragma unroll
  for (int k = 1; k < NS; ++k) r.pk[k] = sigmoidf_fast(dot[k - 1]);
#pragma unroll
  for (int k = 0; k < NS; ++k) t[k] = w[k] * r.pk[k];
  r.p = t[0] + t[1];
#pragma unroll
  for (int k = 2; k < NS; ++k) r.p = r.p + t[k];
  return r;
}

// The operands of an entry point: obj, the NS - 1 dot operands (qd, then qh), ent, w; all [.][D] float32 but w [NS]
template <int NS>
struct MixOperands {
  const float* obj;
  const float* q[NS - 1];
  const float* ent;
  const float* w;
  bool ok() const {
    bool r = obj && ent && w;
    for (int k = 0; k < NS - 1; ++k) r = r && q[k];
    return r;
  }
  MixArgs<NS> args(int D, float gamma) const {
    MixArgs<NS> a{};
    a.obj = obj; a.ent = ent; a.w = w; a.D = D; a.gamma = gamma;
    for (int k = 0; k < NS - 1; ++k) a.q[k] = q[k];
    return a;
  }
};

// tp[i] = the mixed probability of query i's target: the sweep's NS chains, one thread per query
template <int NS>
__global__ void mix_target_k(const MixOperands<NS> in, const int32_t* __restrict__ qinfo, int64_t Q, int D, float gamma, float* __restrict__ tp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const float* __restrict__ o = in.obj + i * D;
  const float* __restrict__ e = in.ent + (int64_t)qinfo[i * 4] * D;
  const float* q[NS - 1];
  float dist = 0.f, dot[NS - 1], wv[NS];
#pragma unroll
  for (int k = 0; k < NS - 1; ++k) { q[k] = in.q[k] + i * D; dot[k] = 0.f; }
  for (int c = 0; c < D; ++c) {
    const float ev = e[c];
    dist += fabsf(o[c] - ev);
#pragma unroll
    for (int k = 0; k < NS - 1; ++k) dot[k] = __builtin_fmaf(q[k][c], ev, dot[k]);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) wv[k] = in.w[k];
  tp[i] = mix_prob<NS>(dist, dot, gamma, wv).p;
}

template <int NS, int EPI, bool VEC4>
__global__ __launch_bounds__(256) void mix_sweep_k(const MixArgs<NS> a) {
  __shared__ __attribute__((aligned(16))) float sm[NS + 1][SWT_C][SWT_T];      // obj, the q_k, the entity rows
  __shared__ unsigned long long smask[SWT_T];
  __shared__ unsigned scnt[SWT_T];
  __shared__ double sred[NS][4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int col0 = blockIdx.x * SWT_T;
  const int64_t row0 = (int64_t)blockIdx.y * SWT_T;
  const int D = a.D;

  // the tile row's labels (filtered members) as bits
  if (tid < SWT_T) smask[tid] = sweep_tile_mask<EPI == MIX_RANK>(a, row0 + tid, col0);

  // staging: thread (r = tid & 63, part = tid >> 6) carries row r of the NS + 1 operands; per slice 8 of its 32 columns
  const int r = tid & 63, part = tid >> 6;
  const bool qok = row0 + r < a.rows, eok = col0 + r < a.ncols;
  const int64_t qoff = qok ? (row0 + r) * D : 0;
  const float* __restrict__ src[NS + 1];
  float pre[NS + 1][8];
  src[0] = a.obj + qoff;
#pragma unroll
  for (int k = 1; k < NS; ++k) src[k] = a.q[k - 1] + qoff;
  src[NS] = a.ent + (eok ? (int64_t)(col0 + r) * D : 0);
  auto fetch = [&](int c0) {
#pragma unroll
    for (int k = 0; k <= NS; ++k) sweep_fetch<VEC4>(src[k], k < NS ? qok : eok, c0, part, D, pre[k]);
  };

  float dist[4][4], dot[NS - 1][4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dist[i][j] = 0.f;
#pragma unroll
      for (int k = 0; k < NS - 1; ++k) dot[k][i][j] = 0.f;
    }

  fetch(0);
  for (int c0 = 0; c0 < D; c0 += SWT_C) {
#pragma unroll
    for (int k = 0; k <= NS; ++k) sweep_stash<VEC4>(sm[k], r, part, pre[k]);
    __syncthreads();
    if (c0 + SWT_C < D) fetch(c0 + SWT_C);                   // the next slice travels while this one is consumed
    const int cn = D - c0 < SWT_C ? D - c0 : SWT_C;
#pragma unroll 4
    for (int c = 0; c < cn; ++c) {
      const float4 o = *reinterpret_cast<const float4*>(&sm[0][c][ty * 4]);
      float4 q[NS - 1];
#pragma unroll
      for (int k = 0; k < NS - 1; ++k) q[k] = *reinterpret_cast<const float4*>(&sm[k + 1][c][ty * 4]);
      const float4 e = *reinterpret_cast<const float4*>(&sm[NS][c][tx * 4]);
      const float ov[4] = {o.x, o.y, o.z, o.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dist[i][j] += fabsf(ov[i] - ev[j]);
#pragma unroll
          for (int k = 0; k < NS - 1; ++k) {
            const float qv[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
            dot[k][i][j] = __builtin_fmaf(qv[i], ev[j], dot[k][i][j]);
          }
        }
    }
    __syncthreads();
  }

  // ---- epilogues: element (i, j) of the thread is (row0 + ty * 4 + i, col0 + tx * 4 + j) ----
  float w[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) w[k] = a.w[k];
  unsigned long long mrow[4];
  bool rok[4], cok[4];
  sweep_edges(smask, tx, ty, row0, col0, a.rows, a.ncols, mrow, rok, cok);
  auto prob = [&](int i, int j) {
    float d[NS - 1];
#pragma unroll
    for (int k = 0; k < NS - 1; ++k) d[k] = dot[k][i][j];
    return mix_prob<NS>(dist[i][j], d, a.gamma, w);
  };
  const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;

  if constexpr (EPI == MIX_LOSS) {
    double s[1] = {0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = sweep_bce_term(prob(i, j).p, ((mrow[i] >> j) & 1ull) ? a.v_one : a.v_zero);
        s[0] += (rok[i] && cok[j]) ? (double)t : 0.0;
      }
    sweep_partials<1>(s, reinterpret_cast<double(&)[1][4]>(sred), tid, a.partial + wg);
  } else if constexpr (EPI == MIX_GRAD) {
    const float gs = a.gscale[0];
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t off = (row0 + ty * 4 + i) * a.ld + col0 + tx * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float y = ((mrow[i] >> j) & 1ull) ? a.v_one : a.v_zero;
        const MixP<NS> m = prob(i, j);
        const float G = gs * (m.p - y) / fmaxf((1.f - m.p) * m.p, 1e-12f);
        const bool ok = rok[i] && cok[j];
        if (ok) mix_each<NS>([&](auto k) __attribute__((always_inline)) { a.dl[k][off + j] = (G * w[k]) * ((1.f - m.pk[k]) * m.pk[k]); });
        mix_each<NS>([&](auto k) __attribute__((always_inline)) { s[k] += ok ? (double)(G * m.pk[k]) : 0.0; });
      }
    }
    sweep_partials<NS>(s, sred, tid, a.partial + wg * NS);
  } else {
    sweep_rank_count<false>(mrow, rok, cok, tid, row0, a.rows, a.e0 + col0, a.tp, a.qinfo, scnt, a.counts, [&](int i, int j) { return prob(i, j).p; });
  }
}

// dw[k] (+)= the n partials [n][NS] of component k = blockIdx.x added in bce_finish_k's order; add != 0: added to what dw holds
__global__ __launch_bounds__(256) void mix_dw_finish_k(const double* __restrict__ partial, int64_t n, int ns, int add, float* __restrict__ dw) {
  __shared__ double s[256];
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i * ns + k];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) dw[k] = add ? dw[k] + (float)s[0] : (float)s[0];
}

inline SweepGrid mix_grid(int64_t rows_all, int64_t c0, int64_t c1) { return SweepGrid{rows_all, c0, c1, SWT_T, SWT_T, RANK_CHUNK}; }
// ncols: the columns a call sweeps (N for the forward, c1 - c0 for the gradient); NS float64 per workgroup (the gradient's NS sums)
inline SweepBcePlan mix_bce_plan(int64_t B, int64_t ncols, int ns) { return sweep_bce_plan(mix_grid(B, 0, ncols), B, ns); }

// The sweep over the columns [c0, c1) of all rows on mix_grid: column blocks of BCE_COLS outermost, row chunks of RANK_CHUNK inside.
// `all` carries what does not change from launch to launch and the operands' first rows; the launches append their partials at
// all.partial.
template <int NS, int EPI>
static int mix_sweep(const MixArgs<NS>& all, int64_t rows_all, int64_t c0, int64_t c1, hipStream_t st) {
  bool vec = all.D % 4 == 0 && aligned16(all.obj) && aligned16(all.ent);
  for (int k = 0; k < NS - 1; ++k) vec = vec && aligned16(all.q[k]);
  const SweepGrid sg = mix_grid(rows_all, c0, c1);
  return sg.each([&](int64_t q0, int64_t rows, int64_t c, int64_t nc, int64_t wg0) {
    MixArgs<NS> a = all;
    a.obj = all.obj + q0 * a.D; a.ent = all.ent + c * a.D; a.rows = rows; a.ncols = (int)nc; a.e0 = (int)c;
    for (int k = 0; k < NS - 1; ++k) a.q[k] = all.q[k] + q0 * a.D;
    if (EPI == MIX_RANK) { a.qinfo = all.qinfo + q0 * 4; a.tp = all.tp + q0; a.counts = all.counts + q0; }
    else a.qlist = all.qlist + q0 * 2;
    if (EPI == MIX_GRAD) {
      for (int k = 0; k < NS; ++k) a.dl[k] = all.dl[k] + q0 * a.ld + (c - c0);
      a.partial = all.partial + wg0 * NS;
    }
    if (EPI == MIX_LOSS) a.partial = all.partial + wg0;
    const dim3 grid(sg.col_tiles(nc), sg.row_tiles(rows));
    if (vec) hipLaunchKernelGGL((mix_sweep_k<NS, EPI, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((mix_sweep_k<NS, EPI, false>), grid, dim3(256), 0, st, a);
    MRG_LAUNCH_CHECK();
    return (int)MRG_OK;
  });
}

// The body of mrg_sfmix[3]_bce_fwd (dl == NULL: the loss over the columns [0, N) = [c0, c1)) and of mrg_sfmix[3]_bce_grad (the
// gradients of the columns [c0, c1)), after the shape checks.
template <int NS>
static int mix_bce_run(const MixOperands<NS>& in, const int64_t* qkey, const int64_t* keys, const int32_t* rowptr, const int32_t* objs, int64_t U,
                       float gamma, float v_zero, float v_one, int64_t B, int64_t N, int D, int64_t c0, int64_t c1, float* loss,
                       const float* gscale, float* const* dl, float* dw, void* ws, int64_t ws_bytes, void* stream) {
  if (B == 0) return MRG_OK;
  if (!in.ok() || (dl ? !gscale || !dw : !loss)) return MRG_E_NULLPTR;
  for (int k = 0; dl && k < NS; ++k)
    if (!dl[k]) return MRG_E_NULLPTR;
  if (!sweep_labels_ok(U, qkey, keys, rowptr, objs)) return MRG_E_NULLPTR;
  const SweepBcePlan p = mix_bce_plan(B, c1 - c0, NS);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* wsb = sweep_ws_base(ws);
  int32_t* qlist = (int32_t*)(wsb + p.qlist);
  double* partial = (double*)(wsb + p.partial);
  int rc = sweep_launch_rows(bce_prep_k, B, st, qkey, keys, rowptr, U, B, qlist);
  if (rc != MRG_OK) return rc;
  MixArgs<NS> a = in.args(D, gamma);
  a.qlist = qlist; a.list = objs; a.v_zero = v_zero; a.v_one = v_one; a.partial = partial;
  if (dl) {
    a.gscale = gscale; a.ld = c1 - c0;
    for (int k = 0; k < NS; ++k) a.dl[k] = dl[k];
    rc = mix_sweep<NS, MIX_GRAD>(a, B, c0, c1, st);
    if (rc != MRG_OK) return rc;
    hipLaunchKernelGGL(mix_dw_finish_k, dim3(NS), dim3(256), 0, st, partial, p.nparts, NS, c0 > 0 ? 1 : 0, dw);
    MRG_LAUNCH_CHECK();
    return MRG_OK;
  }
  rc = mix_sweep<NS, MIX_LOSS>(a, B, c0, c1, st);
  if (rc != MRG_OK) return rc;
  return sweep_launch_rows(bce_finish_k, 1, st, partial, p.nparts, 1.0 / ((double)B * (double)N), loss);
}

// The body of mrg_sfmix[3]_rank after the shape checks
template <int NS>
static int mix_rank_run(const MixOperands<NS>& in, float gamma, const int32_t* t_idx, const int64_t* qkey, const int32_t* when,
                        const int64_t* keys, const int32_t* rowptr, const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q,
                        int64_t N, int D, int64_t* ranks, void* ws, int64_t ws_bytes, void* stream) {
  if (Q == 0) return MRG_OK;
  if (!in.ok() || !t_idx || !ranks) return MRG_E_NULLPTR;
  if (!sweep_labels_ok(U, qkey, when, keys, rowptr, members, gone_at)) return MRG_E_NULLPTR;
  const SweepRankPlan p = sweep_rank_plan(Q);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* wsb = sweep_ws_base(ws);
  int32_t* qinfo = (int32_t*)(wsb + p.qinfo);
  float* tp = (float*)(wsb + p.tval);
  unsigned* counts = (unsigned*)(wsb + p.counts);
  int rc = sweep_launch_rows(rank_prep_k, Q, st, t_idx, qkey, when, keys, rowptr, U, Q, qinfo, counts);
  if (rc != MRG_OK) return rc;
  rc = sweep_launch_rows(mix_target_k<NS>, Q, st, in, qinfo, Q, D, gamma, tp);
  if (rc != MRG_OK) return rc;
  MixArgs<NS> a = in.args(D, gamma);
  a.qinfo = qinfo; a.list = members; a.gone_at = gone_at; a.tp = tp; a.counts = counts;
  rc = mix_sweep<NS, MIX_RANK>(a, Q, 0, N, st);
  if (rc != MRG_OK) return rc;
  return sweep_launch_rows(rank_finish_k, Q, st, counts, ranks, Q);
}

static bool mix_grad_shape_ok(int64_t U, int64_t B, int64_t N, int D, int64_t c0, int64_t c1) {
  return U >= 0 && sweep_shape_ok(B, N, D, false) && c0 >= 0 && c1 > c0 && c1 <= N;
}

}  // namespace mrg

using namespace mrg;

// ---- the C ABI: two scorers (mrg_sfmix_*) and three (mrg_sfmix3_*), thin wrappers over the bodies above ----

extern "C" int64_t mrg_sfmix_bce_workspace_bytes(int64_t B, int64_t ncols, int D) {
  if (!sweep_shape_ok(B, ncols, D, false)) return MRG_E_SHAPE;
  return (int64_t)mix_bce_plan(B, ncols, 2).total;
}

extern "C" int64_t mrg_sfmix3_bce_workspace_bytes(int64_t B, int64_t ncols, int D) {
  if (!sweep_shape_ok(B, ncols, D, false)) return MRG_E_SHAPE;
  return (int64_t)mix_bce_plan(B, ncols, 3).total;
}

extern "C" int mrg_sfmix_bce_fwd(const float* obj, const float* qd, const float* ent, const float* w, const int64_t* qkey, const int64_t* keys,
                                 const int32_t* rowptr, const int32_t* objs, int64_t U, float gamma, float v_zero, float v_one, int64_t B,
                                 int64_t N, int D, float* loss, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, false)) return MRG_E_SHAPE;
  return mix_bce_run<2>({obj, {qd}, ent, w}, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, 0, N, loss, nullptr, nullptr, nullptr, ws,
                        ws_bytes, stream);
}

extern "C" int mrg_sfmix3_bce_fwd(const float* obj, const float* qd, const float* qh, const float* ent, const float* w, const int64_t* qkey,
                                  const int64_t* keys, const int32_t* rowptr, const int32_t* objs, int64_t U, float gamma, float v_zero,
                                  float v_one, int64_t B, int64_t N, int D, float* loss, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, false)) return MRG_E_SHAPE;
  return mix_bce_run<3>({obj, {qd, qh}, ent, w}, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, 0, N, loss, nullptr, nullptr, nullptr,
                        ws, ws_bytes, stream);
}

extern "C" int mrg_sfmix_bce_grad(const float* obj, const float* qd, const float* ent, const float* w, const int64_t* qkey,
                                  const int64_t* keys, const int32_t* rowptr, const int32_t* objs, int64_t U, float gamma, float v_zero,
                                  float v_one, int64_t B, int64_t N, int D, int64_t c0, int64_t c1, const float* gscale, float* dl0, float* dl1,
                                  float* dw, void* ws, int64_t ws_bytes, void* stream) {
  if (!mix_grad_shape_ok(U, B, N, D, c0, c1)) return MRG_E_SHAPE;
  float* const dl[2] = {dl0, dl1};
  return mix_bce_run<2>({obj, {qd}, ent, w}, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, c0, c1, nullptr, gscale, dl, dw, ws,
                        ws_bytes, stream);
}

extern "C" int mrg_sfmix3_bce_grad(const float* obj, const float* qd, const float* qh, const float* ent, const float* w, const int64_t* qkey,
                                   const int64_t* keys, const int32_t* rowptr, const int32_t* objs, int64_t U, float gamma, float v_zero,
                                   float v_one, int64_t B, int64_t N, int D, int64_t c0, int64_t c1, const float* gscale, float* dl0,
                                   float* dl1, float* dl2, float* dw, void* ws, int64_t ws_bytes, void* stream) {
  if (!mix_grad_shape_ok(U, B, N, D, c0, c1)) return MRG_E_SHAPE;
  float* const dl[3] = {dl0, dl1, dl2};
  return mix_bce_run<3>({obj, {qd, qh}, ent, w}, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, c0, c1, nullptr, gscale, dl, dw, ws,
                        ws_bytes, stream);
}

extern "C" int64_t mrg_sfmix_rank_workspace_bytes(int64_t Q, int64_t N, int D) {
  if (!sweep_shape_ok(Q, N, D, false)) return MRG_E_SHAPE;
  return (int64_t)sweep_rank_plan(Q).total;
}

extern "C" int64_t mrg_sfmix3_rank_workspace_bytes(int64_t Q, int64_t N, int D) { return mrg_sfmix_rank_workspace_bytes(Q, N, D); }

extern "C" int mrg_sfmix_rank(const float* obj, const float* qd, const float* ent, const float* w, float gamma, const int32_t* t_idx,
                              const int64_t* qkey, const int32_t* when, const int64_t* keys, const int32_t* rowptr, const int32_t* members,
                              const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t* ranks, void* ws, int64_t ws_bytes,
                              void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, false)) return MRG_E_SHAPE;
  return mix_rank_run<2>({obj, {qd}, ent, w}, gamma, t_idx, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, ranks, ws, ws_bytes, stream);
}

extern "C" int mrg_sfmix3_rank(const float* obj, const float* qd, const float* qh, const float* ent, const float* w, float gamma,
                               const int32_t* t_idx, const int64_t* qkey, const int32_t* when, const int64_t* keys, const int32_t* rowptr,
                               const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t* ranks,
                               void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, false)) return MRG_E_SHAPE;
  return mix_rank_run<3>({obj, {qd, qh}, ent, w}, gamma, t_idx, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, ranks, ws, ws_bytes, stream);
}
