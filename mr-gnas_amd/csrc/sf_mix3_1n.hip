// The score-function search leg over THREE scorers without a [B, N] tensor: the 1-N loss, its gradients and the filtered ranks under the
// MIXED score of MixedOp_SF over ['sf_TransE', 'sf_DisMult', 'sf_ConvE'] (reference models/operations_lp.py:26-30, models/cell_lp.py:36-50;
// the genotype the reference's training driver ships ends in sf_ConvE, train/mr_lp_train.py:380).
//   dist[b, e] = sum_c |obj[b, c] - ent[e, c]|      obj = sub + rel, float32, formed by the caller
//   dot [b, e] = sum_c qd[b, c] * ent[e, c]         qd  = sub * rel, float32, formed by the caller
//   dot2[b, e] = sum_c qh[b, c] * ent[e, c]         qh  = ConvE's hidden row after BN2 + ReLU (sf_ConvE_op.query), formed by the caller
//   p0 = sigmoid(gamma - dist)   p1 = sigmoid(dot)   p2 = sigmoid(dot2)   p = (w0 * p0 + w1 * p1) + w2 * p2   (mix_prob3: no contraction)
//   mrg_sfmix3_bce_fwd   loss = mean over b, e of (y - 1) * max(log1p(-p), -100) - y * max(log p, -100)      (EPI_BCE's term on p)
//   mrg_sfmix3_bce_grad  G = gscale * (p - y) / max((1 - p) p, 1e-12);  dl_k = (G w_k) ((1 - p_k) p_k), k = 0, 1, 2, for the entities
//                        [c0, c1);  dw_k = sum over b, e of G p_k
//   mrg_sfmix3_rank      rank = 1 + #{e != t, not filtered : p_e > p_t or (p_e == p_t and e < t)}
// mix3_sweep_k is sf_mix_1n.hip's mix_sweep_k -- 256 threads, 64 queries x 64 entities as a 16 x 16 grid of 4 x 4 micro-tiles, slices of 32
// columns in LDS laid out [c][row], the next slice fetched while this one is consumed -- with FOUR staged operands (obj, qd, qh, the
// entity rows: 32 KiB) and THREE accumulator sets per thread.  Per (query, entity, column): a subtract, an |.|-add and two fused
// multiply-adds on one entity value read once.  A separate file: the two-way kernels of sf_mix_1n.hip keep their code object as it is.
// LDS: every array is [32][64] floats, one 256-byte bank row per column c.  A wave's lanes are tx = 0 .. 15 and four values of ty: the
// 128-bit reads of the three query arrays touch four slots of a bank row (the rest is broadcast), the entity read all sixteen; the
// 32-bit writes of a wave cover one bank row.  The fourth array is a whole number of bank rows, so it moves no other array's banks:
// conflict free as the two-way sweep is.  32.6 KiB per workgroup would let four workgroups share a CU's 160 KiB; the 48 accumulators,
// 32 staging registers and 16 operand values put the kernel at 138 - 144 VGPRs, so three workgroups (three waves per SIMD) run, against
// four of the two-way sweep (96 - 108 VGPRs).  No scratch.
// Chains: dist and dot are mix_sweep_k's (equal bit for bit, so w2 = 0 reproduces the two-way numbers); dot2 is the same fused
// multiply-add chain on the third operand, c ascending from 0; mix3_target_k (one thread per query) runs the identical three.
// Padding adds exact zeros to all.  mix_prob3 is the one place the probability is formed, for the sweep and the target alike: a
// duplicate of the target's entity row ties exactly.
// No float atomics: the loss and the three weight-gradient sums leave float64 partials per workgroup (lane sums in register order,
// butterfly per wave, the four waves added in order) that a finish kernel adds in a fixed order; counts are integer atomics, one per
// (row, workgroup).
#include "sweep_host.hpp"      // the launch bounds, SweepGrid, the workspace's rounding and base, the checks; the prep / finish kernels

namespace mrg {

constexpr int MIX3_T = 64;          // tile: 64 queries x 64 entities
constexpr int MIX3_C = 32;          // columns per LDS slice
enum { MIX3_LOSS = 0, MIX3_GRAD = 1, MIX3_RANK = 2 };

struct Mix3Args {
  const float* obj;           // [rows][D]: sub + rel of the launch's query rows
  const float* qd;            // [rows][D]: sub * rel of the launch's query rows
  const float* qh;            // [rows][D]: ConvE's hidden rows of the launch's query rows
  const float* ent;           // the entity row of the launch's column 0
  const float* w;             // [3] on the device: TransE's, DistMult's, ConvE's weight
  int64_t rows;
  int ncols, D;
  int e0;                     // entity id of the launch's column 0
  float gamma;
  const int32_t* qlist;       // MIX3_LOSS / MIX3_GRAD: [rows][2] begin and end of the query's object list in `list`
  const int32_t* qinfo;       // MIX3_RANK: [rows][4] target, begin and end of the filter list in `list` / gone_at, `when`
  const int32_t* list;        // entity ids, ascending inside a list
  const int32_t* gone_at;     // MIX3_RANK: per member, filtered iff gone_at > when
  float v_zero, v_one;
  double* partial;            // MIX3_LOSS: [workgroups]; MIX3_GRAD: [workgroups][3] the weight-gradient sums
  const float* gscale;        // MIX3_GRAD: [1] on the device
  float* dl0;                 // MIX3_GRAD: element (row 0, column 0) of the launch, gradient with respect to gamma - dist
  float* dl1;                 //            ... with respect to dot
  float* dl2;                 //            ... with respect to dot2
  int64_t ld;
  const float* tp;            // MIX3_RANK: [rows] the target's mixed probability (mix3_target_k)
  unsigned* counts;           // MIX3_RANK: [rows], zeroed
};

struct MixP3 { float p0, p1, p2, p; };

// The mixed probability of one (query, entity) pair from its three accumulators: the literal formulation's sum(w * op(...)), i.e.
// (w0 * p0 + w1 * p1) + w2 * p2 in float32, each product and each sum rounded on its own.  Contraction is switched off for the
// statements themselves (sf_mix_1n.hip's mix_prob says why).  With w2 = 0 the last sum adds an exact zero: the two-way p.
__device__ __forceinline__ MixP3 mix_prob3(float dist, float dot, float dot2, float gamma, float w0, float w1, float w2) {
#pragma clang fp contract(off)
  MixP3 r;
  r.p0 = sigmoidf_fast(gamma - dist);
  r.p1 = sigmoidf_fast(dot);
  r.p2 = sigmoidf_fast(dot2);
  const float a = w0 * r.p0;
  const float b = w1 * r.p1;
  const float c = w2 * r.p2;
  const float ab = a + b;
  r.p = ab + c;
  return r;
}

// tp[i] = the mixed probability of query i's target: the sweep's three chains, one thread per query
__global__ void mix3_target_k(const float* __restrict__ obj, const float* __restrict__ qd, const float* __restrict__ qh,
                              const float* __restrict__ ent, const float* __restrict__ w, const int32_t* __restrict__ qinfo, int64_t Q, int D,
                              float gamma, float* __restrict__ tp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const float* __restrict__ o = obj + i * D;
  const float* __restrict__ q = qd + i * D;
  const float* __restrict__ h = qh + i * D;
  const float* __restrict__ e = ent + (int64_t)qinfo[i * 4] * D;
  float dist = 0.f, dot = 0.f, dot2 = 0.f;
  for (int c = 0; c < D; ++c) {
    const float ev = e[c];
    dist += fabsf(o[c] - ev);
    dot = __builtin_fmaf(q[c], ev, dot);
    dot2 = __builtin_fmaf(h[c], ev, dot2);
  }
  tp[i] = mix_prob3(dist, dot, dot2, gamma, w[0], w[1], w[2]).p;
}

template <int EPI, bool VEC4>
__global__ __launch_bounds__(256) void mix3_sweep_k(const Mix3Args a) {
  __shared__ __attribute__((aligned(16))) float so[MIX3_C][MIX3_T];
  __shared__ __attribute__((aligned(16))) float sq[MIX3_C][MIX3_T];
  __shared__ __attribute__((aligned(16))) float sh[MIX3_C][MIX3_T];
  __shared__ __attribute__((aligned(16))) float se[MIX3_C][MIX3_T];
  __shared__ unsigned long long smask[MIX3_T];
  __shared__ unsigned scnt[MIX3_T];
  __shared__ double sred[3][4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int col0 = blockIdx.x * MIX3_T;
  const int64_t row0 = (int64_t)blockIdx.y * MIX3_T;
  const int D = a.D;

  if (tid < MIX3_T) {                                        // the tile row's labels (filtered members) as bits
    unsigned long long m = 0ull;
    const int64_t row = row0 + tid;
    if (row < a.rows) {
      int lo, hi, when = 0;
      if constexpr (EPI == MIX3_RANK) {
        const int4 qi = *reinterpret_cast<const int4*>(a.qinfo + row * 4);
        lo = qi.y; hi = qi.z; when = qi.w;
      } else {
        const int2 q = *reinterpret_cast<const int2*>(a.qlist + row * 2);
        lo = q.x; hi = q.y;
      }
      if (lo < hi) {
        const int cbeg = a.e0 + col0, cend = cbeg + MIX3_T;
        int b = lo, e = hi;
        while (b < e) {                                      // first member >= cbeg
          const int mid = b + ((e - b) >> 1);
          if (a.list[mid] < cbeg) b = mid + 1; else e = mid;
        }
        for (; b < hi; ++b) {
          const int id = a.list[b];
          if (id >= cend) break;
          if constexpr (EPI == MIX3_RANK) { if (a.gone_at[b] > when) m |= 1ull << (id - cbeg); }
          else m |= 1ull << (id - cbeg);
        }
      }
    }
    smask[tid] = m;
  }

  // staging: thread (r = tid & 63, part = tid >> 6) carries row r of the four operands; per slice 8 of its 32 columns
  const int r = tid & 63, part = tid >> 6;
  const bool qok = row0 + r < a.rows, eok = col0 + r < a.ncols;
  const int64_t qoff = qok ? (row0 + r) * D : 0;
  const float* __restrict__ op = a.obj + qoff;
  const float* __restrict__ qp = a.qd + qoff;
  const float* __restrict__ hp = a.qh + qoff;
  const float* __restrict__ ep = a.ent + (eok ? (int64_t)(col0 + r) * D : 0);
  float po[8], pq[8], ph[8], pe[8];
  auto fetch = [&](int c0) {
    if constexpr (VEC4) {                                    // D % 4 == 0, 16-byte aligned rows: columns c .. c + 3
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = c0 + (part + 4 * h) * 4;
        float4 vo = make_float4(0.f, 0.f, 0.f, 0.f), vq = vo, vh = vo, ve = vo;
        if (c < D) {
          if (qok) {
            vo = *reinterpret_cast<const float4*>(op + c);
            vq = *reinterpret_cast<const float4*>(qp + c);
            vh = *reinterpret_cast<const float4*>(hp + c);
          }
          if (eok) ve = *reinterpret_cast<const float4*>(ep + c);
        }
        po[h * 4] = vo.x; po[h * 4 + 1] = vo.y; po[h * 4 + 2] = vo.z; po[h * 4 + 3] = vo.w;
        pq[h * 4] = vq.x; pq[h * 4 + 1] = vq.y; pq[h * 4 + 2] = vq.z; pq[h * 4 + 3] = vq.w;
        ph[h * 4] = vh.x; ph[h * 4 + 1] = vh.y; ph[h * 4 + 2] = vh.z; ph[h * 4 + 3] = vh.w;
        pe[h * 4] = ve.x; pe[h * 4 + 1] = ve.y; pe[h * 4 + 2] = ve.z; pe[h * 4 + 3] = ve.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = c0 + part + 4 * k;
        po[k] = (qok && c < D) ? op[c] : 0.f;
        pq[k] = (qok && c < D) ? qp[c] : 0.f;
        ph[k] = (qok && c < D) ? hp[c] : 0.f;
        pe[k] = (eok && c < D) ? ep[c] : 0.f;
      }
    }
  };
  auto stash = [&]() {                                       // lanes of a wave write 64 consecutive floats of one [c] row: conflict free
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = VEC4 ? (part + 4 * (k >> 2)) * 4 + (k & 3) : part + 4 * k;
      so[c][r] = po[k];
      sq[c][r] = pq[k];
      sh[c][r] = ph[k];
      se[c][r] = pe[k];
    }
  };

  float dist[4][4], dot[4][4], dot2[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) { dist[i][j] = 0.f; dot[i][j] = 0.f; dot2[i][j] = 0.f; }

  fetch(0);
  for (int c0 = 0; c0 < D; c0 += MIX3_C) {
    stash();
    __syncthreads();
    if (c0 + MIX3_C < D) fetch(c0 + MIX3_C);                 // the next slice travels while this one is consumed
    const int cn = D - c0 < MIX3_C ? D - c0 : MIX3_C;
#pragma unroll 4
    for (int c = 0; c < cn; ++c) {
      const float4 o = *reinterpret_cast<const float4*>(&so[c][ty * 4]);
      const float4 q = *reinterpret_cast<const float4*>(&sq[c][ty * 4]);
      const float4 h = *reinterpret_cast<const float4*>(&sh[c][ty * 4]);
      const float4 e = *reinterpret_cast<const float4*>(&se[c][tx * 4]);
      const float ov[4] = {o.x, o.y, o.z, o.w}, qv[4] = {q.x, q.y, q.z, q.w}, hv[4] = {h.x, h.y, h.z, h.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dist[i][j] += fabsf(ov[i] - ev[j]);
          dot[i][j] = __builtin_fmaf(qv[i], ev[j], dot[i][j]);
          dot2[i][j] = __builtin_fmaf(hv[i], ev[j], dot2[i][j]);
        }
    }
    __syncthreads();
  }

  // ---- epilogues: element (i, j) of the thread is (row0 + ty * 4 + i, col0 + tx * 4 + j) ----
  const float w0 = a.w[0], w1 = a.w[1], w2 = a.w[2];
  unsigned long long mrow[4];
  bool rok[4], cok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mrow[i] = smask[ty * 4 + i] >> (tx * 4);
    rok[i] = row0 + ty * 4 + i < a.rows;
    cok[i] = col0 + tx * 4 + i < a.ncols;
  }

  if constexpr (EPI == MIX3_LOSS) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float y = ((mrow[i] >> j) & 1ull) ? a.v_one : a.v_zero;
        const float p = mix_prob3(dist[i][j], dot[i][j], dot2[i][j], a.gamma, w0, w1, w2).p;
        const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
        const float t = (y - 1.f) * lq - y * lp;
        s += (rok[i] && cok[j]) ? (double)t : 0.0;
      }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) sred[0][tid >> 6] = s;
    __syncthreads();
    if (tid == 0) a.partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((sred[0][0] + sred[0][1]) + sred[0][2]) + sred[0][3];
  } else if constexpr (EPI == MIX3_GRAD) {
    const float gs = a.gscale[0];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t off = (row0 + ty * 4 + i) * a.ld + col0 + tx * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float y = ((mrow[i] >> j) & 1ull) ? a.v_one : a.v_zero;
        const MixP3 m = mix_prob3(dist[i][j], dot[i][j], dot2[i][j], a.gamma, w0, w1, w2);
        const float G = gs * (m.p - y) / fmaxf((1.f - m.p) * m.p, 1e-12f);
        const bool ok = rok[i] && cok[j];
        if (ok) {
          a.dl0[off + j] = (G * w0) * ((1.f - m.p0) * m.p0);
          a.dl1[off + j] = (G * w1) * ((1.f - m.p1) * m.p1);
          a.dl2[off + j] = (G * w2) * ((1.f - m.p2) * m.p2);
        }
        s0 += ok ? (double)(G * m.p0) : 0.0;
        s1 += ok ? (double)(G * m.p1) : 0.0;
        s2 += ok ? (double)(G * m.p2) : 0.0;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_xor(s0, off); s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
    if ((tid & 63) == 0) { sred[0][tid >> 6] = s0; sred[1][tid >> 6] = s1; sred[2][tid >> 6] = s2; }
    __syncthreads();
    if (tid < 3) a.partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + tid] = ((sred[tid][0] + sred[tid][1]) + sred[tid][2]) + sred[tid][3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = row0 + ty * 4 + i;
      const int64_t rc = rok[i] ? row : a.rows - 1;
      const float pt = a.tp[rc];
      const int tg = a.qinfo[rc * 4];
      unsigned n = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int id = a.e0 + col0 + tx * 4 + j;
        const float p = mix_prob3(dist[i][j], dot[i][j], dot2[i][j], a.gamma, w0, w1, w2).p;
        const bool hit = rok[i] && cok[j] && id != tg && !((mrow[i] >> j) & 1ull) && (p > pt || (p == pt && id < tg));
        n += hit ? 1u : 0u;
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) n += __shfl_xor(n, off);       // the 16 lanes tx of micro-tile row ty are consecutive
      if (tx == 0) scnt[ty * 4 + i] = n;
    }
    __syncthreads();
    if (tid < MIX3_T && row0 + tid < a.rows && scnt[tid]) atomicAdd(a.counts + row0 + tid, scnt[tid]);
  }
}

// dw[k] (+)= the n partials [n][3] of component k = blockIdx.x added in bce_finish_k's order; add != 0: added to what dw holds
__global__ __launch_bounds__(256) void mix3_dw_finish_k(const double* __restrict__ partial, int64_t n, int add, float* __restrict__ dw) {
  __shared__ double s[256];
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i * 3 + k];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) dw[k] = add ? dw[k] + (float)s[0] : (float)s[0];
}

inline SweepGrid mix3_grid(int64_t rows_all, int64_t c0, int64_t c1) { return SweepGrid{rows_all, c0, c1, MIX3_T, MIX3_T, RANK_CHUNK}; }

struct Mix3Plan { size_t qlist, partial, total; int64_t nparts; };
// ncols: the columns a call sweeps (N for the forward, c1 - c0 for the gradient); three float64 per workgroup (the gradient's three sums)
inline Mix3Plan mix3_bce_plan(int64_t B, int64_t ncols) {
  Mix3Plan p{};
  p.nparts = mix3_grid(B, 0, ncols).workgroups();
  size_t off = 256;                                          // slack: the workspace pointer is rounded up to 256 bytes
  p.qlist = off; off += sweep_up((size_t)B * 2 * sizeof(int32_t));
  p.partial = off; off += sweep_up((size_t)p.nparts * 3 * sizeof(double));
  p.total = off;
  return p;
}

struct Mix3RankPlan { size_t qinfo, tp, counts, total; };
inline Mix3RankPlan mix3_rank_plan(int64_t Q) {
  Mix3RankPlan p{};
  size_t off = 256;
  p.qinfo = off; off += sweep_up((size_t)Q * 4 * sizeof(int32_t));
  p.tp = off; off += sweep_up((size_t)Q * sizeof(float));
  p.counts = off; off += sweep_up((size_t)Q * sizeof(unsigned));
  p.total = off;
  return p;
}

// The sweep over the columns [c0, c1) of all rows on mix3_grid: column blocks of BCE_COLS outermost, row chunks of RANK_CHUNK inside.
// `all` carries what does not change from launch to launch; the launches append their partials at all.partial.
template <int EPI>
static int mix3_sweep(const Mix3Args& all, const float* obj, const float* qd, const float* qh, const float* ent, int64_t rows_all,
                      int64_t c0, int64_t c1, hipStream_t st) {
  const bool vec = all.D % 4 == 0 && aligned16(obj) && aligned16(qd) && aligned16(qh) && aligned16(ent);
  const SweepGrid sg = mix3_grid(rows_all, c0, c1);
  return sg.each([&](int64_t q0, int64_t rows, int64_t c, int64_t nc, int64_t wg0) {
    Mix3Args a = all;
    a.obj = obj + q0 * a.D; a.qd = qd + q0 * a.D; a.qh = qh + q0 * a.D; a.ent = ent + c * a.D; a.rows = rows; a.ncols = (int)nc; a.e0 = (int)c;
    if (EPI == MIX3_RANK) { a.qinfo = all.qinfo + q0 * 4; a.tp = all.tp + q0; a.counts = all.counts + q0; }
    else a.qlist = all.qlist + q0 * 2;
    if (EPI == MIX3_GRAD) {
      const int64_t o = q0 * a.ld + (c - c0);
      a.dl0 = all.dl0 + o; a.dl1 = all.dl1 + o; a.dl2 = all.dl2 + o; a.partial = all.partial + wg0 * 3;
    }
    if (EPI == MIX3_LOSS) a.partial = all.partial + wg0;
    const dim3 grid(sg.col_tiles(nc), sg.row_tiles(rows));
    if (vec) hipLaunchKernelGGL((mix3_sweep_k<EPI, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((mix3_sweep_k<EPI, false>), grid, dim3(256), 0, st, a);
    MRG_LAUNCH_CHECK();
    return (int)MRG_OK;
  });
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_sfmix3_bce_workspace_bytes(int64_t B, int64_t ncols, int D) {
  if (!sweep_shape_ok(B, ncols, D, false)) return MRG_E_SHAPE;
  return (int64_t)mix3_bce_plan(B, ncols).total;
}

// The body of both entry points from the label pointers on.  dl0 == NULL: the loss over the columns [0, N) = [c0, c1)
// (mrg_sfmix3_bce_fwd); else the gradients of the columns [c0, c1) (mrg_sfmix3_bce_grad).
static int mix3_bce_run(const float* obj, const float* qd, const float* qh, const float* ent, const float* w, const int64_t* qkey,
                        const int64_t* keys, const int32_t* rowptr, const int32_t* objs, int64_t U, float gamma, float v_zero, float v_one,
                        int64_t B, int64_t N, int D, int64_t c0, int64_t c1, float* loss, const float* gscale, float* dl0, float* dl1,
                        float* dl2, float* dw, void* ws, int64_t ws_bytes, void* stream) {
  if (!sweep_labels_ok(U, qkey, keys, rowptr, objs)) return MRG_E_NULLPTR;
  const Mix3Plan p = mix3_bce_plan(B, c1 - c0);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* wsb = sweep_ws_base(ws);
  int32_t* qlist = (int32_t*)(wsb + p.qlist);
  double* partial = (double*)(wsb + p.partial);
  int rc = sweep_launch_rows(bce_prep_k, B, st, qkey, keys, rowptr, U, B, qlist);
  if (rc != MRG_OK) return rc;
  Mix3Args a{};
  a.D = D; a.w = w; a.gamma = gamma; a.qlist = qlist; a.list = objs; a.v_zero = v_zero; a.v_one = v_one; a.partial = partial;
  if (dl0) {
    a.gscale = gscale; a.dl0 = dl0; a.dl1 = dl1; a.dl2 = dl2; a.ld = c1 - c0;
    rc = mix3_sweep<MIX3_GRAD>(a, obj, qd, qh, ent, B, c0, c1, st);
    if (rc != MRG_OK) return rc;
    hipLaunchKernelGGL(mix3_dw_finish_k, dim3(3), dim3(256), 0, st, partial, p.nparts, c0 > 0 ? 1 : 0, dw);
    MRG_LAUNCH_CHECK();
    return MRG_OK;
  }
  rc = mix3_sweep<MIX3_LOSS>(a, obj, qd, qh, ent, B, c0, c1, st);
  if (rc != MRG_OK) return rc;
  return sweep_launch_rows(bce_finish_k, 1, st, partial, p.nparts, 1.0 / ((double)B * (double)N), loss);
}

extern "C" int mrg_sfmix3_bce_fwd(const float* obj, const float* qd, const float* qh, const float* ent, const float* w, const int64_t* qkey,
                                  const int64_t* keys, const int32_t* rowptr, const int32_t* objs, int64_t U, float gamma, float v_zero,
                                  float v_one, int64_t B, int64_t N, int D, float* loss, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, false)) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!obj || !qd || !qh || !ent || !w || !loss) return MRG_E_NULLPTR;
  return mix3_bce_run(obj, qd, qh, ent, w, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, 0, N, loss, nullptr, nullptr, nullptr,
                      nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int mrg_sfmix3_bce_grad(const float* obj, const float* qd, const float* qh, const float* ent, const float* w, const int64_t* qkey,
                                   const int64_t* keys, const int32_t* rowptr, const int32_t* objs, int64_t U, float gamma, float v_zero,
                                   float v_one, int64_t B, int64_t N, int D, int64_t c0, int64_t c1, const float* gscale, float* dl0,
                                   float* dl1, float* dl2, float* dw, void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(B, N, D, false) || c0 < 0 || c1 <= c0 || c1 > N) return MRG_E_SHAPE;
  if (B == 0) return MRG_OK;
  if (!obj || !qd || !qh || !ent || !w || !gscale || !dl0 || !dl1 || !dl2 || !dw) return MRG_E_NULLPTR;
  return mix3_bce_run(obj, qd, qh, ent, w, qkey, keys, rowptr, objs, U, gamma, v_zero, v_one, B, N, D, c0, c1, nullptr, gscale, dl0, dl1, dl2,
                      dw, ws, ws_bytes, stream);
}

extern "C" int64_t mrg_sfmix3_rank_workspace_bytes(int64_t Q, int64_t N, int D) {
  if (!sweep_shape_ok(Q, N, D, false)) return MRG_E_SHAPE;
  return (int64_t)mix3_rank_plan(Q).total;
}

extern "C" int mrg_sfmix3_rank(const float* obj, const float* qd, const float* qh, const float* ent, const float* w, float gamma,
                               const int32_t* t_idx, const int64_t* qkey, const int32_t* when, const int64_t* keys, const int32_t* rowptr,
                               const int32_t* members, const int32_t* gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t* ranks,
                               void* ws, int64_t ws_bytes, void* stream) {
  if (U < 0 || !sweep_shape_ok(Q, N, D, false)) return MRG_E_SHAPE;
  if (Q == 0) return MRG_OK;
  if (!obj || !qd || !qh || !ent || !w || !t_idx || !ranks) return MRG_E_NULLPTR;
  if (!sweep_labels_ok(U, qkey, when, keys, rowptr, members, gone_at)) return MRG_E_NULLPTR;
  const Mix3RankPlan p = mix3_rank_plan(Q);
  if (!ws || ws_bytes < (int64_t)p.total) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* wsb = sweep_ws_base(ws);
  int32_t* qinfo = (int32_t*)(wsb + p.qinfo);
  float* tp = (float*)(wsb + p.tp);
  unsigned* counts = (unsigned*)(wsb + p.counts);
  int rc = sweep_launch_rows(rank_prep_k, Q, st, t_idx, qkey, when, keys, rowptr, U, Q, qinfo, counts);
  if (rc != MRG_OK) return rc;
  rc = sweep_launch_rows(mix3_target_k, Q, st, obj, qd, qh, ent, w, qinfo, Q, D, gamma, tp);
  if (rc != MRG_OK) return rc;
  Mix3Args a{};
  a.D = D; a.w = w; a.gamma = gamma; a.qinfo = qinfo; a.list = members; a.gone_at = gone_at; a.tp = tp; a.counts = counts;
  rc = mix3_sweep<MIX3_RANK>(a, obj, qd, qh, ent, Q, 0, N, st);
  if (rc != MRG_OK) return rc;
  return sweep_launch_rows(rank_finish_k, Q, st, counts, ranks, Q);
}
