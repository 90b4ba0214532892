// MixedOp epilogue:  out = sum_k w_k * ReLU(BatchNorm_k(y_k))  over K operator outputs y_k [rows, D]
//   reference models/cell_lp.py:25-33 (MixedOp.forward / op_forward) with nn.BatchNorm1d in
//   training mode (:21) -- in the reference 3 ATen launches per branch + the weighted sum,
//   each a full pass over [rows, D], and as many again in backward.
// Here: one statistics pass (column sums in float64, deterministic two-stage reduction), one
// combine pass (reads every y_k once, writes out once), and in backward one reduction pass
// and one apply pass.  A NULL branch pointer stands for an all-zero operator output (f_zero).
// HBM-bound: algorithmic bytes  stats 4*D*rows*Kt,  fwd 4*D*rows*(Kt+1),
// bwd-reduce 4*D*rows*(Kt+1),  bwd-apply 4*D*rows*(2*Kt+1)   (Kt = non-NULL branches).
#include "mixedop_parts.hpp"

namespace mrg {

// optional per-candidate row scale applied to the candidate's output gradient as it is written (mix_bwd_apply_k):
// gy_k[r] *= r < edge_rows[k] ? scale[k] * (rs[k] ? rs[k][r] : 1) : self_scale[k]      when on[k]
// on[k] == 2: the gated form (f_dense_comp, mrg_dense_filter_dz kind 0): with gc = gy * c, the candidate's gradient buffer receives
// dz = gc * s * gate * (1 - gate) and gs_out[k] the direct term gc * gate of the gradient w.r.t. s.
// add_from[k] (gated candidates only, -1 = none): the index of ANOTHER candidate whose own gradient gy is ADDED to gs_out[k] instead
// of being stored -- f_identity of the same MixedOp: its output IS the operand s of candidate k, so both are gradients w.r.t. the
// same rows and the state's fan-in sum would add them anyway (one [rows, D] write here and one read there less).
// full[k] (optional): the same multiplier expanded over ALL rows by the caller -- loaded with the candidates' rows at the top of the
// trip instead of conditionally (edge rows only) between the arithmetic and the stores, where its latency was exposed.
struct RowScalePack { const float* rs[MRG_MIX_MAXK]; float scale[MRG_MIX_MAXK]; float self_scale[MRG_MIX_MAXK]; int64_t edge_rows[MRG_MIX_MAXK]; int on[MRG_MIX_MAXK];
                      const float* full[MRG_MIX_MAXK];
                      const float* s[MRG_MIX_MAXK]; const float* gate[MRG_MIX_MAXK]; float* gs_out[MRG_MIX_MAXK]; int add_from[MRG_MIX_MAXK]; };

// A gated candidate that is never stored (f_dense_comp, reference models/operations_lp.py:356-390): ys.p[k] holds its GATE
// sigmoid(W [s ; s_in] + b) and the candidate's value is recomputed here as  gate * s * c_r  -- the expression, and its order, of
// the row GEMM's gate epilogue (gemm.hpp EPI_GATE: g * in * cs), so every statistic, the output and every gradient are the
// stored form's bit for bit.  The gate is needed by the candidate's backward anyway; its [rows, D] output is one write (GEMM) and
// four reads (statistics, combine, backward reduction, backward apply) that do not happen; s is the MixedOp's input state, which
// the f_identity candidate of the same MixedOp reads at the same place (one L2 / L1 hit more, no HBM pass).   k < 0: none.
struct GatedPack { int k; const float* s; const float* c;
                   int pair_k;      // pair_k: the candidate whose stored output is s itself (f_identity), -1 = none  (statistics kernel)
                   // the row-scaled candidate (f_sparse_op_comp, never stored either): y = s * rf[r]; ys.p[rk] == s.   rk < 0: none
                   int rk; const float* rf;
                   // ... its backward (mix_bwd_apply_k only): rh[r] = d pre-activation / d row dot, the collapsed gate vectors
                   // uvc[seg][uld] of the three direction segments [0, b0) [b0, b1) [b1, rows), rdq[r] out (the gradient w.r.t. rf[r])
                   const float* rh; const float* uvc; int uld; int64_t b0, b1; float* rdq;
                   // mrg_gated_branch.valid_rows (static step graphs): the number of VALID rows lives in device memory; rows at
                   // and beyond it are capacity padding -- left out of every statistic, written as zeros by the passes that write
                   const int32_t* vrows;
                   // the activation behind the BatchNorm: 0 = ReLU (every MixedOp of the search space), 1 = tanh (CompGraphConv's tail,
                   // reference models/compgcn.py:100-111).  A template parameter of the three kernels that apply it (a run-time branch
                   // cost mix_bwd_apply_k 14 %); the tanh instances exist for un-gated launches of at most five candidates.
                   int act; };

// c: the candidate's per-row multiplier for ALL rows (the caller expands scale_edge * norm on edge rows, scale_self on self rows,
// once per graph): an unconditional load.  A conditional one (edge rows only) was compiled into an exec-masked block that waited for
// it -- s_waitcnt vmcnt(0) -- before the candidates' loads were issued: two dependent memory latencies per trip.
// (A function on purpose: with gp.c[r] written out at the call sites gp is no longer passed by reference anywhere, and the compiler
// emits other code for mix_fwd_k / mix_colstats_k / mix_bwd_reduce_k -- profiles/mixedop_split_asm.txt.)
__device__ __forceinline__ float gated_rowscale(const GatedPack& gp, int64_t r) { return gp.c[r]; }

// ---- column statistics: sums[k][0][c] = sum_r y_k[r][c], sums[k][1][c] = sum_r y_k[r][c]^2 (float64)
// block reduction of one candidate's per-lane column sums into its per-block partial [2][D] (every thread of the block calls it)
template <int VEC, int LPR, int KMAX>
__device__ __forceinline__ void colstats_flush(const double (&s1)[KMAX][VEC], const double (&s2)[KMAX][VEC], double* red, double* __restrict__ dst,
                                               int D, int sl, int rw) {
  constexpr int RPB = MRG_BLOCK / LPR;
  constexpr int WIDTH = LPR * KMAX * VEC;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < KMAX; ++q) {
    int c = sl + q * LPR;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      red[(rw * 2 + 0) * WIDTH + c * VEC + j] = s1[q][j];
      red[(rw * 2 + 1) * WIDTH + c * VEC + j] = s2[q][j];
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * D; t += MRG_BLOCK) {
    int which = t / D, c = t - which * D;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < RPB; ++q) acc += red[(q * 2 + which) * WIDTH + c];
    dst[t] = acc;
  }
}

// GATED: candidate gp.k is recomputed from its gate and candidate gp.rk from its row factor (GatedPack); with gp.pair_k >= 0 --
// f_identity of the same MixedOp, whose output IS the multiplicand s -- up to three candidates are functions of the same rows s
// and share ONE sweep (s is read once for all; a sweep per candidate would read it from HBM each time, the tensors being far
// larger than the caches).  Each candidate's sums see the same values in the same order as a sweep of its own.
template <int VEC, int LPR, int KMAX, bool GATED>
__global__ __launch_bounds__(MRG_BLOCK) void mix_colstats_k(PtrPack ys, int K, int64_t rows, int D, double* __restrict__ ws, GatedPack gp) {
  rows = valid_rows(gp.vrows, rows);                        // capacity padding is not part of any statistic
  constexpr int RPB = MRG_BLOCK / LPR;
  constexpr int WIDTH = LPR * KMAX * VEC;
  __shared__ double red[RPB * 2 * WIDTH];
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dv = D / VEC;
  const int64_t step = (int64_t)gridDim.x * RPB;
  int first = MRG_MIX_MAXK;                                // the shared sweep runs at the first of its candidates
  if (GATED) {
    if (gp.k >= 0 && gp.k < first) first = gp.k;
    if (gp.pair_k >= 0 && gp.pair_k < first) first = gp.pair_k;
    if (gp.rk >= 0 && gp.rk < first) first = gp.rk;
  }
  for (int k = 0; k < K; ++k) {
    const float* __restrict__ y = ys.p[k];
    const bool shared = GATED && (k == gp.k || k == gp.pair_k || k == gp.rk);
    if (shared && k != first) continue;
    double s1[KMAX][VEC], s2[KMAX][VEC];
#pragma unroll
    for (int q = 0; q < KMAX; ++q)
#pragma unroll
      for (int j = 0; j < VEC; ++j) { s1[q][j] = 0.0; s2[q][j] = 0.0; }
    if (shared) {
      // s1 / s2: s itself (candidate pair_k); t1 / t2: gate * s * c_r (candidate gp.k); u1 / u2: s * f_r (candidate gp.rk)
      const float* __restrict__ gate = gp.k >= 0 ? ys.p[gp.k] : gp.s;
      double t1[KMAX][VEC], t2[KMAX][VEC], u1[KMAX][VEC], u2[KMAX][VEC];
#pragma unroll
      for (int q = 0; q < KMAX; ++q)
#pragma unroll
        for (int j = 0; j < VEC; ++j) { t1[q][j] = 0.0; t2[q][j] = 0.0; u1[q][j] = 0.0; u2[q][j] = 0.0; }
      int64_t r = (int64_t)blockIdx.x * RPB + rw;
      for (; r + step < rows; r += 2 * step) {              // two rows per trip: four independent 16-byte loads in flight per lane
        const float ck0 = gated_rowscale(gp, r), ck1 = gated_rowscale(gp, r + step);
        const float rf0 = gp.rf[r], rf1 = gp.rf[r + step];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
          int c = sl + q * LPR;
          if (c < dv) {
            const Vec<VEC> sv0 = Vec<VEC>::load(gp.s + r * D + c * VEC), sv1 = Vec<VEC>::load(gp.s + (r + step) * D + c * VEC);
            const Vec<VEC> ga0 = Vec<VEC>::load(gate + r * D + c * VEC), ga1 = Vec<VEC>::load(gate + (r + step) * D + c * VEC);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              double d = (double)sv0[j]; s1[q][j] += d; s2[q][j] += d * d;
              d = (double)sv1[j]; s1[q][j] += d; s2[q][j] += d * d;
              d = (double)(ga0[j] * sv0[j] * ck0); t1[q][j] += d; t2[q][j] += d * d;
              d = (double)(ga1[j] * sv1[j] * ck1); t1[q][j] += d; t2[q][j] += d * d;
              d = (double)(sv0[j] * rf0); u1[q][j] += d; u2[q][j] += d * d;
              d = (double)(sv1[j] * rf1); u1[q][j] += d; u2[q][j] += d * d;
            }
          }
        }
      }
      for (; r < rows; r += step) {
        const float ck = gated_rowscale(gp, r), rf = gp.rf[r];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
          int c = sl + q * LPR;
          if (c < dv) {
            const Vec<VEC> sv = Vec<VEC>::load(gp.s + r * D + c * VEC), ga = Vec<VEC>::load(gate + r * D + c * VEC);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              double d = (double)sv[j]; s1[q][j] += d; s2[q][j] += d * d;
              d = (double)(ga[j] * sv[j] * ck); t1[q][j] += d; t2[q][j] += d * d;
              d = (double)(sv[j] * rf); u1[q][j] += d; u2[q][j] += d * d;
            }
          }
        }
      }
      if (gp.k >= 0) colstats_flush<VEC, LPR, KMAX>(t1, t2, red, ws + ((int64_t)blockIdx.x * K + gp.k) * 2 * D, D, sl, rw);
      if (gp.pair_k >= 0) colstats_flush<VEC, LPR, KMAX>(s1, s2, red, ws + ((int64_t)blockIdx.x * K + gp.pair_k) * 2 * D, D, sl, rw);
      if (gp.rk >= 0) colstats_flush<VEC, LPR, KMAX>(u1, u2, red, ws + ((int64_t)blockIdx.x * K + gp.rk) * 2 * D, D, sl, rw);
      continue;
    }
    if (y != nullptr) {
      // four rows per trip: four independent loads in flight per lane (one load per trip left HBM latency exposed)
      int64_t r = (int64_t)blockIdx.x * RPB + rw;
      for (; r + 3 * step < rows; r += 4 * step) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
          int c = sl + q * LPR;
          if (c < dv) {
            Vec<VEC> v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = Vec<VEC>::load(y + (r + u * step) * D + c * VEC);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int j = 0; j < VEC; ++j) { double d = (double)v[u][j]; s1[q][j] += d; s2[q][j] += d * d; }
          }
        }
      }
      for (; r < rows; r += step) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
          int c = sl + q * LPR;
          if (c < dv) {
            Vec<VEC> v = Vec<VEC>::load(y + r * D + c * VEC);
#pragma unroll
            for (int j = 0; j < VEC; ++j) { double d = (double)v[j]; s1[q][j] += d; s2[q][j] += d * d; }
          }
        }
      }
    }
    colstats_flush<VEC, LPR, KMAX>(s1, s2, red, ws + ((int64_t)blockIdx.x * K + k) * 2 * D, D, sl, rw);
  }
}

// ---- statistics that a candidate's PRODUCER formed (mrg_gated_branch.given): no sweep over the candidate ------------------------
// The producer (the row GEMM's gate / scale epilogue, gate_row_fwd_colsum_k) left n partial [2][D] float64 sums, `stride` doubles
// apart.  Block (b, k) of a G x K grid adds candidate k's partials [n b / G, n (b + 1) / G) in order (four interleaved
// accumulators, fixed association) into ws[b][k][2][D] -- the layout mix_colstats_k's blocks write, so mix_reduce_finalize_fwd_k
// finishes both alike.  zero_absent: no statistics kernel ran; the slots of candidates without given sums (all-zero
// candidates) are zeroed here.
struct GivenPack { const double* p[MRG_MIX_MAXK]; int n[MRG_MIX_MAXK]; int64_t stride[MRG_MIX_MAXK]; };

__global__ __launch_bounds__(MRG_BLOCK) void mix_given_reduce_k(GivenPack gv, int K, int D, double* __restrict__ ws, int zero_absent) {
  const int b = blockIdx.x, k = blockIdx.y, G = gridDim.x;
  double* __restrict__ dst = ws + ((int64_t)b * K + k) * 2 * D;
  const double* __restrict__ src = gv.p[k];
  if (src == nullptr) {
    if (zero_absent)
      for (int t = threadIdx.x; t < 2 * D; t += MRG_BLOCK) dst[t] = 0.0;
    return;
  }
  const int64_t n = gv.n[k], stride = gv.stride[k];
  const int64_t lo = n * b / G, hi = n * (b + 1) / G;
  for (int t = threadIdx.x; t < 2 * D; t += MRG_BLOCK) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t i = lo;
    for (; i + 3 < hi; i += 4) {
      const double v0 = src[i * stride + t], v1 = src[(i + 1) * stride + t], v2 = src[(i + 2) * stride + t], v3 = src[(i + 3) * stride + t];
      a0 += v0; a1 += v1; a2 += v2; a3 += v3;
    }
    for (; i < hi; ++i) a0 += src[i * stride + t];
    dst[t] = (a0 + a1) + (a2 + a3);
  }
}

// ---- finalize forward: statistics -> per-column coefficients, running-stat update
// coef[k][0]=scale=gamma*invstd, [1]=shift=beta-mean*scale, [2]=invstd, [3]=mean*invstd
__global__ void mix_finalize_fwd_k(const double* __restrict__ sums, PtrPack gamma, PtrPack beta, MutPack rmean, MutPack rvar,
                                   int K, double total_rows, int D, float eps, float momentum, float* __restrict__ coef,
                                   const int32_t* __restrict__ vrows) {
  if (vrows) total_rows = *vrows > 0 ? (double)*vrows : 1.0;
  int k = blockIdx.y;
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D || k >= K) return;
  double mean = sums[(k * 2 + 0) * D + c] / total_rows;
  double var = sums[(k * 2 + 1) * D + c] / total_rows - mean * mean;
  if (var < 0) var = 0;
  double invstd = 1.0 / sqrt(var + (double)eps);
  float g = gamma.p[k] ? gamma.p[k][c] : 1.f, b = beta.p[k] ? beta.p[k][c] : 0.f;
  float* o = coef + (int64_t)k * 4 * D;
  o[c] = (float)(g * invstd);
  o[D + c] = (float)(b - mean * g * invstd);
  o[2 * D + c] = (float)invstd;
  o[3 * D + c] = (float)(mean * invstd);
  if (rmean.p[k]) {
    double unbiased = total_rows > 1 ? var * (total_rows / (total_rows - 1.0)) : var;
    rmean.p[k][c] = (1.f - momentum) * rmean.p[k][c] + momentum * (float)mean;
    rvar.p[k][c] = (1.f - momentum) * rvar.p[k][c] + momentum * (float)unbiased;
  }
}

// The ordered reduction of the per-block statistics and the finalize step in ONE launch (single-GPU path: no all-reduce sits
// between them): a 64 x 16 block owns 64 columns of one candidate, reduces their sum and sum of squares over the nb partial
// rows exactly like ordered_reduce_k and turns them into the coefficients.  Bit-identical to the two-launch form.
__global__ void mix_reduce_finalize_fwd_k(const double* __restrict__ ws, int nb, PtrPack gamma, PtrPack beta, MutPack rmean, MutPack rvar,
                                          int K, double total_rows, int D, float eps, float momentum, float* __restrict__ coef,
                                          const int32_t* __restrict__ vrows) {
  if (vrows) total_rows = *vrows > 0 ? (double)*vrows : 1.0;
  __shared__ double part[2][16][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx, k = blockIdx.y;
  const int ld = K * 2 * D;
#pragma unroll
  for (int j = 0; j < 2; ++j) part[j][ty][tx] = c < D ? ordered_partial<double>(ws, 0, nb, ld, (k * 2 + j) * D + c, ty) : 0.0;
  __syncthreads();
  if (ty != 0 || c >= D) return;
  double tot[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double t = part[j][0][tx];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += part[j][i][tx];
    tot[j] = t;
  }
  double mean = tot[0] / total_rows;
  double var = tot[1] / total_rows - mean * mean;
  if (var < 0) var = 0;
  double invstd = 1.0 / sqrt(var + (double)eps);
  float g = gamma.p[k] ? gamma.p[k][c] : 1.f, b = beta.p[k] ? beta.p[k][c] : 0.f;
  float* o = coef + (int64_t)k * 4 * D;
  o[c] = (float)(g * invstd);
  o[D + c] = (float)(b - mean * g * invstd);
  o[2 * D + c] = (float)invstd;
  o[3 * D + c] = (float)(mean * invstd);
  if (rmean.p[k]) {
    double unbiased = total_rows > 1 ? var * (total_rows / (total_rows - 1.0)) : var;
    rmean.p[k][c] = (1.f - momentum) * rmean.p[k][c] + momentum * (float)mean;
    rvar.p[k][c] = (1.f - momentum) * rvar.p[k][c] + momentum * (float)unbiased;
  }
}

// ---- forward combine
// KB: the candidate slots the kernel is unrolled for (K <= KB): 5 covers every MixedOp of the search space (3, 4 or 5 candidates)
// with 3/8 fewer registers than the general 8 -- one more wave per SIMD.
template <int VEC, int LPR, int KMAX, bool GATED, int KB, int ACT = 0>
__global__ __launch_bounds__(MRG_BLOCK) void mix_fwd_k(PtrPack ys, int K, const float* __restrict__ coef, const float* __restrict__ w,
                                                       float* __restrict__ out, int64_t rows, int D,
                                                       const float* __restrict__ addend, GatedPack gp) {
  extern __shared__ float lds[];                 // [K][2][D] scale, shift
  constexpr int RPB = MRG_BLOCK / LPR;
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dv = D / VEC;
  for (int t = threadIdx.x; t < K * 2 * D; t += MRG_BLOCK) {
    int k = t / (2 * D), rem = t - k * 2 * D;
    lds[t] = coef[(int64_t)k * 4 * D + rem];
  }
  __syncthreads();
  float wk[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) wk[k] = k < K ? w[k] : 0.f;
  const int64_t nvalid = valid_rows(gp.vrows, rows);
  for (int64_t r = (int64_t)blockIdx.x * RPB + rw; r < rows; r += (int64_t)gridDim.x * RPB) {
    const bool pad = r >= nvalid;                            // capacity padding: the state keeps zero rows there
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
      int c = sl + q * LPR;
      if (c < dv) {
        // `addend`: the output of the MixedOp this one is summed with (reference models/cell_lp.py:104-113: sum of the
        // MixedOps feeding a state) -- added here instead of by a separate full-size kernel
        Vec<VEC> acc = addend ? Vec<VEC>::load(addend + r * D + c * VEC) : Vec<VEC>::fill(0.f);
        // the recomputed candidate's row scale and multiplicand: issued FIRST (loads return in order: the candidates before
        // it can be consumed while the later loads are in flight).  The candidates that ARE s (f_identity, the row-scaled one) still
        // load it themselves: the repeated addresses hit in L1, and taking them from gsv by a select was measured slower (lab: 413 vs
        // 409 us, backward reduction 482 vs 425 us) and let the compiler re-associate the products (1-ulp differences)
        float gck = 1.f, rfv = 1.f;
        Vec<VEC> gsv = Vec<VEC>::fill(0.f);
        if constexpr (GATED) {
          gck = gated_rowscale(gp, r);
          rfv = gp.rf[r];
          gsv = Vec<VEC>::load(gp.s + r * D + c * VEC);
        }
        // phase 1: every branch's load is issued before any is used (a load consumed inside its own `if (k < K)`
        // block leaves one 16-byte load in flight per lane)
        Vec<VEC> vin[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          vin[k] = Vec<VEC>::fill(0.f);
          if (k < K && ys.p[k]) vin[k] = Vec<VEC>::load(ys.p[k] + r * D + c * VEC);
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          if (k < K) {
            Vec<VEC> v = vin[k];
            if constexpr (GATED) {                         // the recomputed candidates: gate -> gate * s * c_r, s -> s * 1 * f_r; the others * 1 * 1
              const bool isg = k == gp.k;                  // (selects, not a branch: the loads above stay in flight together)
              const float cm = isg ? gck : (k == gp.rk ? rfv : 1.0f);
#pragma unroll
              for (int j = 0; j < VEC; ++j) v[j] = v[j] * (isg ? gsv[j] : 1.0f) * cm;
            }
            Vec<VEC> sc = Vec<VEC>::load(lds + (k * 2 + 0) * D + c * VEC), sh = Vec<VEC>::load(lds + (k * 2 + 1) * D + c * VEC);
            if constexpr (ACT == 0) {
#pragma unroll
              for (int j = 0; j < VEC; ++j) {
                float z = v[j] * sc[j] + sh[j];
                acc[j] += wk[k] * (z > 0.f ? z : 0.f);
              }
            } else {
#pragma unroll
              for (int j = 0; j < VEC; ++j) acc[j] += wk[k] * tanhf(v[j] * sc[j] + sh[j]);
            }
          }
        }
        if (pad) acc = Vec<VEC>::fill(0.f);
        acc.store(out + r * D + c * VEC);
      }
    }
  }
}

// ---- backward reduce: per branch  red[k][0] = sum gr, [1] = sum gr*xhat, [2] = sum g*relu(z)  (gr = w g [z>0])
// rows outermost: g is read once, every y_k once; per-branch column accumulators live in registers.
template <int VEC, int LPR, int KMAX, int KB, bool GATED, int ACT = 0>
__global__ __launch_bounds__(MRG_BLOCK) void mix_bwd_reduce_k(const float* __restrict__ g, PtrPack ys, int K,
                                                              const float* __restrict__ coef, const float* __restrict__ w,
                                                              float* __restrict__ ws, int64_t rows, int D, GatedPack gp) {
  rows = valid_rows(gp.vrows, rows);
  extern __shared__ float lds[];                 // coef [K][4][D], then the block-reduction buffer
  constexpr int RPB = MRG_BLOCK / LPR;
  constexpr int WIDTH = LPR * KMAX * VEC;
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dv = D / VEC;
  float* red = lds + K * 4 * D;                  // [RPB][3][WIDTH]
  for (int t = threadIdx.x; t < K * 4 * D; t += MRG_BLOCK) lds[t] = coef[t];
  __syncthreads();
  float wk[KB];
  Vec<VEC> a0[KB][KMAX], a1[KB][KMAX], a2[KB][KMAX];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    wk[k] = k < K ? w[k] : 0.f;
#pragma unroll
    for (int q = 0; q < KMAX; ++q) { a0[k][q] = Vec<VEC>::fill(0.f); a1[k][q] = Vec<VEC>::fill(0.f); a2[k][q] = Vec<VEC>::fill(0.f); }
  }
  for (int64_t r = (int64_t)blockIdx.x * RPB + rw; r < rows; r += (int64_t)gridDim.x * RPB) {
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
      int c = sl + q * LPR;
      if (c < dv) {
        float gck = 1.f, rfv = 1.f;                        // the recomputed candidates' row multipliers and multiplicand (see mix_fwd_k)
        Vec<VEC> gsv = Vec<VEC>::fill(0.f);
        if constexpr (GATED) {
          gck = gated_rowscale(gp, r);
          rfv = gp.rf[r];
          gsv = Vec<VEC>::load(gp.s + r * D + c * VEC);
        }
        Vec<VEC> gv = Vec<VEC>::load(g + r * D + c * VEC);
        Vec<VEC> vin[KB];                                  // all loads first (see mix_fwd_k)
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          vin[k] = Vec<VEC>::fill(0.f);
          if (k < K && ys.p[k]) vin[k] = Vec<VEC>::load(ys.p[k] + r * D + c * VEC);
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          if (k < K) {
            Vec<VEC> v = vin[k];
            if constexpr (GATED) {                         // the recomputed candidates: gate -> gate * s * c_r, s -> s * 1 * f_r; the others * 1 * 1
              const bool isg = k == gp.k;
              const float cm = isg ? gck : (k == gp.rk ? rfv : 1.0f);
#pragma unroll
              for (int j = 0; j < VEC; ++j) v[j] = v[j] * (isg ? gsv[j] : 1.0f) * cm;
            }
            const float* cf = lds + k * 4 * D + c * VEC;
            const Vec<VEC> c0 = Vec<VEC>::load(cf), c1 = Vec<VEC>::load(cf + D), c2 = Vec<VEC>::load(cf + 2 * D), c3 = Vec<VEC>::load(cf + 3 * D);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              float z = v[j] * c0[j] + c1[j];
              float xh = v[j] * c2[j] - c3[j];
              float rl, gr;
              if constexpr (ACT == 0) { rl = z > 0.f ? z : 0.f; gr = z > 0.f ? wk[k] * gv[j] : 0.f; }
              else { rl = tanhf(z); gr = wk[k] * gv[j] * (1.f - rl * rl); }
              a0[k][q][j] += gr;
              a1[k][q][j] += gr * xh;
              a2[k][q][j] += gv[j] * rl;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    if (k < K) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        int c = sl + q * LPR;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          red[(rw * 3 + 0) * WIDTH + c * VEC + j] = a0[k][q][j];
          red[(rw * 3 + 1) * WIDTH + c * VEC + j] = a1[k][q][j];
          red[(rw * 3 + 2) * WIDTH + c * VEC + j] = a2[k][q][j];
        }
      }
      __syncthreads();
      float* dst = ws + ((int64_t)blockIdx.x * K + k) * 3 * D;
      for (int t = threadIdx.x; t < 3 * D; t += MRG_BLOCK) {
        int which = t / D, c = t - which * D;
        float acc = 0.f;
#pragma unroll
        for (int q2 = 0; q2 < RPB; ++q2) acc += red[(q2 * 3 + which) * WIDTH + c];
        dst[t] = acc;
      }
    }
  }
}

// ---- finalize backward: red[k][3][D] -> c1 = sum gr / rows, c2 = sum gr*xhat / rows into coef2[k][2][D];
//      dgamma_k = sum gr*xhat, dbeta_k = sum gr, dw[k] = sum_c sum g*relu(z)
__global__ void mix_finalize_bwd_k(const float* __restrict__ red, int K, double total_rows, int D, float* __restrict__ coef2,
                                   MutPack dgamma, MutPack dbeta, float* __restrict__ dw, const int32_t* __restrict__ vrows) {
  if (vrows) total_rows = *vrows > 0 ? (double)*vrows : 1.0;
  __shared__ float part[256];
  int k = blockIdx.x;
  float accw = 0.f;
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    float s0 = red[(k * 3 + 0) * D + c], s1 = red[(k * 3 + 1) * D + c];
    coef2[(k * 2 + 0) * D + c] = (float)(s0 / total_rows);
    coef2[(k * 2 + 1) * D + c] = (float)(s1 / total_rows);
    if (dgamma.p[k]) dgamma.p[k][c] = s1;
    if (dbeta.p[k]) dbeta.p[k][c] = s0;
    accw += red[(k * 3 + 2) * D + c];
  }
  part[threadIdx.x] = accw;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < (int)blockDim.x; ++i) tot += part[i];
    dw[k] = tot;
  }
}

// ---- backward apply: gy_k = (gr - c1 - xhat*c2) * scale      (skipped where gy_k is NULL)
// The row-scaled candidate gp.rk (f_sparse_op_comp, y = s * f_r with f_r = sigmoid(u.s + v.s_in + c0) * t_r) has no gradient
// tensor of its own: with gy its gradient w.r.t. y, this kernel forms the row dot q_r = sum_c gy * s (the lanes of the
// row, same order as gate_bwd_k) -> rdq[r], the gradient w.r.t. f_r, from which mrg_gate_row_bwd derives the candidate's
// parameter / s_in gradients; and with dz_r = q_r * h_r (h_r = t_r * gate * (1 - gate), saved by the forward) it ADDS the candidate's
// whole gradient w.r.t. s, gy * f_r + dz_r * u[c], into the gated candidate's direct term gs_out (gradients w.r.t. the same rows s).
//
// ROLES.  The launcher knows before the launch what each candidate is, and hands the kernel one field per role instead of
// per-candidate arrays that the row loop indexes (1056 bytes of by-value packs against 102 scalar registers per wave: 153 to 759
// spilled SGPRs per instance, read back through v_readlane on every row -- profiles/mix_apply_asm.txt):
//   gated  the recomputed candidate (ys holds its GATE, its value is gate * s * c_r) whose folded store writes dz and gs_out,
//   row    the row-scaled candidate (value s * f_r; no gradient tensor: rdq and a term of gs_out),
//   add    the candidate whose output IS s (f_identity) and whose gradient is added into gs_out instead of being stored,
//   other  a stored candidate: gy_k, times a full-row multiplier where one is folded in.
// Which roles exist is a property of the instance: the row loop has no branch or select on a role.  All three s-valued roles take s
// from ONE load.  Anything else (more than five candidates, the edge/self form of a row scale, a stored gated candidate, ...)
// runs on mix_bwd_apply_any_k below.
//
// ROUNDING.  Every expression is the one the by-index kernel compiled to, spelled out: which products are fused into an fma and
// which are rounded on their own is part of the results (tests/golden/mix_apply_*.npz pin them), so contraction is OFF in
// these functions and the fused ones are written as __builtin_fmaf.
// gy of one candidate at one lane: v its value, gv the upstream gradient, cf its six coefficient rows in LDS.
//   z = v c0 + c1 (fma);  xh = v c2 - c3;  gr = [z > 0] w g  (tanh: w g (1 - th^2));  gy = ((gr - c4) - xh c5 (fma)) c0 live
// The by-index kernel's vectorizer paired some of these operations across elements, which decided what was contracted, and the
// pairs are part of the bits (`first`: the candidate is candidate 0 of the MixedOp, the first one the unrolled loop met):
//   xh   one fma -- but a rounded product minus c3 in scalar lanes (VEC == 1), and for the odd elements of candidate 0;
//   tanh gr - c4 is one fma of w g and (1 - th^2) = fma(-th, th, 1) -- but element 3 of candidate 0 rounds w g (1 - th^2), the
//        difference and xh c5 one by one.
template <int VEC, int ACT>
__device__ __forceinline__ Vec<VEC> apply_gy(const Vec<VEC>& v, const Vec<VEC>& gv, const float* cf, int D, float wk, float live, bool first) {
#pragma clang fp contract(off)
  const Vec<VEC> c0 = Vec<VEC>::load(cf), c1 = Vec<VEC>::load(cf + D), c2 = Vec<VEC>::load(cf + 2 * D),
                 c3 = Vec<VEC>::load(cf + 3 * D), c4 = Vec<VEC>::load(cf + 4 * D), c5 = Vec<VEC>::load(cf + 5 * D);
  Vec<VEC> o;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const float z = __builtin_fmaf(v[j], c0[j], c1[j]);
    float xh = __builtin_fmaf(v[j], c2[j], -c3[j]);
    if (VEC == 1 && ACT == 0) xh = v[j] * c2[j] - c3[j];
    else if (ACT == 0 && (j & 1)) xh = first ? v[j] * c2[j] - c3[j] : xh;
    float t;
    if constexpr (ACT == 0) {
      const float gr = z > 0.f ? wk * gv[j] : 0.f;
      t = __builtin_fmaf(-xh, c5[j], gr - c4[j]);
    } else {
      const float th = tanhf(z);
      const float wg = wk * gv[j], om = __builtin_fmaf(-th, th, 1.f);
      t = __builtin_fmaf(-xh, c5[j], __builtin_fmaf(wg, om, -c4[j]));
      if (VEC == 4 && j == 3) t = first ? (wg * om - c4[j]) - xh * c5[j] : t;
    }
    o[j] = t * c0[j] * live;
  }
  return o;
}

// the gated candidate's folded store (same expressions, same order as dense_dz_k<.., 0>): gc = gy * ck;
// dz = gc * s * gate * (1 - gate);  o2 = gc * gate, the direct term of the gradient w.r.t. s
template <int VEC>
__device__ __forceinline__ void apply_gated(const Vec<VEC>& gy, float ck, const Vec<VEC>& sv, const Vec<VEC>& ga, Vec<VEC>& dzv, Vec<VEC>& o2) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const float gc = gy[j] * ck;
    o2[j] = gc * ga[j];
    dzv[j] = gc * sv[j] * ga[j] * (1.0f - ga[j]);
  }
}

// the row-scaled candidate's share of gs_out: o2 + (gy * f_r + dz_r * u)
template <int VEC>
__device__ __forceinline__ void apply_row_term(Vec<VEC>& o2, const Vec<VEC>& orv, float rfv, float dzr, const Vec<VEC>& guv) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < VEC; ++j) o2[j] = o2[j] + __builtin_fmaf(orv[j], rfv, dzr * guv[j]);
}

// this lane's part of the row dot sum_c gy * s: each product rounded, added in column order
template <int VEC>
__device__ __forceinline__ float apply_row_dot(const Vec<VEC>& orv, const Vec<VEC>& sv) {
#pragma clang fp contract(off)
  float dq = 0.f;
#pragma unroll
  for (int j = 0; j < VEC; ++j) dq = dq + orv[j] * sv[j];
  return dq;
}

template <int VEC>
__device__ __forceinline__ Vec<VEC> apply_scaled(const Vec<VEC>& a, float x) {
#pragma clang fp contract(off)
  Vec<VEC> o;
#pragma unroll
  for (int j = 0; j < VEC; ++j) o[j] = a[j] * x;
  return o;
}

template <int VEC>
__device__ __forceinline__ Vec<VEC> apply_sum(const Vec<VEC>& a, const Vec<VEC>& b) {
#pragma clang fp contract(off)
  Vec<VEC> o;
#pragma unroll
  for (int j = 0; j < VEC; ++j) o[j] = a[j] + b[j];
  return o;
}

// the recomputed gated candidate's value gate * s * c_r (the row GEMM's gate epilogue: g * in * cs)
template <int VEC>
__device__ __forceinline__ Vec<VEC> apply_gate_value(const Vec<VEC>& ga, const Vec<VEC>& sv, float gck) {
#pragma clang fp contract(off)
  Vec<VEC> o;
#pragma unroll
  for (int j = 0; j < VEC; ++j) o[j] = ga[j] * sv[j] * gck;
  return o;
}

constexpr int APPLY_NO = 5;                     // stored candidates of a role-resolved launch
struct ApplySlots { int g, r, a, o[APPLY_NO]; };      // the candidate index (coefficient / weight slot) behind each role
struct ApplyOther { const float* y; float* gy; const float* full; };
template <int NO> struct ApplyOthers { ApplyOther o[NO]; };

// HG / HR / HA: the gated, row and add roles exist.  NO: stored candidates -- exactly NO with a gated role, n_oth <= NO without.
template <int VEC, int LPR, int KMAX, int ACT, bool HG, bool HR, bool HA, int NO>
__global__ __launch_bounds__(MRG_BLOCK) void mix_bwd_apply_k(
    const float* __restrict__ g, const float* __restrict__ coef, const float* __restrict__ coef2, const float* __restrict__ w, int K,
    int64_t rows, int D, const int32_t* __restrict__ vrows, ApplySlots slot, int n_oth, ApplyOthers<NO> oth,
    const float* __restrict__ gate, const float* __restrict__ s, const float* __restrict__ c, const float* __restrict__ ck,
    float* __restrict__ dz, float* __restrict__ gs_out,
    const float* __restrict__ rf, const float* __restrict__ rh, const float* __restrict__ uvc, int uld, int64_t b0, int64_t b1,
    float* __restrict__ rdq) {
  static_assert(!HR || (HG && KMAX == 1), "the row dot is one group_sum over the row's lanes; its gradient goes into gs_out");
  static_assert(!HA || HG, "the added candidate goes into the gated candidate's gs_out");
  extern __shared__ float lds[];                 // [K][6][D]: scale, shift, invstd, mean*invstd, c1, c2
  constexpr int RPB = MRG_BLOCK / LPR;
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dv = D / VEC;
  for (int t = threadIdx.x; t < K * 6 * D; t += MRG_BLOCK) {
    int k = t / (6 * D), rem = t - k * 6 * D;
    lds[t] = rem < 4 * D ? coef[(int64_t)k * 4 * D + rem] : coef2[(int64_t)k * 2 * D + rem - 4 * D];
  }
  __syncthreads();
  const int n = HG ? NO : n_oth;
  const bool first0 = slot.o[0] == 0;           // candidate 0 (apply_gy): only the first stored one of a launch without a gated role can be it
  float wg = 0.f, wr = 0.f, wa = 0.f, wo[NO];
  const float* cfo[NO];
  if constexpr (HG) wg = w[slot.g];
  if constexpr (HR) wr = w[slot.r];
  if constexpr (HA) wa = w[slot.a];
#pragma unroll
  for (int i = 0; i < NO; ++i) {
    wo[i] = i < n ? w[slot.o[i]] : 0.f;
    cfo[i] = lds + (i < n ? slot.o[i] : 0) * 6 * D;
  }
  const float* cfg = lds + (HG ? slot.g : 0) * 6 * D;
  const float* cfr = lds + (HR ? slot.r : 0) * 6 * D;
  const float* cfa = lds + (HA ? slot.a : 0) * 6 * D;
  const int64_t nvalid = valid_rows(vrows, rows);
  const int64_t step = (int64_t)gridDim.x * RPB;
  for (int64_t r = (int64_t)blockIdx.x * RPB + rw; r < rows; r += step) {
    const float live = r < nvalid ? 1.0f : 0.0f;             // capacity padding: every gradient row written there is zero
    const int64_t ro = r * D;
    // row-uniform values (with LPR == 64 the row is the wave's: scalar loads)
    float gck = 1.f, ckv = 1.f, rfv = 1.f, rhv = 0.f, fo[NO];
    const float* urow = uvc;
    if constexpr (HG) { gck = c[r]; ckv = ck[r]; }
    if constexpr (HR) {
      rfv = rf[r];
      rhv = rh[r];
      urow = uvc + (int64_t)((r >= b0) + (r >= b1)) * uld;
    }
#pragma unroll
    for (int i = 0; i < NO; ++i) fo[i] = (HG && i < n && oth.o[i].full) ? oth.o[i].full[r] : 1.f;     // (folded multipliers: next to a gated role only)
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
      const int cc = sl + q * LPR;
      const bool act = cc < dv;
      const int off = cc * VEC;
      Vec<VEC> gsv, gga, guv, ovg, ova, orv, ovo[NO];        // (set and read by the active lanes only)
      float dq = 0.f;
      if (act) {
        // every load first
        if constexpr (HG) { gsv = Vec<VEC>::load(s + ro + off); gga = Vec<VEC>::load(gate + ro + off); }
        if constexpr (HR) guv = Vec<VEC>::load(urow + off);
        const Vec<VEC> gv = Vec<VEC>::load(g + ro + off);
        Vec<VEC> vo[NO];
#pragma unroll
        for (int i = 0; i < NO; ++i) {
          vo[i] = Vec<VEC>::fill(0.f);
          if (i < n && oth.o[i].y) vo[i] = Vec<VEC>::load(oth.o[i].y + ro + off);
        }
        if constexpr (HG) ovg = apply_gy<VEC, ACT>(apply_gate_value<VEC>(gga, gsv, gck), gv, cfg + off, D, wg, live, false);
        if constexpr (HA) ova = apply_gy<VEC, ACT>(gsv, gv, cfa + off, D, wa, live, false);
        if constexpr (HR) {
          orv = apply_gy<VEC, ACT>(apply_scaled<VEC>(gsv, rfv), gv, cfr + off, D, wr, live, false);
          dq = apply_row_dot<VEC>(orv, gsv);
        }
#pragma unroll
        for (int i = 0; i < NO; ++i)
          if (i < n) ovo[i] = apply_gy<VEC, ACT>(vo[i], gv, cfo[i] + off, D, wo[i], live, !HG && i == 0 && first0);
      }
      float dzr = 0.f;
      if constexpr (HR) {                                  // all lanes of the row (inactive ones carry 0)
        const float qr = group_sum<LPR>(dq);                // (one row per wave: DPP + scalar registers, no LDS round trips)
        dzr = qr * rhv;
        if (sl == 0) rdq[r] = qr;
      }
      if (act) {
#pragma unroll
        for (int i = 0; i < NO; ++i)
          if (i < n) {
            Vec<VEC> o = ovo[i];
            if (HG && oth.o[i].full) o = apply_scaled<VEC>(o, fo[i]);     // f_comp: dz = g * c
            o.store(oth.o[i].gy + ro + off);
          }
        if constexpr (HG) {
          Vec<VEC> dzv, o2;
          apply_gated<VEC>(ovg, ckv, gsv, gga, dzv, o2);
          if constexpr (HA) o2 = apply_sum<VEC>(o2, ova);   // + the gradient of the candidate whose output IS s
          if constexpr (HR) apply_row_term<VEC>(o2, orv, rfv, dzr, guv);
          o2.store(gs_out + ro + off);
          dzv.store(dz + ro + off);
        }
      }
    }
  }
}

// ---- backward apply, any layout: the candidates one after the other (a loop that is NOT unrolled: the per-candidate arrays stay
// in the argument block and each trip loads the few fields it needs), the row-scaled and the added candidate first.  Same
// expressions as above.
template <int VEC>
struct ApplyAny {
  const PtrPack& ys; const RowScalePack& rsp; const GatedPack& gp;
  const float* lds; const float* w; int D; int act;
  // gy of candidate k at (row offset ro, column offset off); *raw: what its slot of ys holds (the gate of the gated candidate)
  __device__ __forceinline__ Vec<VEC> gy(int k, int64_t r, int64_t ro, int off, const Vec<VEC>& gv, const Vec<VEC>& gsv, float live, Vec<VEC>* raw) const {
    Vec<VEC> v = Vec<VEC>::fill(0.f);
    const float* y = ys.p[k];
    if (y) v = Vec<VEC>::load(y + ro + off);
    *raw = v;
    if (k == gp.k) v = apply_gate_value<VEC>(v, gsv, gp.c[r]);
    if (k == gp.rk) v = apply_scaled<VEC>(v, gp.rf[r]);
    const float* cf = lds + k * 6 * D + off;
    return act == 1 ? apply_gy<VEC, 1>(v, gv, cf, D, w[k], live, k == 0) : apply_gy<VEC, 0>(v, gv, cf, D, w[k], live, k == 0);
  }
};

template <int VEC, int LPR, int KMAX>
__global__ __launch_bounds__(MRG_BLOCK) void mix_bwd_apply_any_k(const float* __restrict__ g, PtrPack ys, MutPack gys, int K,
                                                                 const float* __restrict__ coef, const float* __restrict__ coef2,
                                                                 const float* __restrict__ w, int64_t rows, int D, RowScalePack rsp,
                                                                 GatedPack gp) {
  extern __shared__ float lds[];                 // [K][6][D]: scale, shift, invstd, mean*invstd, c1, c2
  constexpr int RPB = MRG_BLOCK / LPR;
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dv = D / VEC;
  for (int t = threadIdx.x; t < K * 6 * D; t += MRG_BLOCK) {
    int k = t / (6 * D), rem = t - k * 6 * D;
    lds[t] = rem < 4 * D ? coef[(int64_t)k * 4 * D + rem] : coef2[(int64_t)k * 2 * D + rem - 4 * D];
  }
  __syncthreads();
  const ApplyAny<VEC> any{ys, rsp, gp, lds, w, D, gp.act};
  const bool hass = gp.k >= 0 || gp.rk >= 0, hasr = KMAX == 1 && gp.rk >= 0;      // (a row role: KMAX == 1, host-checked)
  const int64_t nvalid = valid_rows(gp.vrows, rows);
  for (int64_t r = (int64_t)blockIdx.x * RPB + rw; r < rows; r += (int64_t)gridDim.x * RPB) {
    const float live = r < nvalid ? 1.0f : 0.0f;
    const int64_t ro = r * D;
#pragma unroll 1
    for (int q = 0; q < KMAX; ++q) {
      const int cc = sl + q * LPR;
      const bool act = cc < dv;
      const int off = cc * VEC;
      Vec<VEC> gsv = Vec<VEC>::fill(0.f), guv, gv, orv, raw;
      float rfv = 1.f, rhv = 0.f, dq = 0.f;
      if (act) {
        gv = Vec<VEC>::load(g + ro + off);
        if (hass) gsv = Vec<VEC>::load(gp.s + ro + off);
        if (hasr) {
          rfv = gp.rf[r];
          rhv = gp.rh[r];
          guv = Vec<VEC>::load(gp.uvc + (int64_t)((r >= gp.b0) + (r >= gp.b1)) * gp.uld + off);
          orv = any.gy(gp.rk, r, ro, off, gv, gsv, live, &raw);
          dq = apply_row_dot<VEC>(orv, gsv);
        }
      }
      float dzr = 0.f;
      if (hasr) {                                          // KMAX == 1 (host-checked)
        const float qr = group_sum<LPR>(dq);
        dzr = qr * rhv;
        if (sl == 0) gp.rdq[r] = qr;
      }
      if (act) {
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
          float* dst = gys.p[k];
          if (dst == nullptr) continue;
          Vec<VEC> o = any.gy(k, r, ro, off, gv, gsv, live, &raw);
          const int on = rsp.on[k];
          if (on) {                                        // the consumer's first backward pass (mrg_dense_filter_dz) folded into this store
            const float* full = rsp.full[k];
            float ckv;
            if (full) ckv = full[r];
            else if (r < rsp.edge_rows[k]) { const float* rs = rsp.rs[k]; ckv = rsp.scale[k] * (rs ? rs[r] : 1.0f); }
            else ckv = rsp.self_scale[k];
            if (on == 2) {
              // (the recomputed candidate holds both already: the host checks rsp.s[k] == gp.s and rsp.gate[k] == ys.p[k])
              const Vec<VEC> sv = k == gp.k ? gsv : Vec<VEC>::load(rsp.s[k] + ro + off);
              const Vec<VEC> ga = k == gp.k ? raw : Vec<VEC>::load(rsp.gate[k] + ro + off);
              Vec<VEC> dzv, o2;
              apply_gated<VEC>(o, ckv, sv, ga, dzv, o2);
              const int af = rsp.add_from[k];
              if (af >= 0) o2 = apply_sum<VEC>(o2, any.gy(af, r, ro, off, gv, gsv, live, &raw));
              if (hasr && k == gp.k) apply_row_term<VEC>(o2, orv, rfv, dzr, guv);
              o2.store(rsp.gs_out[k] + ro + off);
              o = dzv;
            } else {                                       // f_comp: dz = g * c
              o = apply_scaled<VEC>(o, ckv);
            }
          }
          o.store(dst + ro + off);
        }
      }
    }
  }
}

// ---- "static step graphs" (round 5): row counts that live in device memory ------------------------------------------------------
// The reference's search loop draws a NEW step graph every step (search/mr_lp_search.py:187-214) whose node count depends on the
// draw; to replay that step from ONE captured HIP graph every tensor must keep its shape, so the step graph is padded to a host-known
// node CAPACITY and the true counts stay in device memory.  A launch of the MixedOp-epilogue / cell-zero kernels that is given such a
// count (`valid_rows`, an int32 [1] in device memory: mrg_gated_branch.valid_rows, or an argument where the entry point has no
// descriptor; NULL = every row is valid) treats rows at and beyond it as padding: left out of the BatchNorm statistics and of every
// gradient reduction, counted out of `total_rows`, and WRITTEN AS ZEROS by the combine and gradient passes -- which keeps the padding rows of every state zero, and a zero row yields a zero candidate in every operator of
// the search space, so no other kernel needs to know.  The caller that owns the counts (the step graph) passes them per call.
// statistics: the flat kernels' bound (512 blocks measured best: profiles/r3_stream_grid.txt)
static_assert(STREAM_BLOCKS <= 1024, "the statistics' partial buffers are sized for 1024 blocks");
static int mix_grid(int64_t rows, int lpr) { return capped(row_blocks(rows, lpr, 8), STREAM_BLOCKS); }
// backward reduction / combine: since the row addressing became scalar these kernels hold 4 / 8 workgroups per CU and gain from
// more blocks than the 512 of the flat kernels (lab: 3.0 -> 2.4 ms and 2.53 -> 2.42 ms per step at 1024)
static int mix_reduce_grid(int64_t rows, int lpr) { return capped(row_blocks(rows, lpr, 8), 1024); }   // partial buffers: 1024 blocks
static int mix_apply_grid(int64_t rows, int lpr) { return capped(row_blocks(rows, lpr, 4), MRG_MAX_GRID); }
static int mix_fwd_grid(int64_t rows, int lpr) { return capped(row_blocks(rows, lpr, 4), 1024); }

static bool pack_ok(const void* const* host, int K) { return host != nullptr && K >= 1 && K <= MRG_MIX_MAXK; }

// host descriptor (include/mrgnas.h: mrg_gated_branch) -> kernel argument; *al: every pointer it adds is 16-byte aligned.
// Absent candidates keep their index < 0 and get SAFE pointers (valid [rows] / [rows, D] memory): the kernels load their row
// factors unconditionally and discard them by a select.
static int gated_pack(const mrg_gated_branch* gb, const float* const* y_host, int K, GatedPack* gp, bool* al, bool apply = false) {
  *gp = GatedPack{};
  gp->k = -1; gp->pair_k = -1; gp->rk = -1;
  gp->vrows = gb ? gb->valid_rows : nullptr;
  if (gb && gb->act != 0 && gb->act != 1) return MRG_E_ENUM;
  gp->act = gb ? gb->act : 0;
  if (gp->act == 1 && (K > 5 || gb->k >= 0 || gb->row_k >= 0)) return MRG_E_SHAPE;    // the tanh instances: un-gated, at most five candidates
  if (!gb || (gb->k < 0 && gb->row_k < 0)) return MRG_OK;
  if (gb->k >= K || gb->row_k >= K || (gb->k >= 0 && gb->k == gb->row_k)) return MRG_E_SHAPE;
  if (!gb->s) return MRG_E_NULLPTR;
  gp->s = gb->s;
  if (gb->k >= 0) {
    if (!gb->rowscale || !y_host[gb->k]) return MRG_E_NULLPTR;       // the gate stands where the candidate's output would
    gp->k = gb->k; gp->c = gb->rowscale;
  }
  if (gb->row_k >= 0) {
    if (!gb->row_f) return MRG_E_NULLPTR;
    if (y_host[gb->row_k] != gb->s) return MRG_E_SHAPE;               // the row-scaled candidate's slot holds s itself
    gp->rk = gb->row_k; gp->rf = gb->row_f;
    if (apply) {
      if (!gb->row_h || !gb->row_uvc || !gb->row_dq) return MRG_E_NULLPTR;
      if (gb->b0 < 0 || gb->b1 < gb->b0 || gb->row_ld <= 0) return MRG_E_SHAPE;
      gp->rh = gb->row_h; gp->uvc = gb->row_uvc; gp->uld = gb->row_ld; gp->b0 = gb->b0; gp->b1 = gb->b1; gp->rdq = gb->row_dq;
      *al = *al && aligned16(gb->row_uvc) && gb->row_ld % 4 == 0;
    }
  }
  if (!gp->c) gp->c = gp->rf;
  if (!gp->rf) gp->rf = gp->c;
  if (!gp->rh) { gp->rh = gp->rf; gp->uvc = gp->s; gp->uld = 0; gp->b0 = gp->b1 = 0; }   // loaded, never used
  for (int q = 0; q < K; ++q)
    if (q != gb->k && q != gb->row_k && y_host[q] == gb->s) { gp->pair_k = q; break; }
  *al = *al && aligned16(gb->s);
  return MRG_OK;
}

// (declared in mixedop_parts.hpp: cell zero's statistics end in the same kernel)
int launch_reduce_finalize_fwd(const void* ws, int nb, const BnPacks& bn, int K, double total_rows, int D, float eps, float momentum,
                               float* coef, const int32_t* vrows, hipStream_t st) {
  hipLaunchKernelGGL(mix_reduce_finalize_fwd_k, dim3((D + 63) / 64, K), dim3(1024), 0, st, (const double*)ws, nb, bn.gamma, bn.beta, bn.rmean,
                     bn.rvar, K, total_rows > 0 ? total_rows : 1.0, D, eps, momentum, coef, vrows);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_mix_workspace_bytes(int K, int D) {
  if (K < 1 || K > MRG_MIX_MAXK || D <= 0) return 0;
  return (int64_t)1024 * K * 3 * D * sizeof(double);
}

// the statistics kernel: per-block partial sums [grid][K][2][D] in ws
static int mix_colstats_blocks(const float* const* y_host, int K, int64_t rows, int D, void* ws, hipStream_t st, int* grid_out,
                               const mrg_gated_branch* gated) {
  if (!pack_ok((const void* const*)y_host, K)) return MRG_E_SHAPE;
  if (rows < 0 || D <= 0) return MRG_E_SHAPE;
  if (!ws) return MRG_E_WORKSPACE;
  PtrPack ys{};
  bool al = true;
  for (int k = 0; k < K; ++k) { ys.p[k] = y_host[k]; al = al && aligned16(y_host[k]); }
  GatedPack gp;
  const int grc = gated_pack(gated, y_host, K, &gp, &al);
  if (grc != MRG_OK) return grc;
  RowGeom g = row_geom(D, al);
  if (!g.ok) return MRG_E_SHAPE;
  int grid = 1;
#define CALL(V, L, KM)                                                                                    \
  do {                                                                                                    \
    grid = mix_grid(rows, L);                                                                             \
    if (gp.k >= 0 || gp.rk >= 0) hipLaunchKernelGGL((mix_colstats_k<V, L, KM, true>), dim3(grid), dim3(MRG_BLOCK), 0, st, ys, K, rows, D, (double*)ws, gp); \
    else hipLaunchKernelGGL((mix_colstats_k<V, L, KM, false>), dim3(grid), dim3(MRG_BLOCK), 0, st, ys, K, rows, D, (double*)ws, gp); \
  } while (0)
  MRG_DISPATCH_GEOM(g, CALL);
#undef CALL
  MRG_LAUNCH_CHECK();
  *grid_out = grid;
  return MRG_OK;
}

// mrg_mix_colstats + mrg_mix_finalize_fwd in two launches instead of three (statistics kernel, then reduction and finalize fused):
// for callers without a collective between the two (the single-GPU step).  Same results bit for bit.
extern "C" int mrg_mix_stats_coef(const float* const* y_host, const float* const* gamma_host, const float* const* beta_host,
                                  float* const* rmean_host, float* const* rvar_host, int K, int64_t rows, double total_rows, int D, float eps,
                                  float momentum, float* coef, void* ws, const mrg_gated_branch* gated, void* stream) {
  const int32_t* valid_rows = gated ? gated->valid_rows : nullptr;
  if (K < 1 || K > MRG_MIX_MAXK || D <= 0 || total_rows < 0) return MRG_E_SHAPE;
  if (valid_rows && total_rows != (double)rows) return MRG_E_SHAPE;          // a device count names this launch's rows, not a sharded total
  if (!coef || !gamma_host || !beta_host) return MRG_E_NULLPTR;
  hipStream_t st = (hipStream_t)stream;
  int grid = 1;
  bool any_given = false;
  for (int k = 0; gated && k < K; ++k) any_given = any_given || gated->given[k] != nullptr;
  if (!any_given) {
    const int rc = mix_colstats_blocks(y_host, K, rows, D, ws, st, &grid, gated);
    if (rc != MRG_OK) return rc;
  } else {
    // Candidates whose producers formed their sums are hidden from the statistics kernel (an absent candidate costs it nothing);
    // when none is left to read, it does not run.
    if (valid_rows) return MRG_E_SHAPE;                      // a producer counts every row
    if (!pack_ok((const void* const*)y_host, K) || rows < 0) return MRG_E_SHAPE;
    if (!ws) return MRG_E_WORKSPACE;
    const float* y2[MRG_MIX_MAXK];
    mrg_gated_branch g2 = *gated;
    GivenPack gv{};
    bool any_read = false;
    int64_t n_max = 1;
    for (int k = 0; k < K; ++k) {
      y2[k] = y_host[k];
      if (!gated->given[k]) { any_read = any_read || y_host[k] != nullptr; continue; }
      if (gated->given_n[k] < 1 || gated->given_stride[k] < 2 * (int64_t)D) return MRG_E_SHAPE;
      gv.p[k] = gated->given[k]; gv.n[k] = gated->given_n[k]; gv.stride[k] = gated->given_stride[k];
      if (gv.n[k] > n_max) n_max = gv.n[k];
      y2[k] = nullptr;
      if (g2.k == k) g2.k = -1;
      if (g2.row_k == k) g2.row_k = -1;
    }
    if (any_read) {
      const int rc = mix_colstats_blocks(y2, K, rows, D, ws, st, &grid, &g2);
      if (rc != MRG_OK) return rc;
    } else {
      const int64_t g = (n_max + 15) / 16;
      grid = (int)(g < 256 ? g : 256);
    }
    hipLaunchKernelGGL(mix_given_reduce_k, dim3(grid, K), dim3(MRG_BLOCK), 0, st, gv, K, D, (double*)ws, any_read ? 0 : 1);
    MRG_LAUNCH_CHECK();
  }
  BnPacks bn;
  const int prc = bn_packs(&bn, gamma_host, beta_host, rmean_host, rvar_host, K);
  if (prc != MRG_OK) return prc;
  return launch_reduce_finalize_fwd(ws, grid, bn, K, total_rows, D, eps, momentum, coef, valid_rows, st);
}

// sums [K][2][D] float64
// (with mrg_mix_finalize_fwd: the sharded path, whose row totals are host-known -- no device row count)
extern "C" int mrg_mix_colstats(const float* const* y_host, int K, int64_t rows, int D, double* sums, void* ws,
                                const mrg_gated_branch* gated, void* stream) {
  if (!sums) return MRG_E_NULLPTR;
  if (gated && gated->valid_rows) return MRG_E_SHAPE;
  for (int k = 0; gated && k < MRG_MIX_MAXK; ++k)
    if (gated->given[k]) return MRG_E_SHAPE;                 // producer sums are this launch's rows, finished by mrg_mix_stats_coef only
  hipStream_t st = (hipStream_t)stream;
  int grid = 1;
  const int rc = mix_colstats_blocks(y_host, K, rows, D, ws, st, &grid, gated);
  if (rc != MRG_OK) return rc;
  int len = K * 2 * D;
  launch_ordered_reduce<double>((const double*)ws, sums, 0, grid, len, len, st);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

// coef [K][4][D]; gamma/beta/running_mean/running_var: host arrays of K device pointers (entries may be NULL)
extern "C" int mrg_mix_finalize_fwd(const double* sums, const float* const* gamma_host, const float* const* beta_host,
                                    float* const* rmean_host, float* const* rvar_host, int K, double total_rows, int D,
                                    float eps, float momentum, float* coef, void* stream) {
  if (K < 1 || K > MRG_MIX_MAXK || D <= 0 || total_rows < 0) return MRG_E_SHAPE;
  if (!sums || !coef || !gamma_host || !beta_host) return MRG_E_NULLPTR;
  BnPacks bn;
  const int prc = bn_packs(&bn, gamma_host, beta_host, rmean_host, rvar_host, K);
  if (prc != MRG_OK) return prc;
  hipLaunchKernelGGL(mix_finalize_fwd_k, dim3((D + 127) / 128, K), dim3(128), 0, (hipStream_t)stream, sums, bn.gamma, bn.beta, bn.rmean, bn.rvar, K,
                     total_rows > 0 ? total_rows : 1.0, D, eps, momentum, coef, (const int32_t*)nullptr);   // (sharded path: host-known totals)
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_mix_fwd(const float* const* y_host, int K, const float* coef, const float* w, const float* addend, float* out,
                           int64_t rows, int D, const mrg_gated_branch* gated, void* stream) {
  if (!pack_ok((const void* const*)y_host, K) || rows < 0 || D <= 0) return MRG_E_SHAPE;
  if (rows == 0) return MRG_OK;
  if (!coef || !w || !out) return MRG_E_NULLPTR;
  hipStream_t st = (hipStream_t)stream;
  PtrPack ys{};
  bool al = aligned16(out) && aligned16(addend);
  for (int k = 0; k < K; ++k) { ys.p[k] = y_host[k]; al = al && aligned16(y_host[k]); }
  GatedPack gp;
  const int grc = gated_pack(gated, y_host, K, &gp, &al);
  if (grc != MRG_OK) return grc;
  RowGeom g = row_geom(D, al);
  if (!g.ok) return MRG_E_SHAPE;
  size_t lds = (size_t)K * 2 * D * sizeof(float);
  if (lds > 64 * 1024) return MRG_E_SHAPE;
#define CALL(V, L, KM)                                                                                    \
  do {                                                                                                    \
    const dim3 grid_(mix_fwd_grid(rows, L));                                                               \
    if (gp.act == 1) {                                                                                    \
      hipLaunchKernelGGL((mix_fwd_k<V, L, KM, false, 5, 1>), grid_, dim3(MRG_BLOCK), lds, st, ys, K, coef, w, out, rows, D, addend, gp); \
    } else if (gp.k >= 0 || gp.rk >= 0) {                                                                        \
      if (K <= 5) hipLaunchKernelGGL((mix_fwd_k<V, L, KM, true, 5>), grid_, dim3(MRG_BLOCK), lds, st, ys, K, coef, w, out, rows, D, addend, gp); \
      else hipLaunchKernelGGL((mix_fwd_k<V, L, KM, true, MRG_MIX_MAXK>), grid_, dim3(MRG_BLOCK), lds, st, ys, K, coef, w, out, rows, D, addend, gp); \
    } else {                                                                                              \
      if (K <= 5) hipLaunchKernelGGL((mix_fwd_k<V, L, KM, false, 5>), grid_, dim3(MRG_BLOCK), lds, st, ys, K, coef, w, out, rows, D, addend, gp); \
      else hipLaunchKernelGGL((mix_fwd_k<V, L, KM, false, MRG_MIX_MAXK>), grid_, dim3(MRG_BLOCK), lds, st, ys, K, coef, w, out, rows, D, addend, gp); \
    }                                                                                                     \
  } while (0)
  MRG_DISPATCH_GEOM(g, CALL);
#undef CALL
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

// red [K][3][D] float32
extern "C" int mrg_mix_bwd_reduce(const float* g, const float* const* y_host, int K, const float* coef, const float* w, float* red,
                                  void* ws, int64_t rows, int D, const mrg_gated_branch* gated, void* stream) {
  if (!pack_ok((const void* const*)y_host, K) || rows < 0 || D <= 0) return MRG_E_SHAPE;
  if (!coef || !w || !red || (rows > 0 && !g)) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  PtrPack ys{};
  bool al = aligned16(g);
  for (int k = 0; k < K; ++k) { ys.p[k] = y_host[k]; al = al && aligned16(y_host[k]); }
  GatedPack gp;
  const int grc = gated_pack(gated, y_host, K, &gp, &al);
  if (grc != MRG_OK) return grc;
  RowGeom gm = row_geom(D, al);
  if (!gm.ok) return MRG_E_SHAPE;
  int grid = 1;
#define CALL(V, L, KM)                                                                                    \
  do {                                                                                                    \
    grid = mix_reduce_grid(rows, L);                                                                             \
    size_t lds = ((size_t)K * 4 * D + (size_t)(MRG_BLOCK / L) * 3 * (L * KM * V)) * sizeof(float);        \
    if (lds > 64 * 1024) return MRG_E_SHAPE;                                                              \
    if (gp.act == 1) hipLaunchKernelGGL((mix_bwd_reduce_k<V, L, KM, 5, false, 1>), dim3(grid), dim3(MRG_BLOCK), lds, st, g, ys, K, coef, w, (float*)ws, rows, D, gp); \
    else if ((gp.k >= 0 || gp.rk >= 0) && K <= 5) hipLaunchKernelGGL((mix_bwd_reduce_k<V, L, KM, 5, true>), dim3(grid), dim3(MRG_BLOCK), lds, st, g, ys, K, coef, w, (float*)ws, rows, D, gp); \
    else if (gp.k >= 0 || gp.rk >= 0) hipLaunchKernelGGL((mix_bwd_reduce_k<V, L, KM, MRG_MIX_MAXK, true>), dim3(grid), dim3(MRG_BLOCK), lds, st, g, ys, K, coef, w, (float*)ws, rows, D, gp); \
    else if (K <= 4) hipLaunchKernelGGL((mix_bwd_reduce_k<V, L, KM, 4, false>), dim3(grid), dim3(MRG_BLOCK), lds, st, g, ys, K, coef, w, (float*)ws, rows, D, gp); \
    else hipLaunchKernelGGL((mix_bwd_reduce_k<V, L, KM, MRG_MIX_MAXK, false>), dim3(grid), dim3(MRG_BLOCK), lds, st, g, ys, K, coef, w, (float*)ws, rows, D, gp); \
  } while (0)
  MRG_DISPATCH_GEOM(gm, CALL);
#undef CALL
  MRG_LAUNCH_CHECK();
  int len = K * 3 * D;
  launch_ordered_reduce<float>((const float*)ws, red, 0, grid, len, len, st);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

// coef2 [K][2][D]; dgamma/dbeta: host arrays of K device pointers (NULL entries skipped); dw [K]
extern "C" int mrg_mix_finalize_bwd(const float* red, int K, double total_rows, int D, float* coef2, float* const* dgamma_host,
                                    float* const* dbeta_host, float* dw, const int32_t* valid_rows, void* stream) {
  if (K < 1 || K > MRG_MIX_MAXK || D <= 0) return MRG_E_SHAPE;
  // a device count replaces total_rows, which must then be the launch's own row count (whole, not a sharded total)
  if (valid_rows && !(total_rows >= 0 && total_rows == (double)(int64_t)total_rows)) return MRG_E_SHAPE;
  if (!red || !coef2 || !dw) return MRG_E_NULLPTR;
  MutPack dg{}, db{};
  for (int k = 0; k < K; ++k) {
    dg.p[k] = dgamma_host ? dgamma_host[k] : nullptr;
    db.p[k] = dbeta_host ? dbeta_host[k] : nullptr;
  }
  hipLaunchKernelGGL(mix_finalize_bwd_k, dim3(K), dim3(256), 0, (hipStream_t)stream, red, K, total_rows > 0 ? total_rows : 1.0, D,
                     coef2, dg, db, dw, valid_rows);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_mix_bwd_apply(const float* g, const float* const* y_host, float* const* gy_host, int K, const float* coef,
                                 const float* coef2, const float* w, const float* const* rs_host, const float* rs_scale_host,
                                 const float* rs_self_host, const int64_t* rs_edge_rows_host, const int* rs_on_host,
                                 const float* const* rs_full_host,
                                 const float* const* fold_s_host, const float* const* fold_gate_host, float* const* fold_gs_host,
                                 const int* fold_add_from_host, int64_t rows, int D, const mrg_gated_branch* gated, void* stream) {
  if (!pack_ok((const void* const*)y_host, K) || !gy_host || rows < 0 || D <= 0) return MRG_E_SHAPE;
  if (rows == 0) return MRG_OK;
  if (!g || !coef || !coef2 || !w) return MRG_E_NULLPTR;
  hipStream_t st = (hipStream_t)stream;
  PtrPack ys{};
  MutPack gys{};
  bool al = aligned16(g);
  bool any = false;
  for (int k = 0; k < K; ++k) {
    ys.p[k] = y_host[k]; gys.p[k] = gy_host[k];
    al = al && aligned16(y_host[k]) && aligned16(gy_host[k]);
    any = any || gy_host[k] != nullptr;
  }
  if (!any) return MRG_OK;
  RowScalePack rsp{};
  for (int k = 0; k < MRG_MIX_MAXK; ++k) rsp.add_from[k] = -1;
  if (rs_on_host) {
    if (!rs_scale_host || !rs_self_host || !rs_edge_rows_host) return MRG_E_NULLPTR;
    for (int k = 0; k < K; ++k) {
      rsp.on[k] = rs_on_host[k];
      rsp.rs[k] = rs_host ? rs_host[k] : nullptr;
      rsp.full[k] = (rs_full_host && rsp.on[k]) ? rs_full_host[k] : nullptr;
      rsp.scale[k] = rs_scale_host[k]; rsp.self_scale[k] = rs_self_host[k]; rsp.edge_rows[k] = rs_edge_rows_host[k];
      if (rsp.on[k] == 2) {
        if (!fold_s_host || !fold_gate_host || !fold_gs_host || !fold_s_host[k] || !fold_gate_host[k] || !fold_gs_host[k]) return MRG_E_NULLPTR;
        rsp.s[k] = fold_s_host[k]; rsp.gate[k] = fold_gate_host[k]; rsp.gs_out[k] = fold_gs_host[k];
        if (fold_add_from_host && fold_add_from_host[k] >= 0) {
          const int q = fold_add_from_host[k];
          if (q >= K || q == k || !y_host[q] || y_host[q] != rsp.s[k]) return MRG_E_SHAPE;      // only a candidate whose OUTPUT is this one's operand s
          rsp.add_from[k] = q;
          any = true;
        }
        al = al && aligned16(rsp.s[k]) && aligned16(rsp.gate[k]) && aligned16(rsp.gs_out[k]);
      } else if (rsp.on[k] != 0 && rsp.on[k] != 1) {
        return MRG_E_ENUM;
      }
    }
  }
  GatedPack gp;
  const int grc = gated_pack(gated, y_host, K, &gp, &al, true);
  if (grc != MRG_OK) return grc;
  // the recomputed candidate's folded gradient store reads s and the gate it already holds: they must be the same tensors
  if (gp.k >= 0 && rsp.on[gp.k] == 2 && (rsp.s[gp.k] != gp.s || rsp.gate[gp.k] != y_host[gp.k])) return MRG_E_SHAPE;
  // the row-scaled candidate has no gradient tensor: its gradient w.r.t. s goes into the gated candidate's direct term
  if (gp.rk >= 0 && (gp.k < 0 || rsp.on[gp.k] != 2 || gy_host[gp.rk] != nullptr)) return MRG_E_SHAPE;
  RowGeom gm = row_geom(D, al);
  if (!gm.ok) return MRG_E_SHAPE;
  if (gp.rk >= 0 && gm.kmax != 1) return MRG_E_SHAPE;               // the row dot is one group_sum over the row's lanes
  size_t lds = (size_t)K * 6 * D * sizeof(float);
  if (lds > 64 * 1024) return MRG_E_SHAPE;
  // Roles (see mix_bwd_apply_k).  resolved: every candidate is one of gated / row / add / other in a form the role kernel has.
  ApplySlots slot{-1, -1, -1, {0, 0, 0, 0, 0}};
  ApplyOthers<APPLY_NO> oth{};
  int n_oth = 0;
  const int G = gp.k, R = gp.rk, A = G >= 0 ? rsp.add_from[G] : -1;
  bool resolved = K <= 5;
  if (G >= 0) resolved = resolved && rsp.on[G] == 2 && rsp.full[G] && gy_host[G];     // recomputed AND folded (the host checked s / gate above)
  if (A >= 0) resolved = resolved && gy_host[A] == nullptr;
  for (int k = 0; k < K && resolved; ++k) {
    if (k == G || k == R || k == A) continue;
    if (rsp.on[k] == 2 || (rsp.on[k] == 1 && (!rsp.full[k] || G < 0))) resolved = false;
    else if (gy_host[k]) {
      slot.o[n_oth] = k;
      oth.o[n_oth++] = ApplyOther{y_host[k], gy_host[k], rsp.on[k] ? rsp.full[k] : nullptr};
    }
  }
  slot.g = G; slot.r = R; slot.a = A;
  // (candidate 0 next to a gated role -- f_zero in the search space, absent here -- would need apply_gy's `first` in every role)
  if (G >= 0 && (G == 0 || R == 0 || A == 0 || (n_oth > 0 && slot.o[0] == 0))) resolved = false;
  // the instances the library's callers reach: a last-stage / tail MixedOp (no gated role), and the first stage with its row-factor
  // candidate and folded f_identity (default), without the row factor (above 256 columns, or switched off), without the fold
  const int layout = !resolved ? -1 : G < 0 ? 0 : (R >= 0 && A >= 0 && n_oth == 1) ? 1 : (R < 0 && A >= 0 && n_oth == 2) ? 2
                                                  : (R >= 0 && A < 0 && n_oth == 2) ? 3 : -1;
#define ROLE(V, L, KM, ACT, HG, HR, HA, NO)                                                                                        \
  do {                                                                                                                             \
    ApplyOthers<NO> o_{};                                                                                                          \
    for (int i = 0; i < NO; ++i) o_.o[i] = oth.o[i];                                                                                \
    hipLaunchKernelGGL((mix_bwd_apply_k<V, L, KM, ACT, HG, HR, HA, NO>), grid_, dim3(MRG_BLOCK), lds, st, g, coef, coef2, w, K, rows, D, \
                       gp.vrows, slot, n_oth, o_, G >= 0 ? y_host[G] : nullptr, gp.s, gp.c, G >= 0 ? rsp.full[G] : nullptr,          \
                       G >= 0 ? gy_host[G] : nullptr, G >= 0 ? rsp.gs_out[G] : nullptr, gp.rf, gp.rh, gp.uvc, gp.uld, gp.b0, gp.b1,    \
                       gp.rdq);                                                                                                    \
  } while (0)
#define CALL(V, L, KM)                                                                                    \
  do {                                                                                                    \
    const dim3 grid_(mix_apply_grid(rows, L));                                                             \
    if (layout == 0 && gp.act == 1) ROLE(V, L, KM, 1, false, false, false, APPLY_NO);                      \
    else if (layout == 0) ROLE(V, L, KM, 0, false, false, false, APPLY_NO);                                \
    else if (layout == 2) ROLE(V, L, KM, 0, true, false, true, 2);                                         \
    else if (layout == 1) ROLE(V, L, 1, 0, true, true, true, 1);          /* (a row role: KMAX == 1, checked above) */ \
    else if (layout == 3) ROLE(V, L, 1, 0, true, true, false, 2);                                          \
    else hipLaunchKernelGGL((mix_bwd_apply_any_k<V, L, KM>), grid_, dim3(MRG_BLOCK), lds, st, g, ys, gys, K, coef, coef2, w, rows, D, rsp, gp); \
  } while (0)
  MRG_DISPATCH_GEOM(gm, CALL);
#undef CALL
#undef ROLE
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}
