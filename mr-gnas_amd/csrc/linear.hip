// Dense linears on edge / node rows: the C entry points of the row GEMMs (forward, input gradient, the fused a_max / a_mean
// forwards) and the kernel switches.  The weight gradient is wgrad.hip.
//   nn.Linear inside a_max_op / a_mean_op: reference models/operations_lp.py:228,231,243,246
//   W_O / W_I / W_S / W_R of CompGraphConv:  reference models/compgcn.py:36-41,77-78,100,103
// Matrix cores: split bf16 by default (shared parts x3_parts.hpp, kernels gemm_x3*.hpp, which launch takes which kernel:
// gemm_dispatch.hpp), exact f32 (gemm.hpp) in mode 1 and for operands the split core cannot take; all on the pipelined row GEMM.
#include "gemm_dispatch.hpp"

namespace mrg {

// a_max, second half: unpack the 64-bit keys of gemm_epilogue_segmax.  out = max (0 without in-edge) + self row;
// arg = the winning edge id (-1 without in-edge); mx = the max itself (the backward's ReLU mask: mx > 0).
__global__ void segmax_finalize_k(const unsigned long long* __restrict__ keys, const float* __restrict__ self_rows,
                                  const int32_t* __restrict__ eid, float* __restrict__ out, int32_t* __restrict__ arg,
                                  float* __restrict__ mx, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long k = keys[i];
    const unsigned lo = (unsigned)k;
    const float v = __uint_as_float((unsigned)(k >> 32));
    out[i] = self_rows ? v + self_rows[i] : v;
    if (arg) arg[i] = lo == 0u ? -1 : eid[0xFFFFFFFFu - lo];
    if (mx) mx[i] = v;
  }
}

}  // namespace mrg

using namespace mrg;

// ---- a_max as two launches: split-core GEMM with the ReLU + segmented-max epilogue, then the unpack pass ---------------
static bool segmax_shape_ok(int K, int Nout) { return K > 48 && K % 4 == 0 && Nout > 0; }

extern "C" int64_t mrg_linear_relu_segmax_workspace_bytes(int64_t N, int K, int Nout) {
  if (N < 0 || !segmax_shape_ok(K, Nout) || gemm_mode() == 1) return 0;   // 0: the split core cannot take the shape or is switched off (use the unfused entry points)
  return ((N * (int64_t)Nout * 8 + 255) / 256) * 256 + (int64_t)bsplit_bytes_any(Nout, K) + 256;
}

extern "C" int mrg_linear_relu_segmax_fwd(const float* X, const float* W, const float* bias, const int32_t* eid, const int32_t* dst,
                                          const float* self_rows, float* out, int32_t* arg, float* mx, void* ws, int64_t E, int64_t N,
                                          int K, int Nout, void* stream) {
  if (E < 0 || N < 0 || K <= 0 || Nout <= 0 || E >= ((int64_t)1 << 32) - 1) return MRG_E_SHAPE;
  if (!segmax_shape_ok(K, Nout)) return MRG_E_SHAPE;
  if (N == 0) return MRG_OK;
  if (!out || !W) return MRG_E_NULLPTR;
  if (E > 0 && (!X || !eid || !dst)) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  if (!aligned16(X) || !aligned16(ws)) return MRG_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)ws;
  const size_t key_bytes = (size_t)((N * (int64_t)Nout * 8 + 255) / 256) * 256;
  void* bsplit = (char*)ws + key_bytes;
  if (hipMemsetAsync(keys, 0, (size_t)N * Nout * 8, st) != hipSuccess) return MRG_E_WORKSPACE;
  if (E > 0) {
    GemmArgs a{};
    a.A1 = X; a.K1 = K; a.B = W; a.bias = bias; a.N = Nout; a.rows = E; a.act = MRG_ACT_RELU;
    a.row_index = eid; a.row_seg = dst; a.seg_out = keys;
    if (!x3_eligible(a)) return MRG_E_SHAPE;
    launch_bsplit_any(EPI_SEGMAX, E, W, K, 1, Nout, K, bsplit, st);
    const int rc = launch_rowgemm_x3_mode<EPI_SEGMAX>(a, bsplit, st);
    if (rc != MRG_OK) return rc;
  }
  const int64_t total = N * (int64_t)Nout;
  hipLaunchKernelGGL(segmax_finalize_k, dim3(stream_grid_for(total, 256 * 4)), dim3(256), 0, st, keys, self_rows, eid, out, arg, mx, total);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

// ---- a_mean (a_sum over ReLU(Linear)) first level: the split-core GEMM over the edges in destination order with the
// run-sum epilogue (gemm_epilogue_segsum); second level: mrg_seg_reduce_heads_fwd.  part: [E, Nout] floats (only head rows
// are written), relu_bits: [E, ceil(Nout / 32)] words.  ws: mrg_gemm_workspace_bytes(K, Nout).
extern "C" int mrg_linear_relu_segsum_fwd(const float* X, const float* W, const float* bias, const int32_t* eid, const int32_t* dst,
                                          float* part, unsigned* relu_bits, void* ws, int64_t E, int K, int Nout, void* stream) {
  if (E < 0 || K <= 0 || Nout <= 0 || E >= ((int64_t)1 << 31)) return MRG_E_SHAPE;
  if (!segmax_shape_ok(K, Nout)) return MRG_E_SHAPE;
  if (E == 0) return MRG_OK;
  if (!X || !W || !eid || !dst || !part) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  if (!aligned16(X) || !aligned16(ws)) return MRG_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  GemmArgs a{};
  a.A1 = X; a.K1 = K; a.B = W; a.bias = bias; a.N = Nout; a.rows = E; a.act = MRG_ACT_RELU;
  a.row_index = eid; a.row_seg = dst; a.seg_part = part; a.relu_bits = relu_bits; a.bits_ld = (Nout + 31) / 32;
  if (!x3_eligible(a)) return MRG_E_SHAPE;
  launch_bsplit_any(EPI_SEGSUM, E, W, K, 1, Nout, K, ws, st);
  return launch_rowgemm_x3_mode<EPI_SEGSUM>(a, ws, st);
}

extern "C" int64_t mrg_gemm_workspace_bytes(int K, int Nout) {
  if (K <= 0 || Nout <= 0) return 0;
  return (int64_t)gemm_workspace_bytes(K, Nout);
}

extern "C" int mrg_gemm_set_mode(int mode) {
  if (mode < 0 || mode > 2) return MRG_E_ENUM;
  gemm_switches().mode = mode;
  return MRG_OK;
}

extern "C" int mrg_gemm_set_wide8(int on) {
  if (on < 0 || on > 1) return MRG_E_ENUM;
  gemm_switches().wide8 = on;
  return MRG_OK;
}

extern "C" int mrg_gemm_set_small(int on) {
  if (on < 0 || on > 1) return MRG_E_ENUM;
  gemm_switches().small_rows = on ? X3N_MAX_ROWS : 0;      // 0 off, 1 the row bound
  return MRG_OK;
}

extern "C" int mrg_gemm_set_q(int on) {
  if (on < 0 || on > 2) return MRG_E_ENUM;          // 2 (lab, tests): every eligible K, not only K > 224
  gemm_switches().q = on;
  return MRG_OK;
}

extern "C" int mrg_linear_fwd(const float* X, const float* W, const float* bias, float* Y, void* ws, int64_t rows, int K, int Nout,
                              int act, void* stream) {
  if (rows < 0 || K <= 0 || Nout <= 0) return MRG_E_SHAPE;
  if (act != MRG_ACT_NONE && act != MRG_ACT_RELU && act != MRG_ACT_SIGMOID) return MRG_E_ENUM;
  if (rows == 0) return MRG_OK;
  if (!X || !W || !Y) return MRG_E_NULLPTR;
  GemmArgs a{};
  a.A1 = X; a.K1 = K; a.B = W; a.bias = bias; a.C = Y; a.ldc = Nout; a.N = Nout; a.rows = rows; a.act = act;
  return launch_gemm<EPI_BIAS_ACT>(a, K, 1, ws, (hipStream_t)stream);
}

extern "C" int64_t mrg_linear_bwd_input_workspace_bytes(int K, int Nout) {
  if (K <= 0 || Nout <= 0) return 0;
  return (int64_t)gemm_workspace_bytes(Nout, K);
}

// gX[rows, K] (+)= gY[rows, Nout] * W[:, 0:K]   where W is [Nout][ldw] row-major (ldw >= K: a column block
// of a wider weight, e.g. one half of an nn.Linear(2D, D)); accumulate != 0 adds into the existing gX.
// The core sees B(n = k_in, k = n_out) = W[n_out * ldw + k_in]: a strided view, no transpose pass on the split path.
extern "C" int mrg_linear_bwd_input(const float* gY, const float* W, float* gX, void* ws, int64_t rows, int K, int Nout,
                                    int ldw, int accumulate, void* stream) {
  if (rows < 0 || K <= 0 || Nout <= 0 || ldw < K) return MRG_E_SHAPE;
  if (rows == 0) return MRG_OK;
  if (!gY || !W || !gX) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  GemmArgs a{};
  a.A1 = gY; a.K1 = Nout; a.B = W; a.C = gX; a.ldc = K; a.N = K; a.rows = rows; a.act = MRG_ACT_NONE;
  if (accumulate) {
    a.Cin = gX; a.ld_cin = K;
    return launch_gemm<EPI_ACCUM>(a, 1, ldw, ws, st);
  }
  return launch_gemm<EPI_BIAS_ACT>(a, 1, ldw, ws, st);
}

// The same joined to a running gradient fan-in sum `total` [rows, K] (functional/fanin.py): gX = (gY W[:, 0:K] + gX) + total with
// accumulate != 0, gX = gY W[:, 0:K] + total without.  total may be gX itself where gX is not also the first addend.
extern "C" int mrg_linear_bwd_input_acc2(const float* gY, const float* W, float* gX, void* ws, int64_t rows, int K, int Nout,
                                         int ldw, int accumulate, void* stream, const float* total) {
  if (rows < 0 || K <= 0 || Nout <= 0 || ldw < K) return MRG_E_SHAPE;
  if (rows == 0) return MRG_OK;
  if (!gY || !W || !gX || !total) return MRG_E_NULLPTR;
  if (accumulate && total == gX) return MRG_E_SHAPE;
  if (!ws) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  GemmArgs a{};
  a.A1 = gY; a.K1 = Nout; a.B = W; a.C = gX; a.ldc = K; a.N = K; a.rows = rows; a.act = MRG_ACT_NONE;
  if (accumulate) {
    a.Cin = gX; a.ld_cin = K;
    gemm_set_cin2(a, total, K);
    return launch_gemm<EPI_ACCUM2>(a, 1, ldw, ws, st);
  }
  a.Cin = total; a.ld_cin = K;
  return launch_gemm<EPI_ACCUM>(a, 1, ldw, ws, st);
}

// ---- the three direction segments of a dense filter in one launch each (split core only) -----------------------------------
// gX rows [0, b0) (+)= gY W[0][:, 0:K], rows [b0, b1) with W[1], rows [b1, M) with W[2]; W: HOST array of three device
// pointers to [Nout][ldw] weights (a column block when offset by the caller).
// The pair form (gY2, W2_host not NULL): gX rows of the three ranges (+)= gY1 W1[s][:, 0:K] + gY2 W2[s][:, 0:K] as ONE product over
// the concatenated reduction dimension, [gY1 | gY2] [W1 ; W2]: the input gradient of two candidates that read the same rows
// (f_dense_comp and f_comp of one MixedOp, reference models/cell_lp.py:95-113, models/operations_lp.py:266-288,356-390) written
// once instead of two gradients that a fan-in pass adds.
static size_t bwd_input3_each(int K, int Nred) { return (size_t)(((int64_t)bsplit_bytes_any(K, Nred) + 255) / 256 * 256); }

// the arguments as checked by the two entry points below; gY2 / W2_host NULL: the single form
// total (NULL: none): the running fan-in sum this product is joined to, gX = (product [+ gX]) + total (mrg_linear_bwd_input_acc2)
static int bwd_input3(const float* gY1, const float* gY2, const float* const* W1_host, const float* const* W2_host, float* gX, void* ws,
                      int64_t b0, int64_t b1, int64_t M, int K, int Nout, int ldw, int accumulate, hipStream_t st,
                      const float* total = nullptr) {
  const bool pair = gY2 != nullptr;
  const int Nred = pair ? 2 * Nout : Nout;       // the reduction dimension
  GemmArgs a{};
  a.A1 = gY1; a.K1 = Nout; a.C = gX; a.ldc = K; a.N = K; a.rows = M; a.act = MRG_ACT_NONE;
  if (pair) { a.A2 = gY2; a.K2 = Nout; }
  if (accumulate) { a.Cin = gX; a.ld_cin = K; }
  if (total && accumulate) {
    if (total == gX) return MRG_E_SHAPE;
    gemm_set_cin2(a, total, K);
  } else if (total) {
    a.Cin = total; a.ld_cin = K;
  }
  // the epilogue kind: the weight split and the launch must name the same one (x3q_shape / x3n_shape are functions of it)
  const int epi = total && accumulate ? EPI_ACCUM2 : (total || accumulate ? EPI_ACCUM : EPI_BIAS_ACT);
  if (!x3_eligible(a)) return MRG_E_SHAPE;
  const int64_t lo[3] = {0, b0, b1}, hi[3] = {b0, b1, M};
  const size_t each = bwd_input3_each(K, Nred);
  const float* Bs[3]; const float* Bs2[3]; void* outs[3];
  a.grp.n = 3;
  a.grp.bp_stride = (int64_t)each;
  for (int i = 0; i < 3; ++i) {
    const bool live = hi[i] > lo[i];
    if (live && (!W1_host[i] || (pair && !W2_host[i]))) return MRG_E_NULLPTR;
    Bs[i] = live ? W1_host[i] : nullptr;
    Bs2[i] = live && pair ? W2_host[i] : nullptr;
    outs[i] = (char*)ws + i * each;
    a.grp.lo[i] = lo[i]; a.grp.hi[i] = live ? hi[i] : lo[i];
    a.grp.scale[i] = 1.0f;
  }
  // B(n = k_in, k) = k < Nout ? W1[k * ldw + k_in] : W2[(k - Nout) * ldw + k_in]
  launch_bsplit3_any(epi, M, Bs, 1, ldw, K, Nred, outs, st, pair ? Bs2 : nullptr, pair ? Nout : 0);
  MRG_LAUNCH_CHECK();
  if (epi == EPI_ACCUM2) return launch_rowgemm_x3_mode<EPI_ACCUM2>(a, outs[0], st);
  if (epi == EPI_ACCUM) return launch_rowgemm_x3_mode<EPI_ACCUM>(a, outs[0], st);
  return launch_rowgemm_x3_mode<EPI_BIAS_ACT>(a, outs[0], st);
}

extern "C" int64_t mrg_linear_bwd_input3_workspace_bytes(int K, int Nout) {
  if (K <= 0 || Nout <= 48 || Nout % 4 != 0 || gemm_mode() == 1) return 0;      // 0: the split core cannot take the shape / is switched off
  return 3 * (int64_t)bwd_input3_each(K, Nout);
}

extern "C" int mrg_linear_bwd_input3(const float* gY, const float* const* W_host, float* gX, void* ws, int64_t b0, int64_t b1, int64_t M,
                                     int K, int Nout, int ldw, int accumulate, void* stream) {
  if (K <= 0 || Nout <= 0 || ldw < K || M < 0 || b0 < 0 || b1 < b0 || M < b1) return MRG_E_SHAPE;
  if (K <= 0 || Nout <= 48 || Nout % 4 != 0) return MRG_E_SHAPE;
  if (M == 0) return MRG_OK;
  if (!gY || !W_host || !gX) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  return bwd_input3(gY, nullptr, W_host, nullptr, gX, ws, b0, b1, M, K, Nout, ldw, accumulate, (hipStream_t)stream);
}

extern "C" int mrg_linear_bwd_input3_acc2(const float* gY, const float* const* W_host, float* gX, void* ws, int64_t b0, int64_t b1, int64_t M,
                                          int K, int Nout, int ldw, int accumulate, void* stream, const float* total) {
  if (K <= 0 || Nout <= 0 || ldw < K || M < 0 || b0 < 0 || b1 < b0 || M < b1) return MRG_E_SHAPE;
  if (K <= 0 || Nout <= 48 || Nout % 4 != 0) return MRG_E_SHAPE;
  if (M == 0) return MRG_OK;
  if (!gY || !W_host || !gX || !total) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  return bwd_input3(gY, nullptr, W_host, nullptr, gX, ws, b0, b1, M, K, Nout, ldw, accumulate, (hipStream_t)stream, total);
}

extern "C" int64_t mrg_linear_bwd_input3_pair_workspace_bytes(int K, int Nout) {
  if (K <= 0 || Nout <= 24 || Nout % 4 != 0 || gemm_mode() == 1) return 0;
  return 3 * (int64_t)bwd_input3_each(K, 2 * Nout);
}

extern "C" int mrg_linear_bwd_input3_pair(const float* gY1, const float* gY2, const float* const* W1_host, const float* const* W2_host, float* gX,
                                          void* ws, int64_t b0, int64_t b1, int64_t M, int K, int Nout, int ldw, int accumulate, void* stream) {
  if (K <= 0 || Nout <= 24 || Nout % 4 != 0 || ldw < K || M < 0 || b0 < 0 || b1 < b0 || M < b1) return MRG_E_SHAPE;
  if (M == 0) return MRG_OK;
  if (!gY1 || !gY2 || !W1_host || !W2_host || !gX) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  return bwd_input3(gY1, gY2, W1_host, W2_host, gX, ws, b0, b1, M, K, Nout, ldw, accumulate, (hipStream_t)stream);
}

extern "C" int mrg_linear_bwd_input3_pair_acc2(const float* gY1, const float* gY2, const float* const* W1_host, const float* const* W2_host, float* gX,
                                               void* ws, int64_t b0, int64_t b1, int64_t M, int K, int Nout, int ldw, int accumulate, void* stream,
                                               const float* total) {
  if (K <= 0 || Nout <= 24 || Nout % 4 != 0 || ldw < K || M < 0 || b0 < 0 || b1 < b0 || M < b1) return MRG_E_SHAPE;
  if (M == 0) return MRG_OK;
  if (!gY1 || !gY2 || !W1_host || !W2_host || !gX || !total) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  return bwd_input3(gY1, gY2, W1_host, W2_host, gX, ws, b0, b1, M, K, Nout, ldw, accumulate, (hipStream_t)stream, total);
}
