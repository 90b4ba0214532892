// The candidate Linears of one node-classification MixedOp in one launch (reference models/cell.py:17-31): up to four members of
// the same rows and the same square D,
//   forward          Y[k]  = X[k]  W[k]^T + bias[k]     (+ the float64 column sums of Y[k] for the BatchNorm that reads it)
//   input gradient   gX[k] = gY[k] W[k]                 (the same product, the weight read through transposed strides)
//
// Which matrix core, and why.  At the reference's default feature_dim = 64 the product has 2 D = 128 flop per 8 bytes of its own
// traffic: 16 flop / byte.  The exact-f32 core (v_mfma_f32_32x32x2_f32, 64 cycles per instruction per SIMD, 157 TF/s chip peak)
// then keeps up with 9.8 TB/s of activation traffic, above what HBM delivers (8 TB/s peak); at D = 128 with 4.9 TB/s, about the
// rate a streaming kernel reaches.  So up to D = 128 the f32 pipe is not the bound, and it needs what the split-bf16 core does not
// have for free here: no pre-split weight in global memory (no workspace, no split launch in front of every one of the 22 MixedOps
// of a cell) and no VALU work per activation element.  Beyond D = 128 the matrix time would exceed the memory time and the shape
// is left to the row GEMM (mrg_linear_fwd), whose split core is built for it.
//
// Geometry.  A workgroup of four waves owns 256 rows of ONE member (blockIdx.y): wave w owns the 32-row strips w and w + 4.
// The member's weight is staged once per workgroup in LDS as Wl[j][k] = B(k, j) (j: output column, k: reduction index), rows padded
// to LD = round8(D) + 4 floats: LD = 4 (mod 8), so the 16 lanes that one ds_read_b128 cycle serves fall on 16 distinct 16-byte
// slots of the bank row (MI355X_MICROARCH.md, LDS: lane groups of ds_read_b128; an odd multiple of 4 banks per lane).
// A lane (li = lane % 32, lh = lane / 32) reads the whole activation row of its strip as 16-byte loads: chunk c holds
// k = 8 c + 4 lh + {0..3}.  One MFMA step multiplies k = 8 c + i of the lower half wave with k = 8 c + 4 + i of the upper one
// (i = 0..3: the .x .y .z .w of the two 16-byte fragments) -- the order of k inside a chunk is permuted the same way for both
// operands, the order rowgemm_dma_k (gemm.hpp) uses.  All loads of a strip are in flight before its first MFMA; two to four
// workgroups per CU overlap one strip's loads with another's matrix work.
// Accumulator map of a 32 x 32 tile: column li, row (reg & 3) + 8 (reg >> 2) + 4 lh.  The epilogue adds the bias and stores in
// accumulator order (one store = two 128-byte row pieces); with SUMS a lane also adds the values it stores -- valid rows, register
// order, converted to double -- and the workgroup adds its eight (wave, half) slots through LDS in slot order: bitwise reproducible.
#include "x3_parts.hpp"     // launch_kernel; gemm.hpp for the accumulator type

namespace mrg {

constexpr int CAND_MAX = 4;            // members per launch
constexpr int CAND_GBM = 256;          // rows per workgroup: 4 waves x 2 strips of 32
constexpr int CAND_D_MIN = 16, CAND_D_MAX = 128;

struct CandArgs {
  const float* X[CAND_MAX];
  const float* W[CAND_MAX];
  const float* bias[CAND_MAX];
  float* Y[CAND_MAX];
  double* colsum;                      // [n][gridDim.x][2][D] or NULL
  int64_t rows;
  int D;
};

inline bool cand_shape_ok(int D) { return D >= CAND_D_MIN && D <= CAND_D_MAX && D % 4 == 0; }
inline int cand_ld(int D) { return ((D + 7) / 8) * 8 + 4; }
inline size_t cand_lds_bytes(int D) {
  const int nt = (D + 31) / 32;
  const size_t w = (size_t)nt * 32 * cand_ld(D) * sizeof(float), s = (size_t)8 * 2 * nt * 32 * sizeof(double);
  return w > s ? w : s;
}

#define CAND_PICK(F, m) ((m) == 0 ? a.F[0] : ((m) == 1 ? a.F[1] : ((m) == 2 ? a.F[2] : a.F[3])))

// NT: column tiles of 32 (D <= 32 NT);  TRANS: B(k, j) = W[k][j] (input gradient) instead of W[j][k] (forward);  SUMS: column sums
template <int NT, bool TRANS, bool SUMS>
__global__ __launch_bounds__(MRG_BLOCK) void cand_linear_k(CandArgs a) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = blockIdx.y;
  const float* __restrict__ X = CAND_PICK(X, m);
  const float* __restrict__ W = CAND_PICK(W, m);
  const float* __restrict__ bias = CAND_PICK(bias, m);
  float* __restrict__ Y = CAND_PICK(Y, m);
  const int D = a.D;
  const int64_t rows = a.rows;
  const int Kp = ((D + 7) >> 3) << 3, LD = Kp + 4, kc = Kp >> 3;
  constexpr int DP = NT * 32;

  // ---- the weight image: Wl[j][k], zero beyond D in both directions
  if constexpr (!TRANS) {
    const int kq = Kp >> 2;
    for (int idx = tid; idx < DP * kq; idx += MRG_BLOCK) {
      const int j = idx / kq, k = (idx - j * kq) << 2;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < D && k < D) v = *reinterpret_cast<const float4*>(W + (int64_t)j * D + k);      // D % 4 == 0: k < D means k + 4 <= D
      *reinterpret_cast<float4*>(smem + j * LD + k) = v;
    }
  } else {
    constexpr int JQ = DP >> 2;
    for (int idx = tid; idx < Kp * JQ; idx += MRG_BLOCK) {
      const int k = idx / JQ, j = (idx - k * JQ) << 2;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < D && j < D) v = *reinterpret_cast<const float4*>(W + (int64_t)k * D + j);
      smem[(j + 0) * LD + k] = v.x; smem[(j + 1) * LD + k] = v.y; smem[(j + 2) * LD + k] = v.z; smem[(j + 3) * LD + k] = v.w;
    }
  }
  __syncthreads();

  double s1[NT], s2[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) { s1[n] = 0.0; s2[n] = 0.0; }

  const int64_t row0 = (int64_t)blockIdx.x * CAND_GBM;
  const float* Wl = smem + li * LD + lh * 4;
#pragma unroll 1
  for (int s = 0; s < 2; ++s) {
    const int64_t rowbase = row0 + (int64_t)(s * 4 + wave) * 32;
    if (rowbase >= rows) break;                              // wave-uniform; the second strip lies behind the first
    // ---- this lane's activation row: every 16-byte fragment in flight before the first MFMA
    const int64_t row = rowbase + li;
    const float* __restrict__ xr = X + (row < rows ? row : rows - 1) * D;
    float4 af[NT * 4];
#pragma unroll
    for (int c = 0; c < NT * 4; ++c) {
      af[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < kc) {
        const int k = 8 * c + 4 * lh;
        const float4 v = *reinterpret_cast<const float4*>(xr + (k < D ? k : 0));
        if (k < D) af[c] = v;                                // D % 8 == 4: the upper half of the last chunk is beyond the row
      }
    }
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
#pragma unroll
    for (int c = 0; c < NT * 4; ++c) {
      if (c < kc) {
        float4 bf[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) bf[n] = *reinterpret_cast<const float4*>(Wl + n * 32 * LD + 8 * c);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c].x, bf[n].x, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c].y, bf[n].y, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c].z, bf[n].z, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c].w, bf[n].w, acc[n], 0, 0, 0);
      }
    }
    // ---- epilogue: bias, store in accumulator order, column sums of what is stored
    const bool full = rowbase + 32 <= rows;                  // wave-uniform
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int col = n * 32 + li;
      const bool cok = col < D;
      const float bv = (bias && cok) ? bias[col] : 0.f;
      float* __restrict__ yp = Y + (rowbase + 4 * lh) * D + (cok ? col : 0);
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = acc[n][r] + bv;
      if (full) {
        if (cok) {
#pragma unroll
          for (int r = 0; r < 16; ++r) yp[(int64_t)((r & 3) + 8 * (r >> 2)) * D] = v[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = (r & 3) + 8 * (r >> 2);
          if (cok && rowbase + 4 * lh + rr < rows) yp[(int64_t)rr * D] = v[r];
        }
      }
      if constexpr (SUMS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = (r & 3) + 8 * (r >> 2);
          const double d = (cok && (full || rowbase + 4 * lh + rr < rows)) ? (double)v[r] : 0.0;
          s1[n] += d; s2[n] += d * d;
        }
      }
    }
  }

  if constexpr (SUMS) {
    __syncthreads();                                         // every wave has read its last weight fragment: the image is dead
    double* __restrict__ sl = reinterpret_cast<double*>(smem);
    const int slot = wave * 2 + lh;                          // [8 slots][2][DP]
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      sl[(slot * 2 + 0) * DP + n * 32 + li] = s1[n];
      sl[(slot * 2 + 1) * DP + n * 32 + li] = s2[n];
    }
    __syncthreads();
    double* __restrict__ dst = a.colsum + ((int64_t)m * gridDim.x + blockIdx.x) * 2 * D;
    for (int t = tid; t < 2 * D; t += MRG_BLOCK) {
      const int which = t / D, c = t - which * D;
      double tot = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) tot += sl[(q * 2 + which) * DP + c];
      dst[which * D + c] = tot;
    }
  }
}

template <bool TRANS, bool SUMS>
static int cand_launch(const CandArgs& a, int n, hipStream_t st) {
  const dim3 grid((unsigned)((a.rows + CAND_GBM - 1) / CAND_GBM), (unsigned)n);
  const size_t lds = cand_lds_bytes(a.D);
  switch ((a.D + 31) / 32) {
    case 1: return launch_kernel(cand_linear_k<1, TRANS, SUMS>, grid, dim3(MRG_BLOCK), lds, st, a);
    case 2: return launch_kernel(cand_linear_k<2, TRANS, SUMS>, grid, dim3(MRG_BLOCK), lds, st, a);
    case 3: return launch_kernel(cand_linear_k<3, TRANS, SUMS>, grid, dim3(MRG_BLOCK), lds, st, a);
    default: return launch_kernel(cand_linear_k<4, TRANS, SUMS>, grid, dim3(MRG_BLOCK), lds, st, a);
  }
}

// Argument checks shared by the two entry points; fills `a`.  Returns MRG_OK, or the code to return (1: nothing to do).
static int cand_args(CandArgs& a, int n, const float* const* X, const float* const* W, const float* const* bias, float* const* Y,
                     void* ws, int64_t rows, int D) {
  if (!X || !W || !Y) return MRG_E_NULLPTR;
  if (n < 1 || n > CAND_MAX || rows < 0 || D <= 0) return MRG_E_SHAPE;
  for (int k = 0; k < n; ++k)
    if (!X[k] || !W[k] || !Y[k]) return MRG_E_NULLPTR;
  if (!cand_shape_ok(D) || (rows + CAND_GBM - 1) / CAND_GBM > 0x7fffffffLL) return MRG_E_SHAPE;
  if (mrg_cand_linear_workspace_bytes(n, D) > 0 && !ws) return MRG_E_WORKSPACE;
  a = CandArgs{};
  for (int k = 0; k < CAND_MAX; ++k) {                       // unused slots repeat member 0: every pointer of the block is valid
    const int q = k < n ? k : 0;
    a.X[k] = X[q]; a.W[k] = W[q]; a.bias[k] = bias ? bias[q] : nullptr; a.Y[k] = Y[q];
    if (!aligned16(a.X[k]) || !aligned16(a.W[k]) || !aligned16(a.Y[k]) || !aligned16(a.bias[k])) return MRG_E_SHAPE;
  }
  a.rows = rows; a.D = D;
  return rows == 0 ? 1 : MRG_OK;
}

}  // namespace mrg

extern "C" int64_t mrg_cand_linear_colsum_blocks(int64_t rows, int D) {
  if (rows <= 0 || !mrg::cand_shape_ok(D)) return 0;
  return (rows + mrg::CAND_GBM - 1) / mrg::CAND_GBM;
}

extern "C" int64_t mrg_cand_linear_workspace_bytes(int n, int D) {
  (void)n; (void)D;
  return 0;                                                   // the weight image lives in LDS
}

extern "C" int mrg_cand_linear_fwd(int n, const float* const* X, const float* const* W, const float* const* bias, float* const* Y,
                                   void* ws, int64_t rows, int D, void* stream, double* colsum, int64_t colsum_blocks) {
  mrg::CandArgs a;
  const int rc = mrg::cand_args(a, n, X, W, bias, Y, ws, rows, D);
  if (rc != MRG_OK) return rc == 1 ? MRG_OK : rc;
  if (colsum && (colsum_blocks != mrg_cand_linear_colsum_blocks(rows, D) || !mrg::aligned16(colsum))) return MRG_E_SHAPE;
  a.colsum = colsum;
  hipStream_t st = (hipStream_t)stream;
  return colsum ? mrg::cand_launch<false, true>(a, n, st) : mrg::cand_launch<false, false>(a, n, st);
}

extern "C" int mrg_cand_linear_bwd_input(int n, const float* const* gY, const float* const* W, float* const* gX, void* ws,
                                         int64_t rows, int D, void* stream) {
  mrg::CandArgs a;
  const int rc = mrg::cand_args(a, n, gY, W, nullptr, gX, ws, rows, D);
  if (rc != MRG_OK) return rc == 1 ? MRG_OK : rc;
  return mrg::cand_launch<true, false>(a, n, (hipStream_t)stream);
}
