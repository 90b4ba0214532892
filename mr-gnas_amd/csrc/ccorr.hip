// Standalone circular correlation ccorr(a, b) (reference utils/utils.py:285-301, models/operations_lp.py:58-68) and its gradients.
//   CCORR: out[k] = sum_j x[j] * y[(j + k) % D]         CCONV: out[m] = sum_j x[j] * y[(m - j) % D]
// dL/da = ccorr(g, b), dL/db = cconv(a, g).  Two forms:
//   - ccorr_rows_k: one pair of rows per lane group, O(D^2) multiply-adds per row on the f32 vector pipe;
//   - a shared row (one operand broadcast over every row of the other) as a row GEMM on the matrix pipe: ccorr_matrix_k builds the
//     D x D circulant H(b)[k, j] = b[(j + k) % D] or T(a)[k, m] = a[(m - k) % D], mrg_linear_fwd multiplies, and ccorr_reduce_k folds
//     the D x D weight gradient back onto the shared row.
#include "common.hpp"

namespace mrg {

// A lane owns OUT = 8 consecutive outputs k0 .. k0+7 and slides a twelve-value register window over z (the ideas of gcs_corr8_k in
// fused_gcs.hip without its segment plans): one step of four j costs a broadcast ds_read_b128 of x and a ds_read_b128 of the next four
// window values for thirty-two multiply-adds.  z = y stored twice (z | z: no modulo), index-reversed for CCONV (z[m] = y[(D - m) % D],
// so conv(x, y)[k] = corr(x, z)[(D - k) % D] and only the final store permutes).  x is zero past D up to the lanes' reach and z is zero
// past 2 D, so any D works: the terms j >= D are 0 * finite, the outputs k >= D of a partial last lane are never stored.
// LPR lanes per row cover D <= 8 LPR; every block holds 24 KB of LDS whatever LPR is.  Every output's sum runs over j ascending.
template <int LPR, int MODE>
__global__ __launch_bounds__(MRG_BLOCK) void ccorr_rows_k(const float* __restrict__ X, const float* __restrict__ Y, float* __restrict__ out,
                                                          int64_t N, int D, int vec4) {
  constexpr int OUT = 8, RPB = MRG_BLOCK / LPR;
  constexpr int XW = LPR * OUT, ZW = 2 * XW;                // reads reach z[8 dl + d4 - 1] <= z[2 XW - 1]
  __shared__ __align__(16) float lds[RPB * (XW + ZW)];
  const int sl = threadIdx.x % LPR, rw = row_group_of_thread<LPR>();
  const int dl = (D + OUT - 1) / OUT, d4 = (D + 3) & ~3;   // lanes of a row that own outputs, x length the loop walks
  float* lx = lds + rw * (XW + ZW);
  float* lz = lx + XW;
  for (int64_t row = (int64_t)blockIdx.x * RPB + rw; row < N; row += (int64_t)gridDim.x * RPB) {
    const float* xr = X + row * D;
    const float* yr = Y + row * D;
    __threadfence_block();                                  // earlier reads of lx / lz by this lane group are done
    __builtin_amdgcn_wave_barrier();
    if (vec4) {                                             // D % 4 == 0 and 16-byte aligned rows
      for (int c = sl; c < (D >> 2); c += LPR) {
        const float4 a = *reinterpret_cast<const float4*>(xr + c * 4), b = *reinterpret_cast<const float4*>(yr + c * 4);
        *reinterpret_cast<float4*>(lx + c * 4) = a;
        if (MODE == MRG_CCORR) {
          *reinterpret_cast<float4*>(lz + c * 4) = b;
          *reinterpret_cast<float4*>(lz + D + c * 4) = b;
        } else {
          const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = (c * 4 + i) == 0 ? 0 : D - (c * 4 + i);
            lz[m] = bb[i];
            lz[D + m] = bb[i];
          }
        }
      }
      for (int m = D + sl; m < XW; m += LPR) lx[m] = 0.f;
    } else {
      for (int m = sl; m < XW; m += LPR) lx[m] = m < D ? xr[m] : 0.f;
      for (int m = sl; m < D; m += LPR) {
        const float b = yr[m];
        const int zi = (MODE == MRG_CCORR || m == 0) ? m : D - m;
        lz[zi] = b;
        lz[D + zi] = b;
      }
    }
    for (int m = 2 * D + sl; m < ZW; m += LPR) lz[m] = 0.f;
    __threadfence_block();                                  // the group's rows are in LDS before anyone reads them
    __builtin_amdgcn_wave_barrier();
    if (sl < dl) {
      const float* zp = lz + sl * OUT;
      float w[OUT + 4];
#pragma unroll
      for (int q = 0; q < OUT; q += 4) {
        const float4 t = *reinterpret_cast<const float4*>(zp + q);
        w[q] = t.x; w[q + 1] = t.y; w[q + 2] = t.z; w[q + 3] = t.w;
      }
      float p[OUT];
#pragma unroll
      for (int q = 0; q < OUT; ++q) p[q] = 0.f;
#pragma unroll 10
      for (int i = 0; i < d4; i += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(lx + i);
        const float4 wn = *reinterpret_cast<const float4*>(zp + i + OUT);
        w[OUT] = wn.x; w[OUT + 1] = wn.y; w[OUT + 2] = wn.z; w[OUT + 3] = wn.w;
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int q = 0; q < OUT; ++q) p[q] += xs[t] * w[t + q];
#pragma unroll
        for (int q = 0; q < OUT; ++q) w[q] = w[q + 4];
      }
      float* dst = out + row * D;
      const int k0 = sl * OUT;
      if (MODE == MRG_CCORR && vec4) {
#pragma unroll
        for (int q = 0; q < OUT; q += 4)
          if (k0 + q < D) *reinterpret_cast<float4*>(dst + k0 + q) = make_float4(p[q], p[q + 1], p[q + 2], p[q + 3]);
      } else {
#pragma unroll
        for (int q = 0; q < OUT; ++q) {
          const int k = k0 + q;
          if (k < D) dst[(MODE == MRG_CCORR || k == 0) ? k : D - k] = p[q];
        }
      }
    }
  }
}

// W[k][j] = r[(j + k) % D] (MRG_CCORR_H) or r[(j - k) % D] (MRG_CCORR_T); one element per thread.
__global__ __launch_bounds__(MRG_BLOCK) void ccorr_matrix_k(const float* __restrict__ r, float* __restrict__ W, int D, int mode) {
  const int64_t idx = (int64_t)blockIdx.x * MRG_BLOCK + threadIdx.x;
  if (idx >= (int64_t)D * D) return;
  const int k = (int)(idx / D), j = (int)(idx - (int64_t)k * D);
  int s = mode == MRG_CCORR_H ? j + k : j - k;
  if (s >= D) s -= D;
  if (s < 0) s += D;
  W[idx] = r[s];
}

// gr[m] = sum over k of gW[k][(m - k) % D] (H: the wrapped anti-diagonal j + k = m) or gW[k][(k + m) % D] (T: the wrapped diagonal
// j - k = m).  A block owns 64 outputs; its four waves sum k over four consecutive quarters, ascending, and the quarters are added in
// order 0..3: a fixed order, bit-reproducible.  For fixed k the 64 lanes read 64 consecutive (wrapped) columns of row k.
__global__ __launch_bounds__(MRG_BLOCK) void ccorr_reduce_k(const float* __restrict__ gW, float* __restrict__ gr, int D, int mode) {
  constexpr int M = 64, P = MRG_BLOCK / M;
  __shared__ float part[P][M];
  const int ml = threadIdx.x % M, pq = threadIdx.x / M;
  const int m = blockIdx.x * M + ml;
  const int kc = (D + P - 1) / P;
  const int k0 = pq * kc, k1 = min(D, k0 + kc);
  float s = 0.f;
  if (m < D && k0 < k1) {
    int col = mode == MRG_CCORR_H ? m - k0 : m + k0;      // |k0| < D: one wrap at most
    if (col < 0) col += D;
    if (col >= D) col -= D;
    const float* rowp = gW + (int64_t)k0 * D;
    for (int k = k0; k < k1; ++k, rowp += D) {
      s += rowp[col];
      if (mode == MRG_CCORR_H) col = col == 0 ? D - 1 : col - 1;
      else col = col + 1 == D ? 0 : col + 1;
    }
  }
  part[pq][ml] = s;
  __syncthreads();
  if (pq == 0 && m < D) {
    float t = part[0][ml];
#pragma unroll
    for (int q = 1; q < P; ++q) t += part[q][ml];
    gr[m] = t;
  }
}

// Grid of ccorr_rows_k: one residency round of blocks (every block then walks the same number of row groups, +- 1), or fewer
// when there are fewer row groups.  Device attributes are cached per device; no stream work, so a captured launch is unaffected.
template <int LPR, int MODE>
static int rows_grid(int64_t N) {
  constexpr int RPB = MRG_BLOCK / LPR;
  static int cached[16][2] = {};                            // [device] = {CUs, blocks per CU}
  int dev = 0;
  (void)hipGetDevice(&dev);
  int cus = 256, per = 4;
  if (dev >= 0 && dev < 16) {
    if (cached[dev][0] == 0) {
      int c = 0, b = 0;
      if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<const void*>(&ccorr_rows_k<LPR, MODE>), MRG_BLOCK, 0) != hipSuccess || b <= 0) b = 4;
      cached[dev][0] = c;
      cached[dev][1] = b;
    }
    cus = cached[dev][0];
    per = cached[dev][1];
  }
  const int64_t groups = (N + RPB - 1) / RPB;
  const int64_t cap = (int64_t)cus * per;
  return (int)(groups < cap ? groups : cap);
}

template <int MODE>
static void launch_rows(const float* X, const float* Y, float* out, int64_t N, int D, int vec4, hipStream_t st) {
  if (D <= 64) hipLaunchKernelGGL((ccorr_rows_k<8, MODE>), dim3(rows_grid<8, MODE>(N)), dim3(MRG_BLOCK), 0, st, X, Y, out, N, D, vec4);
  else if (D <= 256) hipLaunchKernelGGL((ccorr_rows_k<32, MODE>), dim3(rows_grid<32, MODE>(N)), dim3(MRG_BLOCK), 0, st, X, Y, out, N, D, vec4);
  else hipLaunchKernelGGL((ccorr_rows_k<64, MODE>), dim3(rows_grid<64, MODE>(N)), dim3(MRG_BLOCK), 0, st, X, Y, out, N, D, vec4);
}

}  // namespace mrg

using namespace mrg;

extern "C" int mrg_ccorr_rows(int mode, const float* X, const float* Y, float* out, int64_t N, int D, void* stream) {
  if (mode != MRG_CCORR && mode != MRG_CCONV) return MRG_E_ENUM;
  if (N < 0 || D < 1 || D > MRG_CCORR_MAX_D) return MRG_E_SHAPE;
  if (N == 0) return MRG_OK;
  if (!X || !Y || !out) return MRG_E_NULLPTR;
  const int vec4 = D % 4 == 0 && aligned16(X) && aligned16(Y) && aligned16(out);
  hipStream_t st = (hipStream_t)stream;
  if (mode == MRG_CCORR) launch_rows<MRG_CCORR>(X, Y, out, N, D, vec4, st);
  else launch_rows<MRG_CCONV>(X, Y, out, N, D, vec4, st);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_ccorr_matrix(int mode, const float* r, float* W, int D, void* stream) {
  if (mode != MRG_CCORR_H && mode != MRG_CCORR_T) return MRG_E_ENUM;
  if (D < 1 || D > MRG_CCORR_MAX_D) return MRG_E_SHAPE;
  if (!r || !W) return MRG_E_NULLPTR;
  const int64_t n = (int64_t)D * D;
  hipLaunchKernelGGL(ccorr_matrix_k, dim3((unsigned)((n + MRG_BLOCK - 1) / MRG_BLOCK)), dim3(MRG_BLOCK), 0, (hipStream_t)stream, r, W, D, mode);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_ccorr_matrix_grad(int mode, const float* gW, float* gr, int D, void* stream) {
  if (mode != MRG_CCORR_H && mode != MRG_CCORR_T) return MRG_E_ENUM;
  if (D < 1 || D > MRG_CCORR_MAX_D) return MRG_E_SHAPE;
  if (!gW || !gr) return MRG_E_NULLPTR;
  hipLaunchKernelGGL(ccorr_reduce_k, dim3((D + 63) / 64), dim3(MRG_BLOCK), 0, (hipStream_t)stream, gW, gr, D, mode);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}
