// ConvE feature path (reference models/operations_lp.py:150-205 sf_ConvE_op, models/compgcn.py:188-269 CompGCN_ConvE): from the
// (subject, relation) rows to the hidden vector h [B, D] in front of BN2, forward and backward.
//
//   img = layout(sub, rel) [B, 1, Hi, Wi]      x0 = BN0(img)      z = conv(x0, Wc) + bc  [B, F, Ho, Wo]
//   a   = keep1 * relu(BN1(z))                  h  = keep2 * (a.view(B, K) Wfc^T + bfc),   K = F Ho Wo
//
// Forward, five launches: conve_bn0_stats_k (one workgroup), conve_conv_fwd_k (image x filter chunk, the BN0-normalised image and
// the filter chunk staged in LDS, 4 x 4 outputs per lane on f32 FMA), conve_bn1_fwd_k (one workgroup per filter: statistics, running
// update and the BN1 / ReLU / keep1 apply), conve_gemm_k split over K (the short, deep fc product) and conve_fc_reduce_k (the split
// partials in order, + bfc, * keep2).  Backward, six: conve_fc_gpre_k (keep2 and the bias gradient), conve_gemm_k twice (dL/da and
// dL/dWfc), conve_bn1_bwd_k (one workgroup per filter), conve_conv_bwd_k (per-image transposed conv with the BN0 partial sums, and
// conve weight-gradient slabs over image ranges, in one grid) and conve_finish_k (BN0 backward, the scatter to dL/dsub and dL/drel by
// layout, the weight-gradient slabs in order).  Every sum runs in a fixed order (no atomics): two runs give the same bits.
// Arithmetic is f32 FMA throughout; BatchNorm statistics and their gradient sums accumulate in float64.
#include "common.hpp"

namespace mrg {

constexpr int CV_LDS_FLOATS = 14336;   // dynamic LDS per workgroup (56 KB; with the 2 KB reduction array, under 64 KB)
constexpr int CV_GEMM_T = 64, CV_GEMM_BK = 16;
constexpr int CV_WG_FILTERS = 32;      // filters per weight-gradient workgroup: 4 waves x 8
constexpr int CV_MAX_PJ = 8;           // pixels per lane of the input gradient: 2 D <= 8 * 256

__device__ __forceinline__ float conve_pixel(const float* __restrict__ sub, const float* __restrict__ rel, int64_t b, int D, int t, int layout) {
  if (layout == MRG_CONVE_STACKED) return t < D ? sub[b * D + t] : rel[b * D + t - D];
  return (t & 1) ? rel[b * D + (t >> 1)] : sub[b * D + (t >> 1)];
}

// Sum over the workgroup in a fixed tree order; every thread receives the result.
template <int NT>
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------
// BN0 over all 2 B D values: two passes (mean, then the centred sum of squares), float64.  stats0 = {mean, invstd}.
__global__ __launch_bounds__(1024) void conve_bn0_stats_k(const float* __restrict__ sub, const float* __restrict__ rel, int64_t nh,
                                                          float* __restrict__ rm, float* __restrict__ rv, int training, float eps,
                                                          float mom, float* __restrict__ stats0) {
  __shared__ double red[1024];
  if (!training) {
    if (threadIdx.x == 0) {
      stats0[0] = rm[0];
      stats0[1] = (float)(1.0 / sqrt((double)rv[0] + (double)eps));
    }
    return;
  }
  const int64_t n = 2 * nh;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nh; i += 1024) s += (double)sub[i];
  for (int64_t i = threadIdx.x; i < nh; i += 1024) s += (double)rel[i];
  const double mean = block_sum_d<1024>(s, red) / (double)n;
  double q = 0.0;
  for (int64_t i = threadIdx.x; i < nh; i += 1024) { const double d = (double)sub[i] - mean; q += d * d; }
  for (int64_t i = threadIdx.x; i < nh; i += 1024) { const double d = (double)rel[i] - mean; q += d * d; }
  const double var = block_sum_d<1024>(q, red) / (double)n;
  if (threadIdx.x == 0) {
    stats0[0] = (float)mean;
    stats0[1] = (float)(1.0 / sqrt(var + (double)eps));
    if (rm) rm[0] = (float)((1.0 - mom) * rm[0] + mom * mean);
    if (rv) rv[0] = (float)((1.0 - mom) * rv[0] + mom * var * (double)n / (double)(n - 1));
  }
}

// z for one image and a chunk of FC filters.  LDS: the BN0-normalised image [Hi][Wi], the chunk's filters [FC][ks][ks] and biases.
// A lane owns 4 filters x 4 consecutive output positions: per tap 4 image and 4 (wave-broadcast) weight reads for 16 FMA.
__global__ __launch_bounds__(MRG_BLOCK) void conve_conv_fwd_k(int layout, const float* __restrict__ sub, const float* __restrict__ rel,
                                                              int D, int Wi, const float* __restrict__ stats0, const float* __restrict__ w0,
                                                              const float* __restrict__ b0, const float* __restrict__ Wc,
                                                              const float* __restrict__ bc, int F, int ks, int FC, int Wo, int P,
                                                              float* __restrict__ z) {
  extern __shared__ float lds[];
  const int64_t b = blockIdx.x;
  const int f0 = blockIdx.y * FC, fc = min(FC, F - f0), ks2 = ks * ks, n2 = 2 * D;
  float* img = lds;
  float* wl = img + n2;
  float* bl = wl + FC * ks2;
  const float mean = stats0[0], invstd = stats0[1], g0 = w0[0], be0 = b0[0];
  for (int t = threadIdx.x; t < n2; t += MRG_BLOCK) img[t] = (conve_pixel(sub, rel, b, D, t, layout) - mean) * invstd * g0 + be0;
  for (int i = threadIdx.x; i < fc * ks2; i += MRG_BLOCK) wl[i] = Wc[(int64_t)f0 * ks2 + i];
  for (int i = threadIdx.x; i < fc; i += MRG_BLOCK) bl[i] = bc ? bc[f0 + i] : 0.f;
  __syncthreads();
  const int fg = (fc + 3) / 4, pg = (P + 3) / 4;
  float* zb = z + (b * F + f0) * (int64_t)P;
  for (int it = threadIdx.x; it < fg * pg; it += MRG_BLOCK) {
    const int fi = it / pg, pi = it - fi * pg;             // consecutive lanes: consecutive positions of the same four filters
    int base[4], wrow[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = min(pi * 4 + q, P - 1);
      const int oy = p / Wo;
      base[q] = oy * Wi + (p - oy * Wo);
      wrow[q] = min(fi * 4 + q, fc - 1) * ks2;
    }
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[r][q] = 0.f;
    for (int ky = 0; ky < ks; ++ky) {
      for (int kx = 0; kx < ks; ++kx) {
        const int toff = ky * Wi + kx, tap = ky * ks + kx;
        float x[4], w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = img[base[q] + toff];
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = wl[wrow[r] + tap];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[r][q] = fmaf(w[r], x[q], acc[r][q]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = fi * 4 + r;
      if (f >= fc) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = pi * 4 + q;
        if (p < P) zb[(int64_t)f * P + p] = acc[r][q] + bl[f];
      }
    }
  }
}

// One workgroup per filter f over its B x P values: batch statistics (training) or the running ones, the running update, then
// a = keep1 * relu((z - mean) * invstd * w + b).  stats1 = {mean [F], invstd [F]}.
__global__ __launch_bounds__(MRG_BLOCK) void conve_bn1_fwd_k(const float* __restrict__ z, int B, int F, int P, const float* __restrict__ w1,
                                                             const float* __restrict__ b1, float* __restrict__ rm, float* __restrict__ rv,
                                                             const float* __restrict__ keep1, int training, float eps, float mom,
                                                             float* __restrict__ stats1, float* __restrict__ a) {
  __shared__ double red[MRG_BLOCK];
  const int f = blockIdx.x;
  const int n = B * P;
  const int64_t K = (int64_t)F * P;
  const float* zf = z + (int64_t)f * P;
  float mean, invstd;
  if (training) {
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += MRG_BLOCK) {
      const int bb = e / P;
      s += (double)zf[bb * K + (e - bb * P)];
    }
    const double m = block_sum_d<MRG_BLOCK>(s, red) / (double)n;
    double q = 0.0;
    for (int e = threadIdx.x; e < n; e += MRG_BLOCK) {
      const int bb = e / P;
      const double d = (double)zf[bb * K + (e - bb * P)] - m;
      q += d * d;
    }
    const double var = block_sum_d<MRG_BLOCK>(q, red) / (double)n;
    mean = (float)m;
    invstd = (float)(1.0 / sqrt(var + (double)eps));
    if (threadIdx.x == 0) {
      if (rm) rm[f] = (float)((1.0 - mom) * rm[f] + mom * m);
      if (rv) rv[f] = (float)((1.0 - mom) * rv[f] + mom * var * (double)n / (double)(n - 1));
    }
  } else {
    mean = rm[f];
    invstd = (float)(1.0 / sqrt((double)rv[f] + (double)eps));
  }
  if (threadIdx.x == 0) {
    stats1[f] = mean;
    stats1[F + f] = invstd;
  }
  const float g = w1[f], be = b1[f];
  for (int e = threadIdx.x; e < n; e += MRG_BLOCK) {
    const int bb = e / P;
    const int64_t idx = bb * K + (int64_t)f * P + (e - bb * P);
    const float y = (z[idx] - mean) * invstd * g + be;
    float v = y > 0.f ? y : 0.f;
    if (keep1) v *= keep1[idx];
    a[idx] = v;
  }
}

// C_s[m][n] = sum over k in split s of A(m, k) Bm(k, n), A(m, k) = A[m sam + k sak], Bm(k, n) = Bp[k sbk + n sbn].  64 x 64 tile,
// 16-deep LDS stages, 4 x 4 outputs per lane, every output an f32 FMA chain over k ascending.  A_KC: A is contiguous along k (else
// along m); B_NC: Bm is contiguous along n (else along k) -- the global loads of a stage walk the contiguous dimension.
// Split s writes C + s M N; the k range of split s is [s kc, min(K, (s + 1) kc)).
template <bool A_KC, bool B_NC>
__global__ __launch_bounds__(MRG_BLOCK) void conve_gemm_k(const float* __restrict__ A, int64_t sam, int64_t sak, const float* __restrict__ Bp,
                                                          int64_t sbk, int64_t sbn, float* __restrict__ C, int M, int N, int K, int kc) {
  constexpr int T = CV_GEMM_T, BK = CV_GEMM_BK, LD = T + 4;
  __shared__ __align__(16) float As[BK][LD];
  __shared__ __align__(16) float Bs[BK][LD];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int m0 = blockIdx.y * T, n0 = blockIdx.x * T;
  const int kb = blockIdx.z * kc, ke = min(K, kb + kc);
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = kb; k0 < ke; k0 += BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + MRG_BLOCK * i;
      const int mm = A_KC ? e / BK : e % T, ka = A_KC ? e % BK : e / T;
      const int m = m0 + mm, k = k0 + ka;
      As[ka][mm] = (m < M && k < ke) ? A[(int64_t)m * sam + (int64_t)k * sak] : 0.f;
      const int nn = B_NC ? e % T : e / BK, kq = B_NC ? e / T : e % BK;
      const int n = n0 + nn, k2 = k0 + kq;
      Bs[kq][nn] = (n < N && k2 < ke) ? Bp[(int64_t)k2 * sbk + (int64_t)n * sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      const float4 av = *reinterpret_cast<const float4*>(&As[kk][ty * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&Bs[kk][tx * 4]);
      const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], br[j], acc[i][j]);
    }
    __syncthreads();
  }
  float* Cs = C + (int64_t)blockIdx.z * M * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty * 4 + i;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx * 4 + j;
      if (n < N) Cs[(int64_t)m * N + n] = acc[i][j];
    }
  }
}

// h = keep2 * (bfc + sum over s ascending of the split partials).
__global__ __launch_bounds__(MRG_BLOCK) void conve_fc_reduce_k(const float* __restrict__ part, int S, const float* __restrict__ bfc,
                                                               const float* __restrict__ keep2, float* __restrict__ h, int64_t MN, int N) {
  const int64_t i = (int64_t)blockIdx.x * MRG_BLOCK + threadIdx.x;
  if (i >= MN) return;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += part[s * MN + i];
  if (bfc) v += bfc[i % N];
  if (keep2) v *= keep2[i];
  h[i] = v;
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// gpre = gh * keep2 and gbfc[n] = sum over b of gpre[b][n]: 64 columns x 4 row quarters per workgroup, the quarters added in order.
__global__ __launch_bounds__(MRG_BLOCK) void conve_fc_gpre_k(const float* __restrict__ gh, const float* __restrict__ keep2, float* __restrict__ gpre,
                                                             float* __restrict__ gbfc, int B, int D) {
  __shared__ double part[4][64];
  const int c = threadIdx.x % 64, r = threadIdx.x / 64;
  const int n = blockIdx.x * 64 + c;
  double s = 0.0;
  if (n < D) {
    for (int b = r; b < B; b += 4) {
      const int64_t i = (int64_t)b * D + n;
      const float v = keep2 ? gh[i] * keep2[i] : gh[i];
      gpre[i] = v;
      s += (double)v;
    }
  }
  part[r][c] = s;
  __syncthreads();
  if (r == 0 && n < D && gbfc) gbfc[n] = (float)(part[0][c] + part[1][c] + part[2][c] + part[3][c]);
}

// One workgroup per filter.  In: ga = dL/da; out (in place): dL/dz.  gy = a > 0 ? ga * keep1 : 0 (a = keep1 * relu(y) is positive
// exactly where the ReLU passed and the mask kept); gw1 = sum gy xhat, gb1 = sum gy; training: dz = w invstd (gy - gb1 / n - xhat gw1 / n),
// eval: dz = w invstd gy.
__global__ __launch_bounds__(MRG_BLOCK) void conve_bn1_bwd_k(float* __restrict__ g, const float* __restrict__ z, const float* __restrict__ a,
                                                             const float* __restrict__ keep1, const float* __restrict__ stats1,
                                                             const float* __restrict__ w1, int training, int B, int F, int P,
                                                             float* __restrict__ gw1, float* __restrict__ gb1) {
  __shared__ double red[MRG_BLOCK];
  const int f = blockIdx.x;
  const int n = B * P;
  const int64_t K = (int64_t)F * P, fo = (int64_t)f * P;
  const float mean = stats1[f], invstd = stats1[F + f], w = w1[f];
  double s1 = 0.0, s2 = 0.0;
  for (int e = threadIdx.x; e < n; e += MRG_BLOCK) {
    const int bb = e / P;
    const int64_t idx = bb * K + fo + (e - bb * P);
    const float gy = a[idx] > 0.f ? (keep1 ? g[idx] * keep1[idx] : g[idx]) : 0.f;
    const float xh = (z[idx] - mean) * invstd;
    s1 += (double)gy;
    s2 += (double)gy * (double)xh;
  }
  const double S1 = block_sum_d<MRG_BLOCK>(s1, red), S2 = block_sum_d<MRG_BLOCK>(s2, red);
  if (threadIdx.x == 0) {
    gw1[f] = (float)S2;
    gb1[f] = (float)S1;
  }
  const float c0 = w * invstd, m1 = training ? (float)(S1 / n) : 0.f, m2 = training ? (float)(S2 / n) : 0.f;
  for (int e = threadIdx.x; e < n; e += MRG_BLOCK) {
    const int bb = e / P;
    const int64_t idx = bb * K + fo + (e - bb * P);
    const float gy = a[idx] > 0.f ? (keep1 ? g[idx] * keep1[idx] : g[idx]) : 0.f;
    const float xh = (z[idx] - mean) * invstd;
    g[idx] = c0 * (gy - m1 - xh * m2);
  }
}

struct ConvBwdArgs {
  int layout;
  const float* sub;
  const float* rel;
  int B, D, Hi, Wi, F, ks, Ho, Wo, P;
  const float* stats0;
  const float* w0;
  const float* b0;
  const float* Wc;
  const float* gz;
  float* gx0;       // [B][2D]
  double* slab0;    // [B][2]: per image sum g_x0, sum g_x0 xhat0
  double* slabw;    // [BS][F][ks2 + 1]: per image range, the filter taps' gradient and the bias gradient
  int FCI;          // filters per LDS stage of the input gradient
  int BPB;          // images per weight-gradient workgroup
  int NFC;          // filter chunks of the weight gradient
  int PC;           // positions per LDS stage of the weight gradient
};

// dL/dx0 of image b: a lane owns pixels t = tid + 256 j; per filter of the LDS stage it walks the taps whose output lies inside
// the Ho x Wo grid (the weight reads are wave-broadcast).  Then the BN0 partial sums of the image.
__device__ void conve_igrad(const ConvBwdArgs& p, float* lds, double* red, int b) {
  const int ks2 = p.ks * p.ks, n2 = 2 * p.D;
  float* wl = lds;
  float* gl = lds + p.FCI * ks2;
  double acc[CV_MAX_PJ];                                  // per pixel: an f32 sum per filter, added in float64 over the F filters
#pragma unroll
  for (int j = 0; j < CV_MAX_PJ; ++j) acc[j] = 0.0;
  const float* gzb = p.gz + (int64_t)b * p.F * p.P;
  for (int f0 = 0; f0 < p.F; f0 += p.FCI) {
    const int fc = min(p.FCI, p.F - f0);
    for (int i = threadIdx.x; i < fc * ks2; i += MRG_BLOCK) wl[i] = p.Wc[(int64_t)f0 * ks2 + i];
    for (int i = threadIdx.x; i < fc * p.P; i += MRG_BLOCK) gl[i] = gzb[(int64_t)f0 * p.P + i];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CV_MAX_PJ; ++j) {
      const int t = threadIdx.x + MRG_BLOCK * j;
      if (t < n2) {
        const int iy = t / p.Wi, ix = t - iy * p.Wi;
        const int ky0 = max(0, iy - p.Ho + 1), ky1 = min(p.ks - 1, iy);
        const int kx0 = max(0, ix - p.Wo + 1), kx1 = min(p.ks - 1, ix);
        double sd = acc[j];
        for (int fl = 0; fl < fc; ++fl) {
          const float* wf = wl + fl * ks2;
          const float* gf = gl + fl * p.P;
          float s = 0.f;
          for (int ky = ky0; ky <= ky1; ++ky) {
            const int orow = (iy - ky) * p.Wo + ix;
            for (int kx = kx0; kx <= kx1; ++kx) s = fmaf(gf[orow - kx], wf[ky * p.ks + kx], s);
          }
          sd += (double)s;
        }
        acc[j] = sd;
      }
    }
    __syncthreads();
  }
  const float mean = p.stats0[0], invstd = p.stats0[1];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int j = 0; j < CV_MAX_PJ; ++j) {
    const int t = threadIdx.x + MRG_BLOCK * j;
    if (t < n2) {
      const float gv = (float)acc[j];
      p.gx0[(int64_t)b * n2 + t] = gv;
      const float xh = (conve_pixel(p.sub, p.rel, b, p.D, t, p.layout) - mean) * invstd;
      s1 += (double)gv;
      s2 += (double)gv * (double)xh;
    }
  }
  s1 = block_sum_d<MRG_BLOCK>(s1, red);
  s2 = block_sum_d<MRG_BLOCK>(s2, red);
  if (threadIdx.x == 0) {
    p.slab0[2 * b] = s1;
    p.slab0[2 * b + 1] = s2;
  }
}

// Weight gradient of filters [fc0, fc0 + 32) over images [b0, b1): wave w owns 8 filters, lane l the taps l + 64 j (tap ks2 is the
// bias: multiplier 1).  Per image, an f32 sum over the positions of an LDS stage is added into float64 accumulators.
__device__ void conve_wgrad(const ConvBwdArgs& p, float* lds, int r) {
  constexpr int FW = 8, TJ = 4;
  const int ks2 = p.ks * p.ks, n2 = 2 * p.D, ntap = ks2 + 1;
  const int fci = r % p.NFC, bs = r / p.NFC;
  const int fcb = fci * CV_WG_FILTERS;
  const int wv = threadIdx.x / MRG_WAVE, ln = threadIdx.x % MRG_WAVE;
  const int bb0 = bs * p.BPB, bb1 = min(p.B, bb0 + p.BPB);
  float* img = lds;
  float* gl = lds + n2;
  int toff[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int tap = ln + MRG_WAVE * j;
    toff[j] = tap < ks2 ? (tap / p.ks) * p.Wi + tap % p.ks : -1;
  }
  double accd[TJ][FW];
#pragma unroll
  for (int j = 0; j < TJ; ++j)
#pragma unroll
    for (int q = 0; q < FW; ++q) accd[j][q] = 0.0;
  const float mean = p.stats0[0], invstd = p.stats0[1], g0 = p.w0[0], be0 = p.b0[0];
  const int nf = min(CV_WG_FILTERS, p.F - fcb);
  for (int b = bb0; b < bb1; ++b) {
    for (int t = threadIdx.x; t < n2; t += MRG_BLOCK) img[t] = (conve_pixel(p.sub, p.rel, b, p.D, t, p.layout) - mean) * invstd * g0 + be0;
    const float* gzb = p.gz + ((int64_t)b * p.F + fcb) * p.P;
    for (int pc0 = 0; pc0 < p.P; pc0 += p.PC) {
      const int pn = min(p.PC, p.P - pc0);
      for (int i = threadIdx.x; i < CV_WG_FILTERS * pn; i += MRG_BLOCK) {
        const int fl = i / pn, pp = i - fl * pn;
        gl[fl * p.PC + pp] = fl < nf ? gzb[(int64_t)fl * p.P + pc0 + pp] : 0.f;
      }
      __syncthreads();
      float accf[TJ][FW];
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int q = 0; q < FW; ++q) accf[j][q] = 0.f;
      const float* gw = gl + wv * FW * p.PC;
      for (int pp = 0; pp < pn; ++pp) {
        const int pos = pc0 + pp;
        const int oy = pos / p.Wo, pb = oy * p.Wi + (pos - oy * p.Wo);
        float gv[FW];
#pragma unroll
        for (int q = 0; q < FW; ++q) gv[q] = gw[q * p.PC + pp];
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          if (ln + MRG_WAVE * j >= ntap) continue;
          const float x = toff[j] >= 0 ? img[pb + toff[j]] : 1.f;
#pragma unroll
          for (int q = 0; q < FW; ++q) accf[j][q] = fmaf(gv[q], x, accf[j][q]);
        }
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int q = 0; q < FW; ++q) accd[j][q] += (double)accf[j][q];
      __syncthreads();
    }
  }
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int tap = ln + MRG_WAVE * j;
    if (tap >= ntap) continue;
#pragma unroll
    for (int q = 0; q < FW; ++q) {
      const int f = fcb + wv * FW + q;
      if (f < p.F) p.slabw[((int64_t)bs * p.F + f) * ntap + tap] = accd[j][q];
    }
  }
}

// Workgroups [0, B): the input gradient of one image each; the rest: weight-gradient slabs.
__global__ __launch_bounds__(MRG_BLOCK) void conve_conv_bwd_k(ConvBwdArgs p) {
  extern __shared__ float lds[];
  __shared__ double red[MRG_BLOCK];
  if ((int)blockIdx.x < p.B) conve_igrad(p, lds, red, blockIdx.x);
  else conve_wgrad(p, lds, blockIdx.x - p.B);
}

// Workgroups [0, NE): BN0 backward over 256 pixels each (the image partial sums reduced in order b = 0 .. B-1 first), scattered to
// gsub / grel by layout; the rest: the weight-gradient slabs summed over the image ranges in order.
__global__ __launch_bounds__(MRG_BLOCK) void conve_finish_k(int layout, const float* __restrict__ sub, const float* __restrict__ rel, int B, int D,
                                                            const float* __restrict__ stats0, const float* __restrict__ w0, int training,
                                                            const float* __restrict__ gx0, const double* __restrict__ slab0,
                                                            const double* __restrict__ slabw, int BS, int F, int ntap, int NE,
                                                            float* __restrict__ gsub, float* __restrict__ grel, float* __restrict__ gw0,
                                                            float* __restrict__ gb0, float* __restrict__ gWc, float* __restrict__ gbc) {
  __shared__ double red[MRG_BLOCK];
  if ((int)blockIdx.x >= NE) {
    const int64_t i = (int64_t)(blockIdx.x - NE) * MRG_BLOCK + threadIdx.x;
    const int64_t nw = (int64_t)F * ntap;
    if (i >= nw) return;
    double s = 0.0;
    for (int bs = 0; bs < BS; ++bs) s += slabw[bs * nw + i];
    const int f = (int)(i / ntap), tap = (int)(i - (int64_t)f * ntap);
    if (tap < ntap - 1) gWc[(int64_t)f * (ntap - 1) + tap] = (float)s;
    else if (gbc) gbc[f] = (float)s;
    return;
  }
  double s1 = 0.0, s2 = 0.0;
  for (int b = threadIdx.x; b < B; b += MRG_BLOCK) {
    s1 += slab0[2 * b];
    s2 += slab0[2 * b + 1];
  }
  const double S1 = block_sum_d<MRG_BLOCK>(s1, red), S2 = block_sum_d<MRG_BLOCK>(s2, red);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gw0[0] = (float)S2;
    gb0[0] = (float)S1;
  }
  const int n2 = 2 * D;
  const int64_t e = (int64_t)blockIdx.x * MRG_BLOCK + threadIdx.x;
  if (e >= (int64_t)B * n2) return;
  const int64_t b = e / n2;
  const int t = (int)(e - b * n2);
  const float mean = stats0[0], invstd = stats0[1];
  const float c0 = w0[0] * invstd;
  const double nn = (double)B * n2;
  const float g = gx0[e];
  float gi;
  if (training) {
    const float xh = (conve_pixel(sub, rel, b, D, t, layout) - mean) * invstd;
    gi = c0 * (g - (float)(S1 / nn) - xh * (float)(S2 / nn));
  } else {
    gi = c0 * g;
  }
  if (layout == MRG_CONVE_STACKED) {
    if (t < D) gsub[b * D + t] = gi;
    else grel[b * D + t - D] = gi;
  } else {
    if (t & 1) grel[b * D + (t >> 1)] = gi;
    else gsub[b * D + (t >> 1)] = gi;
  }
}

// ---- host-side shapes ----------------------------------------------------------------------------------------------------------
static bool shape_ok(int64_t B, int D, int Hi, int Wi, int F, int ks) {
  if (B < 1 || D < 1 || D > MRG_CONVE_MAX_D || F < 1 || ks < 1 || ks > MRG_CONVE_MAX_KS) return false;
  if (Hi < ks || Wi < ks || (int64_t)Hi * Wi != 2 * (int64_t)D) return false;
  const int64_t P = (int64_t)(Hi - ks + 1) * (Wi - ks + 1);
  return B * 2 * D < (1ll << 31) && B * P < (1ll << 31) && (int64_t)F * P < (1ll << 31);
}

// split count of the forward fc product: about 1024 workgroups, at least 256 of K per split
static int fc_splits(int64_t B, int64_t K, int D) {
  const int64_t tiles = ((B + CV_GEMM_T - 1) / CV_GEMM_T) * ((D + CV_GEMM_T - 1) / CV_GEMM_T);
  int64_t s = (1024 + tiles - 1) / tiles;
  const int64_t kmax = (K + 255) / 256;
  if (s > kmax) s = kmax;
  return (int)(s < 1 ? 1 : s);
}

static int64_t fc_chunk(int64_t K, int S) {
  const int64_t kc = (K + S - 1) / S;
  return (kc + CV_GEMM_BK - 1) / CV_GEMM_BK * CV_GEMM_BK;
}

// weight-gradient partition: images per workgroup so that (filter chunks) x (image ranges) is about 512 workgroups
static void wgrad_split(int64_t B, int F, int* nfc, int* bpb, int* bs) {
  *nfc = (F + CV_WG_FILTERS - 1) / CV_WG_FILTERS;
  int64_t want = 512 / *nfc;
  if (want < 1) want = 1;
  if (want > B) want = B;
  *bpb = (int)((B + want - 1) / want);
  *bs = (int)((B + *bpb - 1) / *bpb);
}

template <bool A_KC, bool B_NC>
static void gemm(const float* A, int64_t sam, int64_t sak, const float* Bp, int64_t sbk, int64_t sbn, float* C, int64_t M, int64_t N, int64_t K,
                 int S, hipStream_t st) {
  const int64_t kc = fc_chunk(K, S);
  const dim3 grid((unsigned)((N + CV_GEMM_T - 1) / CV_GEMM_T), (unsigned)((M + CV_GEMM_T - 1) / CV_GEMM_T), (unsigned)S);
  hipLaunchKernelGGL((conve_gemm_k<A_KC, B_NC>), grid, dim3(MRG_BLOCK), 0, st, A, sam, sak, Bp, sbk, sbn, C, (int)M, (int)N, (int)K, (int)kc);
}

}  // namespace mrg

using namespace mrg;

extern "C" int64_t mrg_conve_fc_workspace_bytes(int64_t B, int64_t K, int D) {
  if (B < 1 || K < 1 || D < 1) return 0;
  const int64_t fwd = (int64_t)fc_splits(B, K, D) * B * D * 4;
  const int64_t bwd = B * D * 4;
  return fwd > bwd ? fwd : bwd;
}

extern "C" int64_t mrg_conve_bwd_workspace_bytes(int64_t B, int D, int F, int ks) {
  if (B < 1 || D < 1 || F < 1 || ks < 1) return 0;
  int nfc, bpb, bs;
  wgrad_split(B, F, &nfc, &bpb, &bs);
  const int64_t gx0 = (B * 2 * D * 4 + 15) / 16 * 16;
  return gx0 + B * 2 * 8 + (int64_t)bs * F * (ks * ks + 1) * 8;
}

extern "C" int mrg_conve_bn0_fwd(const float* sub, const float* rel, int64_t B, int D, float* running_mean, float* running_var, int training,
                                 float eps, float momentum, float* stats0, void* stream) {
  if (B < 1 || D < 1 || (training && 2 * B * D < 2)) return MRG_E_SHAPE;
  if (!sub || !rel || !stats0 || (!training && (!running_mean || !running_var))) return MRG_E_NULLPTR;
  hipLaunchKernelGGL(conve_bn0_stats_k, dim3(1), dim3(1024), 0, (hipStream_t)stream, sub, rel, B * D, running_mean, running_var, training, eps,
                     momentum, stats0);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_conve_conv_fwd(int layout, const float* sub, const float* rel, int64_t B, int D, int Hi, int Wi, const float* stats0,
                                  const float* bn0_w, const float* bn0_b, const float* Wc, const float* bc, int F, int ks, float* z,
                                  void* stream) {
  if (layout != MRG_CONVE_STACKED && layout != MRG_CONVE_INTERLEAVED) return MRG_E_ENUM;
  if (!shape_ok(B, D, Hi, Wi, F, ks)) return MRG_E_SHAPE;
  if (!sub || !rel || !stats0 || !bn0_w || !bn0_b || !Wc || !z) return MRG_E_NULLPTR;
  const int Ho = Hi - ks + 1, Wo = Wi - ks + 1, P = Ho * Wo, FC = F < CV_WG_FILTERS ? F : CV_WG_FILTERS;
  const size_t lds = (size_t)(2 * D + FC * ks * ks + FC) * 4;
  const dim3 grid((unsigned)B, (unsigned)((F + FC - 1) / FC));
  hipLaunchKernelGGL(conve_conv_fwd_k, grid, dim3(MRG_BLOCK), lds, (hipStream_t)stream, layout, sub, rel, D, Wi, stats0, bn0_w, bn0_b, Wc, bc, F,
                     ks, FC, Wo, P, z);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_conve_bn1_fwd(const float* z, int64_t B, int F, int P, const float* bn1_w, const float* bn1_b, float* running_mean,
                                 float* running_var, const float* keep1, int training, float eps, float momentum, float* stats1, float* a,
                                 void* stream) {
  if (B < 1 || F < 1 || P < 1 || B * P >= (1ll << 31) || (training && B * P < 2)) return MRG_E_SHAPE;
  if (!z || !bn1_w || !bn1_b || !stats1 || !a || (!training && (!running_mean || !running_var))) return MRG_E_NULLPTR;
  hipLaunchKernelGGL(conve_bn1_fwd_k, dim3((unsigned)F), dim3(MRG_BLOCK), 0, (hipStream_t)stream, z, (int)B, F, P, bn1_w, bn1_b, running_mean,
                     running_var, keep1, training, eps, momentum, stats1, a);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_conve_fc_fwd(const float* a, const float* Wfc, const float* bfc, const float* keep2, float* h, void* ws, int64_t B, int64_t K,
                                int D, void* stream) {
  if (B < 1 || K < 1 || D < 1 || K >= (1ll << 31) || B >= (1ll << 31)) return MRG_E_SHAPE;
  if (!a || !Wfc || !h) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int S = fc_splits(B, K, D);
  float* part = (float*)ws;
  gemm<true, false>(a, K, 1, Wfc, 1, K, part, B, D, K, S, st);
  MRG_LAUNCH_CHECK();
  const int64_t MN = B * D;
  hipLaunchKernelGGL(conve_fc_reduce_k, dim3((unsigned)((MN + MRG_BLOCK - 1) / MRG_BLOCK)), dim3(MRG_BLOCK), 0, st, part, S, bfc, keep2, h, MN, D);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_conve_fc_bwd(const float* gh, const float* keep2, const float* a, const float* Wfc, float* ga, float* gWfc, float* gbfc,
                                void* ws, int64_t B, int64_t K, int D, void* stream) {
  if (B < 1 || K < 1 || D < 1 || K >= (1ll << 31) || B >= (1ll << 31)) return MRG_E_SHAPE;
  if (!gh || !a || !Wfc || !ga || !gWfc) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* gpre = (float*)ws;
  hipLaunchKernelGGL(conve_fc_gpre_k, dim3((unsigned)((D + 63) / 64)), dim3(MRG_BLOCK), 0, st, gh, keep2, gpre, gbfc, (int)B, D);
  MRG_LAUNCH_CHECK();
  gemm<true, true>(gpre, D, 1, Wfc, K, 1, ga, B, K, D, 1, st);        // dL/da [B, K] = gpre Wfc
  MRG_LAUNCH_CHECK();
  gemm<false, true>(gpre, 1, D, a, K, 1, gWfc, D, K, B, 1, st);       // dL/dWfc [D, K] = gpre^T a
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_conve_bn1_bwd(float* g, const float* z, const float* a, const float* keep1, const float* stats1, const float* bn1_w, int training,
                                 int64_t B, int F, int P, float* gw1, float* gb1, void* stream) {
  if (B < 1 || F < 1 || P < 1 || B * P >= (1ll << 31)) return MRG_E_SHAPE;
  if (!g || !z || !a || !stats1 || !bn1_w || !gw1 || !gb1) return MRG_E_NULLPTR;
  hipLaunchKernelGGL(conve_bn1_bwd_k, dim3((unsigned)F), dim3(MRG_BLOCK), 0, (hipStream_t)stream, g, z, a, keep1, stats1, bn1_w, training, (int)B,
                     F, P, gw1, gb1);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_conve_conv_bwd(int layout, const float* sub, const float* rel, int64_t B, int D, int Hi, int Wi, const float* stats0,
                                  const float* bn0_w, const float* bn0_b, const float* Wc, int F, int ks, const float* gz, void* ws,
                                  void* stream) {
  if (layout != MRG_CONVE_STACKED && layout != MRG_CONVE_INTERLEAVED) return MRG_E_ENUM;
  if (!shape_ok(B, D, Hi, Wi, F, ks)) return MRG_E_SHAPE;
  if (!sub || !rel || !stats0 || !bn0_w || !bn0_b || !Wc || !gz) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  ConvBwdArgs p;
  p.layout = layout; p.sub = sub; p.rel = rel; p.B = (int)B; p.D = D; p.Hi = Hi; p.Wi = Wi; p.F = F; p.ks = ks;
  p.Ho = Hi - ks + 1; p.Wo = Wi - ks + 1; p.P = p.Ho * p.Wo;
  p.stats0 = stats0; p.w0 = bn0_w; p.b0 = bn0_b; p.Wc = Wc; p.gz = gz;
  char* w = (char*)ws;
  const int64_t gx0b = (B * 2 * D * 4 + 15) / 16 * 16;
  p.gx0 = (float*)w;
  p.slab0 = (double*)(w + gx0b);
  p.slabw = p.slab0 + 2 * B;
  const int ks2 = ks * ks;
  p.FCI = CV_LDS_FLOATS / (ks2 + p.P);
  if (p.FCI > F) p.FCI = F;
  int bs;
  wgrad_split(B, F, &p.NFC, &p.BPB, &bs);
  p.PC = (CV_LDS_FLOATS - 2 * D) / CV_WG_FILTERS;
  if (p.PC > p.P) p.PC = p.P;
  if (p.FCI < 1 || p.PC < 1 || 2 * D > CV_MAX_PJ * MRG_BLOCK) return MRG_E_SHAPE;
  const size_t li = (size_t)p.FCI * (ks2 + p.P), lw = (size_t)2 * D + (size_t)CV_WG_FILTERS * p.PC;
  const size_t lds = (li > lw ? li : lw) * 4;
  hipLaunchKernelGGL(conve_conv_bwd_k, dim3((unsigned)(B + (int64_t)p.NFC * bs)), dim3(MRG_BLOCK), lds, (hipStream_t)stream, p);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

extern "C" int mrg_conve_finish_bwd(int layout, const float* sub, const float* rel, int64_t B, int D, int F, int ks, const float* stats0,
                                    const float* bn0_w, int training, const void* ws, float* gsub, float* grel, float* gw0, float* gb0,
                                    float* gWc, float* gbc, void* stream) {
  if (layout != MRG_CONVE_STACKED && layout != MRG_CONVE_INTERLEAVED) return MRG_E_ENUM;
  if (B < 1 || D < 1 || D > MRG_CONVE_MAX_D || F < 1 || ks < 1 || ks > MRG_CONVE_MAX_KS || B * 2 * D >= (1ll << 31)) return MRG_E_SHAPE;
  if (!sub || !rel || !stats0 || !bn0_w || !gsub || !grel || !gw0 || !gb0 || !gWc) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  int nfc, bpb, bs;
  wgrad_split(B, F, &nfc, &bpb, &bs);
  const char* w = (const char*)ws;
  const int64_t gx0b = (B * 2 * D * 4 + 15) / 16 * 16;
  const float* gx0 = (const float*)w;
  const double* slab0 = (const double*)(w + gx0b);
  const double* slabw = slab0 + 2 * B;
  const int ntap = ks * ks + 1;
  const int NE = (int)((B * 2 * D + MRG_BLOCK - 1) / MRG_BLOCK);
  const int NR = (int)(((int64_t)F * ntap + MRG_BLOCK - 1) / MRG_BLOCK);
  hipLaunchKernelGGL(conve_finish_k, dim3((unsigned)(NE + NR)), dim3(MRG_BLOCK), 0, (hipStream_t)stream, layout, sub, rel, (int)B, D, stats0, bn0_w,
                     training, gx0, slab0, slabw, bs, F, ntap, NE, gsub, grel, gw0, gb0, gWc, gbc);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}
