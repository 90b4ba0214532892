// Shared parts of the split-bf16 ("3-way split") matrix core: ONE definition of everything the row GEMM kernels
// (gemm_x3.hpp, gemm_x3s.hpp, gemm_x3s8.hpp, gemm_x3q.hpp), the weight-gradient kernels (wgrad.hip: wgrad_x3_k, wgrad_x3v_k) and
// the lab kernels (tools/lab/) have in common, so that the bit-exactness the tests pin between them rests on one text:
//   * the process-wide kernel switches (GemmSwitches),
//   * the arithmetic: the split of f32 into three bf16 planes and the six-term product chain,
//   * the weight split kernel (bsplit_k) over a layout policy,
//   * the pipeline parts of the LDS-weight kernels (activation fragment loads, weight slab L2 -> LDS, fragment read-back) and
//     the grouped-launch preamble,
//   * the launch helper.
// Everything here is __forceinline__: the kernels that use these parts compile to the machine code of the spelled-out form
// (tools/lab/asm_diff.py compares two device assemblies kernel by kernel).
//
// The arithmetic.  Every f32 operand is written as the exact-to-2^-26 sum of three bf16 numbers,
//   x = h + m + l,   h = bf16(x),  m = bf16(x - h),  l = bf16(x - h - m)       (round-to-nearest-even each)
// and a product is evaluated as the six leading cross terms, accumulated in f32 by the MFMA:
//   a*b ~= ah*bh + ah*bm + am*bh + ah*bl + al*bh + am*bm        dropped: am*bl + al*bm + al*bl  (<= 2^-25 |a b|)
// so the result carries an error below one f32 ulp of each product -- the same class as the f32 pipe
// (tests pin |err| against a float64 product next to the exact-f32 kernel).  Why: v_mfma_f32_32x32x2_f32
// retires 64 flop/cycle/SIMD (157 TF/s chip peak), v_mfma_f32_32x32x16_bf16 1024; six bf16 MFMAs replace
// eight f32 MFMAs per 16 k-columns at 1/16 of the cycles each: 2.7x less matrix-pipe time for the same
// answer.  The price is VALU work for the splits.
#pragma once
#include <type_traits>
#include "gemm.hpp"

namespace mrg {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- process-wide kernel switches ------------------------------------------------------------------------------------------
// Which kernel a launch takes.  One object per shared library (the static of an inline function), written by the
// mrg_gemm_set_* / mrg_wgrad_set_variant entry points (linear.hip, wgrad.hip), read by the launchers and by gemm_dispatch.hpp.  The
// non-default values are the comparison points of the tests, of bench.py and of the lab tools.
constexpr int64_t X3N_MAX_ROWS = 16384;     // measured crossover (linear 200 x 200, one MI355X): 13 vs 24 us at 4 096 rows, 19 vs 27 at 16 384, 31 vs 30 at 32 768
struct GemmSwitches {
  // mrg_gemm_set_mode.  0 (default): split-bf16 core whenever the operands qualify and a workspace was given, on the LDS-weight
  // kernels (gemm_x3s.hpp and siblings); 1: exact-f32 core only (v_mfma_f32_32x32x2_f32) -- the comparison point of the tests and of
  // bench.py; 2: the split arithmetic on the wave-autonomous one-wave-per-SIMD kernel of gemm_x3.hpp (rounds 1-2's default).
  int mode = 0;
  // mrg_gemm_set_q.  1 (default): products of 129..224 columns with K > X3Q_MIN_K run on the 16 x 16 x 32 kernel of gemm_x3q.hpp;
  // 0: every launch stays on rowgemm_x3s_k (rollback); 2 (lab, tests): every eligible K > 48.
  int q = 1;
  // mrg_gemm_set_small.  The row bound up to which a product runs on the wave-autonomous kernel with two-tile column blocks
  // (gemm_dispatch.hpp: x3n_shape); 0 = off.
  int64_t small_rows = X3N_MAX_ROWS;
  // mrg_gemm_set_wide8.  1 (default): plain launches whose output is eight column tiles wide run on rowgemm_x3s8_k; 0: two
  // four-tile column blocks (round 3).
  int wide8 = 1;
  // mrg_wgrad_set_variant.  1 (default): weight-gradient fragments split once per workgroup (wgrad_x3v_k); 0: by every consuming
  // wave (wgrad_x3_k).
  int wgrad_variant = 1;
};
inline GemmSwitches& gemm_switches() { static GemmSwitches s; return s; }

// ---- arithmetic --------------------------------------------------------------------------------------------------------------
// two floats -> three packed bf16 pairs (element 0 in the low half).
// The residual subtractions are spelled as single v_sub_f32: hipcc would SLP-pack the pair into v_pk_add_f32,
// which costs ~13 cycles of matrix-pipe time each when issued beside MFMAs (MI355X_MICROARCH.md, "price of one
// filler"), against ~0 for a plain 4-cycle VALU instruction.
__device__ __forceinline__ float sub1(float a, float b) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  f32x2 v = {x0, x1};
  h = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  f32x2 r = {sub1(x0, __builtin_bit_cast(float, h << 16)), sub1(x1, __builtin_bit_cast(float, h & 0xffff0000u))};
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
  f32x2 r2 = {sub1(r.x, __builtin_bit_cast(float, m << 16)), sub1(r.y, __builtin_bit_cast(float, m & 0xffff0000u))};
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
}
// 8 floats (one MFMA operand fragment: 8 consecutive k) -> the three bf16 planes
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& H, u32x4& M, u32x4& L) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned h, m, l;
    split_pair(v[2 * j], v[2 * j + 1], h, m, l);
    H[j] = h; M[j] = m; L[j] = l;
  }
}
// pair q = 0..3 (floats 2q, 2q + 1) of a fragment held as two float4: the kernels split a fragment pair by pair in the shadow
// of their MFMAs
__device__ __forceinline__ void split_pair_of(const v4f (&x)[2], int q, u32x4& H, u32x4& M, u32x4& L) {
  const v4f& v = x[q >> 1];
  unsigned h, m, l;
  if (q & 1) split_pair(v.z, v.w, h, m, l); else split_pair(v.x, v.y, h, m, l);
  H[q] = h; M[q] = m; L[q] = l;
}

// One matrix instruction of the chain: 32 x 32 x 16 on a 16-register accumulator, 16 x 16 x 32 on a 4-register one (gemm_x3q.hpp).
__device__ __forceinline__ f32x16 x3_mm(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4v x3_mm(bf16x8 a, bf16x8 b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
// THE TERM ORDER of every split-core kernel: Am*Bm, Al*Bh, Ah*Bl, Am*Bh, Ah*Bm, Ah*Bh -- small terms first, the leading term
// last, so that the small ones are not rounded away against an accumulator that already holds the large one.  Every accumulator
// of every kernel receives its six terms in this order; that (and the order of the k-slabs) is what makes the kernels agree bit
// for bit.
// One accumulator (a single chain: each MFMA waits for its predecessor):
template <class ACC>
__device__ __forceinline__ void x3_chain(ACC& c, bf16x8 Ah, bf16x8 Am, bf16x8 Al, bf16x8 Bh, bf16x8 Bm, bf16x8 Bl) {
  c = x3_mm(Am, Bm, c);
  c = x3_mm(Al, Bh, c);
  c = x3_mm(Ah, Bl, c);
  c = x3_mm(Am, Bh, c);
  c = x3_mm(Ah, Bm, c);
  c = x3_mm(Ah, Bh, c);
}
// Two accumulators interleaved (a dependent MFMA issued back to back costs ~6 extra cycles, measured with
// tools/mfma_bf16_peak.hip; with another accumulator's MFMA in between the pipe stays busy): accumulator i takes A_i * B_i.
// The callers pass the same A twice (two column tiles of one row tile) or the same B twice (two row tiles of one column tile).
__device__ __forceinline__ void x3_chain2(f32x16& c0, f32x16& c1, bf16x8 Ah0, bf16x8 Am0, bf16x8 Al0, bf16x8 Bh0, bf16x8 Bm0, bf16x8 Bl0,
                                          bf16x8 Ah1, bf16x8 Am1, bf16x8 Al1, bf16x8 Bh1, bf16x8 Bm1, bf16x8 Bl1) {
  c0 = x3_mm(Am0, Bm0, c0); c1 = x3_mm(Am1, Bm1, c1);
  c0 = x3_mm(Al0, Bh0, c0); c1 = x3_mm(Al1, Bh1, c1);
  c0 = x3_mm(Ah0, Bl0, c0); c1 = x3_mm(Ah1, Bl1, c1);
  c0 = x3_mm(Am0, Bh0, c0); c1 = x3_mm(Am1, Bh1, c1);
  c0 = x3_mm(Ah0, Bm0, c0); c1 = x3_mm(Ah1, Bm1, c1);
  c0 = x3_mm(Ah0, Bh0, c0); c1 = x3_mm(Ah1, Bh1, c1);
}
// MT = 1 or 2 row tiles of column tile n against one weight fragment (the wave-autonomous kernels)
template <int MT, int NT>
__device__ __forceinline__ void x3_chain_rows(f32x16 (&acc)[MT][NT], int n, const u32x4 (&Ah)[MT], const u32x4 (&Am)[MT], const u32x4 (&Al)[MT],
                                              bf16x8 Bh, bf16x8 Bm, bf16x8 Bl) {
  static_assert(MT == 1 || MT == 2, "one or two row tiles per wave");
  auto c = [](const u32x4& v) { return __builtin_bit_cast(bf16x8, v); };
  if constexpr (MT == 2) x3_chain2(acc[0][n], acc[1][n], c(Ah[0]), c(Am[0]), c(Al[0]), Bh, Bm, Bl, c(Ah[1]), c(Am[1]), c(Al[1]), Bh, Bm, Bl);
  else x3_chain(acc[0][n], c(Ah[0]), c(Am[0]), c(Al[0]), Bh, Bm, Bl);
}

// ---- weight split ------------------------------------------------------------------------------------------------------------
// B (a weight matrix, a few hundred KB) is split ONCE per call into fragment order: one 16-byte chunk per (fragment, plane, lane),
// so that a kernel fetches a fragment with one global_load_dwordx4 / ds_read_b128 per plane, conflict free.  B(n, k) =
// B[n * sn + k * sk]; rows >= N and columns >= K are zero, which is also what makes the clamped out-of-range A chunks harmless.
// sk != 1 presents W^T without a transpose pass.
// Up to three weights of the same shape in one launch (blockIdx.y): the direction segments of a dense filter.
// Optional second source along k (the input gradient of two candidates in one product, [dz_a | dz_b] [W_a ; W_b]):
// columns k >= ksplit come from B2 at k - ksplit (ksplit = 0: single source).
inline int x3_tiles(int N, int nt) { return ((N + nt * 32 - 1) / (nt * 32)) * nt; }     // column tiles, padded to blocks of nt
inline int x3_slabs(int K) { return (K + 15) / 16; }
inline size_t x3_bsplit_bytes(int N, int K, int nt) { return (size_t)x3_slabs(K) * x3_tiles(N, nt) * 3 * 64 * 16; }
// Output: Bp[slab][tile][plane][lane], one 16-byte chunk each; thread idx makes the three chunks of lane idx % 64 of column tile
// (idx / 64) % tiles of k-slab (idx / 64) / tiles.  The layout policy says how many chunks and how many tiles per slab there are
// and which B(n, k0 .. k0 + 7) that lane holds (source).
// 32 x 32 x 16 kernels: n = tile*32 + lane%32, k = slab*16 + (lane/32)*8 + j
struct BSplitTiles32 {
  static __host__ __device__ int chunks(int ntile, int nslab) { return nslab * ntile * 64; }
  static __host__ __device__ int tiles(int ntile, int) { return ntile; }
  static __device__ __forceinline__ void source(int lane, int tile, int slab, int& n, int& k0) {
    n = tile * 32 + (lane & 31); k0 = slab * 16 + (lane >> 5) * 8;
  }
};
// 16 x 16 x 32 kernel (gemm_x3q.hpp): slabs of 32 k, 14 tiles of 16 columns that the kernel fetches as two half-slabs of seven
// (Bp[slab32][half][tile 0..6][plane][lane] is the same order); lane (column c = lane % 16, k-group g = lane / 16) holds
// B[n = tile * 16 + c][k = 32 slab + 8 g + 0..7]
constexpr int X3Q_HT = 7;                       // 16-column tiles per half-slab
constexpr int X3Q_NT = 2 * X3Q_HT;              // 14 tiles = 224 columns
struct BSplitTiles16 {
  static __host__ __device__ int chunks(int nslab) { return nslab * X3Q_NT * 64; }
  static __host__ __device__ int tiles(int) { return X3Q_NT; }
  static __device__ __forceinline__ void source(int lane, int tile, int slab, int& n, int& k0) {
    n = tile * 16 + (lane & 15); k0 = slab * 32 + (lane >> 4) * 8;
  }
};
struct BSplit3 { const float* B[3]; u32x4* out[3]; const float* B2[3]; int ksplit; };
template <class LAYOUT, class... DIMS>              // DIMS: the layout's run-time dimensions (ntile, nslab / nslab)
static __global__ void bsplit_k(BSplit3 p, int64_t sn, int64_t sk, int N, int K, DIMS... dims) {
  const float* __restrict__ B = p.B[blockIdx.y];
  const float* __restrict__ B2 = p.B2[blockIdx.y];
  const int ksplit = (p.ksplit > 0 && B2) ? p.ksplit : K;
  u32x4* __restrict__ Bp = p.out[blockIdx.y];
  if (!B) return;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= LAYOUT::chunks(dims...)) return;
  const int ntile = LAYOUT::tiles(dims...);
  const int lane = idx & 63, tile = (idx >> 6) % ntile, slab = (idx >> 6) / ntile;
  int n, k0;
  LAYOUT::source(lane, tile, slab, n, k0);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    v[j] = (n < N && k < K) ? (k < ksplit ? B[n * sn + k * sk] : B2[n * sn + (k - ksplit) * sk]) : 0.f;
  }
  u32x4 h, m, l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {                        // (split8 spelled out: through it the loads above are grouped differently)
    unsigned a, b, c;
    split_pair(v[2 * j], v[2 * j + 1], a, b, c);
    h[j] = a; m[j] = b; l[j] = c;
  }
  u32x4* o = Bp + ((int64_t)(slab * ntile + tile) * 3) * 64 + lane;
  o[0] = h; o[64] = m; o[128] = l;
}
// `count` weights (<= 3) B[i] -> out[i] in one launch
template <class LAYOUT, class... DIMS>
inline void launch_bsplit_layout(const float* const* B, int64_t sn, int64_t sk, int N, int K, void* const* out, int count, hipStream_t st,
                                 const float* const* B2, int ksplit, DIMS... dims) {
  BSplit3 p{};
  for (int i = 0; i < count; ++i) { p.B[i] = B[i]; p.out[i] = (u32x4*)out[i]; p.B2[i] = B2 ? B2[i] : nullptr; }
  p.ksplit = B2 ? ksplit : 0;
  hipLaunchKernelGGL((bsplit_k<LAYOUT, DIMS...>), dim3((LAYOUT::chunks(dims...) + 255) / 256, count), dim3(256), 0, st, p, sn, sk, N, K, dims...);
}
inline void launch_bsplit3(const float* const* B, int64_t sn, int64_t sk, int N, int K, int nt, void* const* out, hipStream_t st,
                           const float* const* B2 = nullptr, int ksplit = 0) {
  const int ntile = x3_tiles(N, nt), nslab = x3_slabs(K);
  launch_bsplit_layout<BSplitTiles32>(B, sn, sk, N, K, out, 3, st, B2, ksplit, ntile, nslab);
}
inline void launch_bsplit(const float* B, int64_t sn, int64_t sk, int N, int K, int nt, void* Bp, hipStream_t st) {
  const int ntile = x3_tiles(N, nt), nslab = x3_slabs(K);
  launch_bsplit_layout<BSplitTiles32>(&B, sn, sk, N, K, &Bp, 1, st, nullptr, 0, ntile, nslab);
}
inline int x3q_slabs(int K) { return (K + 31) / 32; }
inline void launch_bsplitq3(const float* const* B, int64_t sn, int64_t sk, int N, int K, void* const* out, int count, hipStream_t st,
                            const float* const* B2 = nullptr, int ksplit = 0) {
  const int nslab = x3q_slabs(K);
  launch_bsplit_layout<BSplitTiles16>(B, sn, sk, N, K, out, count, st, B2, ksplit, nslab);
}

// ---- pipeline parts ----------------------------------------------------------------------------------------------------------
// s_waitcnt vmcnt(n) with a run-time (wave-uniform) n <= 63
__device__ __forceinline__ void wait_vmcnt(int n) {
#define MRG_VM(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
  switch (n) {
    MRG_VM(0) MRG_VM(1) MRG_VM(2) MRG_VM(3) MRG_VM(4) MRG_VM(5) MRG_VM(6) MRG_VM(7)
    MRG_VM(8) MRG_VM(9) MRG_VM(10) MRG_VM(11) MRG_VM(12) MRG_VM(13) MRG_VM(14) MRG_VM(15)
    MRG_VM(16) MRG_VM(17) MRG_VM(18) MRG_VM(19) MRG_VM(20) MRG_VM(21) MRG_VM(22) MRG_VM(23)
    MRG_VM(24) MRG_VM(25) MRG_VM(26) MRG_VM(27) MRG_VM(28) MRG_VM(29) MRG_VM(30) MRG_VM(31)
    MRG_VM(32) MRG_VM(33) MRG_VM(34) MRG_VM(35) MRG_VM(36) MRG_VM(37) MRG_VM(38) MRG_VM(39)
    MRG_VM(40) MRG_VM(41) MRG_VM(42) MRG_VM(43) MRG_VM(44) MRG_VM(45) MRG_VM(46) MRG_VM(47)
    MRG_VM(48) MRG_VM(49) MRG_VM(50) MRG_VM(51) MRG_VM(52) MRG_VM(53) MRG_VM(54) MRG_VM(55)
    MRG_VM(56) MRG_VM(57) MRG_VM(58) MRG_VM(59) MRG_VM(60) MRG_VM(61) MRG_VM(62)
    default: asm volatile("s_waitcnt vmcnt(63)" ::: "memory"); break;
  }
#undef MRG_VM
}

// Grouped launch (GemmGroups): this workgroup's row range and its weight.  Declares row0 (first row of the workgroup) and Bq (the
// pre-split weight of its range) and re-points a.rows / bias / scale / rowscale of the kernel's own argument block `a` at range sg.
// The range index and the weight pointer are formed by unconditional scalar arithmetic (bp_stride = 0 in a plain launch): the B
// loads address through an SGPR pair.  GBM: rows per workgroup.
// A macro, not a function: it has to work on the kernel's own copy of the argument block.  Through a reference MRG_PICK becomes a
// select of ADDRESSES and the whole block moves to scratch (tried: 328 bytes, every epilogue store a flat_store); on a by-value
// copy the code is right but the scalar loads of the preamble change places.
#define MRG_PICK(F) (sg == 0 ? a.grp.F[0] : (sg == 1 ? a.grp.F[1] : a.grp.F[2]))
#define MRG_GROUP_SELECT(GBM)                                                                                          \
  int64_t row0 = (int64_t)blockIdx.x * (GBM);                                                                          \
  int sg = 0;                                                                                                          \
  if (a.grp.n > 0) sg = ((int)blockIdx.x >= a.grp.tile0[1] ? 1 : 0) + ((int)blockIdx.x >= a.grp.tile0[2] ? 1 : 0);     \
  sg = __builtin_amdgcn_readfirstlane(sg);                                                                             \
  const char* __restrict__ Bq = Bp + (int64_t)sg * a.grp.bp_stride;                                                    \
  if (a.grp.n > 0) {               /* constant indices only: a dynamic one would move the argument block to scratch */ \
    row0 = MRG_PICK(lo) + (int64_t)((int)blockIdx.x - MRG_PICK(tile0)) * (GBM);                                        \
    a.rows = MRG_PICK(hi);                                                                                             \
    a.bias = MRG_PICK(bias);                                                                                           \
    a.scale = MRG_PICK(scale);                                                                                         \
    if (!MRG_PICK(use_rowscale)) a.rowscale = nullptr;                                                                 \
  }

// The activation row a lane reads its fragments from: output row `row` (clamped into the operand; gathered through row_index:
// EPI_SEGMAX / EPI_SEGSUM walk the edges in destination order) of A1 and of A2.
__device__ __forceinline__ void x3_a_row(const GemmArgs& a, int64_t row, const float*& ar1, const float*& ar2) {
  int64_t rc = row < a.rows ? row : a.rows - 1;
  if (rc < 0) rc = 0;
  if (a.row_index) rc = a.row_index[rc];
  ar1 = a.A1 + rc * a.K1;
  ar2 = a.A2 + rc * a.K2;
}
// This lane's fragment of a slab: 8 consecutive k of its row from k = slab * KSLAB + kg * 8 on, as two 16-byte loads --
// asynchronous register fills, first read behind the matching counted s_waitcnt (gemm_x3.hpp).  Beyond the last slab the last one
// is read again (an asynchronous fill is never conditional).  K: columns of the reduction dimension (K1 alone when !DUAL).
template <int KSLAB, bool DUAL>
__device__ __forceinline__ void x3_load_a(v4f (&x)[2], int slab, int nslab, int kg, const float* ar1, const float* ar2, int K1, int K2, int K) {
  const int sl = slab < nslab ? slab : nslab - 1;
  const int k = sl * KSLAB + kg * 8;
  const float* p0 = gemm_a_ptr<DUAL>(ar1, ar2, K1, K2, K, k);
  const float* p1 = gemm_a_ptr<DUAL>(ar1, ar2, K1, K2, K, k + 4);
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(x[0]) : "v"(p0));
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(x[1]) : "v"(p1));
}
// Weight slab L2 -> LDS by LDS-DMA: the NCH 1 KB chunks (64 lanes x 16 B) at src go to dst, (NCH + 3) / 4 per wave; the last
// wave repeats the last chunk (same bytes to the same place).  Everything the DMA writes lies below 64 KiB of the workgroup's LDS.
// (wave and lane by reference, src and dst restrict: with plain value parameters hipcc adds the lane offset to the source first and
// the chunk offset second -- 64-bit vector adds where the kernels had a scalar base and a 32-bit lane offset.)
template <int NCH>
__device__ __forceinline__ void x3_fetch_b(const char* __restrict__ src, char* __restrict__ dst, const int& wave, const int& lane) {
  constexpr int NBW = (NCH + 3) / 4;
#pragma unroll
  for (int i = 0; i < NBW; ++i) {
    int c = wave * NBW + i;
    c = c < NCH ? c : NCH - 1;
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + c * 1024 + lane * 16), (lds_ptr_t)(dst + c * 1024), 16, 0, 0);
  }
}
// The three planes of one pre-split weight fragment from LDS byte address ad (this lane's chunk of plane 0)
__device__ __forceinline__ void x3_read_b(unsigned ad, u32x4 (&q)[3]) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(q[0]) : "v"(ad));
  asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(q[1]) : "v"(ad));
  asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(q[2]) : "v"(ad));
}

// ---- launch ------------------------------------------------------------------------------------------------------------------
// Allows the kernel `lds` bytes of dynamic LDS, launches it, returns MRG_OK or the HIP error.
template <class... KARGS, class... ARGS>
inline int launch_kernel(void (*kernel)(KARGS...), dim3 grid, dim3 block, size_t lds, hipStream_t st, ARGS... args) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<KARGS>(args)...);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MRG_OK : (int)e;
}

}  // namespace mrg
