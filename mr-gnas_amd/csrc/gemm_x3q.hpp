// Split-bf16 row GEMM on 16 x 16 x 32 tiles: 64-row workgroups, THREE per CU (round 5).
//
// What round 4's phase stamps said about rowgemm_x3s_k (profiles/r4_rowgemm_phases.txt): a wave that owns a 32-row strip of
// seven 32 x 32 tiles carries 112 accumulator registers, so a SIMD holds two waves, and a wave's life is prologue -> k-loop ->
// store tail IN SEQUENCE (7 500 / 48 200 / 18 800 cycles for 17 472 cycles of MFMA issue): two waves per SIMD are not enough to
// keep the matrix pipe busy through each other's load and store phases (busy 0.42-0.47).  The structural candidate the stamps
// named -- an output tile small enough for three waves per SIMD -- is this kernel:
//
//   * a wave owns 16 rows x 14 column tiles of 16 (v_mfma_f32_16x16x32_bf16: 4 accumulator registers per tile, 56 in all; the
//     same flop per cycle as the 32 x 32 x 16 form), a workgroup of four waves 64 rows; <= 168 registers -> three workgroups per
//     CU, whose prologues, k-loops and store tails interleave on every SIMD;
//   * k advances in slabs of 32; the pre-split weight of a slab travels L2 -> LDS by LDS-DMA as two half-slabs of seven column
//     tiles (21 KB each) into a ring of two buffers (42 KB per workgroup: three workgroups fit the CU's 160 KB); one barrier per
//     half-slab; the MFMA operands are read back with ds_read_b128 (fragment order: conflict free);
//   * activations go straight into registers in fragment order (lane (row r, k-group g) reads the 8 consecutive floats
//     k = 32 s + 8 g ..: two global_load_dwordx4 per slab), two slabs ahead, and are split into their bf16 planes in the shadow
//     of the second half-slab's MFMAs;
//   * the epilogue turns PAIRS of 16 x 16 tiles into the 32 x 32 store shape with v_permlane16_swap_b32 (one VALU instruction per
//     register pair): a store instruction then writes 2 rows x 128 bytes, exactly what gemm_epilogue's stores write -- four rows x
//     64 bytes per instruction (the 16 x 16 accumulator as it stands) would double the memory pipeline's line transactions.
//
// Same six cross terms per product and the same order of the terms per accumulator as the other split-core kernels; the sums over
// k are formed 32 at a time by the matrix instruction instead of 16, so results agree with them to rounding, not bit for bit
// (tests/test_ops_gpu.py pins the error against float64 next to the exact-f32 core: <= 1.5 x).
//
// The weight split for this kernel has its own layout (launch_bsplitq): [slab32][half][tile 0..6][plane][lane] x 16 bytes with
// lane (column c = lane % 16, k-group g = lane / 16) holding B[n = (half * 7 + tile) * 16 + c][k = 32 slab + 8 g + 0..7].
#pragma once
#include "gemm_x3.hpp"

namespace mrg {

// (X3Q_HT = 7 tiles of 16 columns per half-slab, X3Q_NT = 14 per slab: x3_parts.hpp, next to the weight split's layout)
constexpr int X3Q_CHUNK = X3Q_HT * 3 * 1024;    // bytes of one half-slab of the pre-split weight
constexpr int X3Q_ROWS = 64;                    // rows per workgroup

inline size_t x3q_bsplit_bytes(int K) { return (size_t)x3q_slabs(K) * 2 * X3Q_CHUNK; }

// ---- epilogue on PAIRS of 16 x 16 tiles ------------------------------------------------------------------------------------------
// C/D map of a 16 x 16 tile: col = lane & 15, row = 4 * (lane >> 4) + reg.  v_permlane16_swap_b32 a, b exchanges a's odd 16-lane
// rows with b's even ones, so for tiles 2j (a) and 2j + 1 (b) and register r:
//   a' : lanes  0-15 row r      of tile 2j | lanes 16-31 row r      of tile 2j+1 | lanes 32-47 row 8+r  of 2j | lanes 48-63 row 8+r  of 2j+1
//   b' : lanes  0-15 row 4+r    of tile 2j | lanes 16-31 row 4+r    of tile 2j+1 | lanes 32-47 row 12+r of 2j | lanes 48-63 row 12+r of 2j+1
// i.e. with li = lane & 31, lh = lane >> 5 a lane holds column 32 j + li of rows i + 8 lh, i = r (a') or 4 + r (b'): one store
// instruction writes two 128-byte row pieces.  Arithmetic per element is gemm_epilogue's (bias add, activation / gate / scale /
// accumulate in the same order).
// SUMS: as gemm_epilogue's -- the lane's sums over its eight rows of pair j go to sums[(lh * 2 + {0, 1}) * X3Q_HT * 32 + j * 32 + li].
template <int EPI, bool SUMS = false>
__device__ __forceinline__ void gemm_epilogue_q(const GemmArgs& a, f32x4v (&acc)[X3Q_NT], int64_t rowbase, int li, int lh, bool full,
                                                double* __restrict__ sums = nullptr) {
  static_assert(!SUMS || EPI == EPI_GATE || EPI == EPI_SCALE, "column sums: gate and scale epilogues only");
  constexpr int W = X3Q_HT * 32;
  if (rowbase >= a.rows) {                                 // wave-uniform: the whole 16-row strip is out of range
    if constexpr (SUMS) {
#pragma unroll
      for (int j = 0; j < X3Q_HT; ++j) { sums[(lh * 2 + 0) * W + j * 32 + li] = 0.0; sums[(lh * 2 + 1) * W + j * 32 + li] = 0.0; }
    }
    return;
  }
  const int last = (int)((a.rows - 1 - rowbase) < 15 ? (a.rows - 1 - rowbase) : 15);
  const int colw = li < a.N ? li : a.N - 1;
  float* crow[8];
  const float* srow[8];
  const float* trow[8];                                    // EPI_ACCUM2: the second addend
  float* xrow[8];
  float cs[8];
  bool rok[8];
  const bool cstore = EPI != EPI_GATE || a.C != nullptr;   // EPI_GATE with C == NULL: only the gate (aux) is stored
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = i + 8 * lh;
    const int rc = row < last ? row : last;
    rok[i] = row <= last;
    crow[i] = a.C + (rowbase + rc) * a.ldc + colw;
    if (EPI == EPI_GATE) srow[i] = a.S + (rowbase + rc) * a.ld_s + colw;
    if (epi_accum(EPI)) srow[i] = a.Cin + (rowbase + rc) * a.ld_cin + colw;
    if (EPI == EPI_ACCUM2) trow[i] = a.S + (rowbase + rc) * a.ld_s + colw;
    if (EPI == EPI_GATE) xrow[i] = a.aux ? a.aux + (rowbase + rc) * a.N + colw : nullptr;
    cs[i] = 1.0f;
    if (EPI == EPI_GATE || EPI == EPI_SCALE) cs[i] = a.scale * (a.rowscale ? a.rowscale[rowbase + rc] : 1.0f);
  }
  const int lc = li & 15;
#pragma unroll
  for (int j = 0; j < X3Q_HT; ++j) {
    // The bias is added BEFORE the lanes exchange (same sum per element: the exchange only moves data), so that the first reader of
    // an accumulator is an instruction the compiler sees -- it inserts the MFMA-result wait states itself; the exchange is inline
    // asm (the builtin __builtin_amdgcn_permlane16_swap of ROCm 7.2 returns its FIRST result twice and merges calls with different
    // operands: tools/lab/permlane16_swap_probe.hip) with the two wait states a VALU write of a swap operand needs inside the string.
    const int ca = (2 * j) * 16 + lc, cb = (2 * j + 1) * 16 + lc;
    const float bva = a.bias ? a.bias[ca < a.N ? ca : a.N - 1] : 0.f;
    const float bvb = a.bias ? a.bias[cb < a.N ? cb : a.N - 1] : 0.f;
    float acc8[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float xa = acc[2 * j][r] + bva, xb = acc[2 * j + 1][r] + bvb;
      asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(xa), "+v"(xb));
      acc8[r] = xa;
      acc8[4 + r] = xb;
    }
    const int col = j * 32 + li;
    const bool cok = col < a.N;                             // columns of this pair that exist; a lane beyond them re-reads its column of pair 0 (never stored)
    const int off = cok ? j * 32 : 0;
    float in[8], in2[8], v[8], g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) in[i] = 0.f;
    if ((EPI == EPI_GATE && (cstore || SUMS)) || epi_accum(EPI)) {
#pragma unroll
      for (int i = 0; i < 8; ++i) in[i] = srow[i][off];
    }
    if (EPI == EPI_ACCUM2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) in2[i] = trow[i][off];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x = acc8[i];
      if (EPI == EPI_BIAS_ACT) {
        v[i] = (a.act == MRG_ACT_RELU) ? (x > 0.f ? x : 0.f) : (a.act == MRG_ACT_SIGMOID ? sigmoidf_fast(x) : x);
      } else if (EPI == EPI_GATE) {
        g[i] = sigmoidf_fast(x);
        v[i] = g[i] * in[i] * cs[i];
      } else if (EPI == EPI_ACCUM2) {
        v[i] = (x + in[i]) + in2[i];
      } else if (EPI == EPI_SCALE) {
        v[i] = x * cs[i];
      } else {
        v[i] = x + in[i];
      }
    }
    if constexpr (SUMS) {
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double d = (full || rok[i]) ? (double)v[i] : 0.0;
        s1 += d; s2 += d * d;
      }
      sums[(lh * 2 + 0) * W + j * 32 + li] = cok ? s1 : 0.0;
      sums[(lh * 2 + 1) * W + j * 32 + li] = cok ? s2 : 0.0;
    }
    if (full) {
      if (cok) {
        if (cstore) {
#pragma unroll
          for (int i = 0; i < 8; ++i) crow[i][j * 32] = v[i];
        }
        if (EPI == EPI_GATE && a.aux) {
#pragma unroll
          for (int i = 0; i < 8; ++i) xrow[i][j * 32] = g[i];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (cok && rok[i]) {
          if (cstore) crow[i][j * 32] = v[i];
          if (EPI == EPI_GATE && a.aux) xrow[i][j * 32] = g[i];
        }
      }
    }
  }
}

constexpr int X3Q_WPS = 3;   // waves per SIMD the kernel is compiled for (3: <= 168 registers)
// (what each part of the kernel costs, one part removed at a time: profiles/r5_rowgemm_q.txt)

template <int EPI, bool DUAL>
__global__ __launch_bounds__(256, X3Q_WPS) void rowgemm_x3q_k(GemmArgs a, const char* __restrict__ Bp) {
  constexpr int NCH = X3Q_HT * 3;               // 1 KB pieces (64 lanes x 16 B) of a half-slab
  constexpr int NBW = (NCH + 3) / 4;            // DMA instructions per wave and half-slab
  extern __shared__ __align__(16) char smem_q[];          // [2][X3Q_CHUNK]
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lg = lane >> 4;              // MFMA operand coordinates: row (column for B) and k-group
  MRG_GROUP_SELECT(X3Q_ROWS)                                // row0, Bq; a.rows / bias / scale / rowscale of a grouped launch's range
  const int64_t roww = row0 + wave * 16;
  const int K = a.K1 + a.K2;
  const int nslab = (K + 31) >> 5;

  f32x4v acc[X3Q_NT];
#pragma unroll
  for (int n = 0; n < X3Q_NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[n][r] = 0.f;

  // ---- A: this lane's fragment of slab s = row lr, k = 32 s + 8 lg + {0..3, 4..7}: two 16-byte loads
  const float* ar1; const float* ar2;
  x3_a_row(a, roww + lr, ar1, ar2);
  v4f xr[2][2];                                          // raw fragments: a ring of two slabs
  auto load_a = [&](int slab, v4f (&x)[2]) { x3_load_a<32, DUAL>(x, slab, nslab, lg, ar1, ar2, a.K1, a.K2, K); };
  // ---- B: half-slab c = 2 s + half lives in buffer `half`; NBW pieces per wave (the last wave repeats the last piece)
  auto fetch_b = [&](int c) { x3_fetch_b<NCH>(Bq + (int64_t)c * X3Q_CHUNK, smem_q + (c & 1) * X3Q_CHUNK, wave, lane); };
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem_q + (unsigned)lane * 16u;
  u32x4 bq[2][3];                                        // [ping-pong][plane]: the fragments of one column tile
  auto read_b = [&](int t, int buf, u32x4 (&q)[3]) { x3_read_b(lds0 + (unsigned)(buf * X3Q_CHUNK + t * 3072), q); };
  u32x4 ch, cm, cl, nh, nm, nl;
  // ---- prologue.  Issue order of a wave:  A(0) B(0) B(1) A(1) | s = 0, half 1: B(2) A(2) | s = 1, half 0: B(3) | half 1: B(4) A(3) | ...
  load_a(0, xr[0]);
  fetch_b(0);
  fetch_b(1);
  load_a(1, xr[1]);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NBW + 2) : "memory");       // A(0) and this wave's share of B(0) have landed
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) split_pair_of(xr[0], q, ch, cm, cl);
  __builtin_amdgcn_s_barrier();                                          // everybody's share of B(0) is in LDS

  // One half-slab: seven column tiles, six MFMAs each on the tile's own accumulator (a single accumulation chain of this
  // instruction needs no interleaving with other accumulators: MI355X_MICROARCH.md, cycle constants), the next tile's fragments
  // read meanwhile.  SPLIT: the four float pairs of the NEXT slab's activations are split in the shadow of tiles 0..3.
  auto half_slab = [&](auto half_c, auto split_c, const v4f (&xn)[2]) {
    constexpr int HF = decltype(half_c)::value;
    constexpr bool SPLIT = decltype(split_c)::value;
    read_b(0, HF, bq[0]);
#pragma unroll
    for (int t = 0; t < X3Q_HT; ++t) {
      if (t + 1 < X3Q_HT) {
        read_b(t + 1, HF, bq[(t + 1) & 1]);
        asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");       // tile t's fragments are there; the three just issued may be in flight
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
      if (SPLIT && t < 4) split_pair_of(xn, t, nh, nm, nl);
      const bf16x8 Ah = __builtin_bit_cast(bf16x8, ch), Am = __builtin_bit_cast(bf16x8, cm), Al = __builtin_bit_cast(bf16x8, cl);
      const bf16x8 Bh = __builtin_bit_cast(bf16x8, bq[t & 1][0]), Bm = __builtin_bit_cast(bf16x8, bq[t & 1][1]), Bl = __builtin_bit_cast(bf16x8, bq[t & 1][2]);
      x3_chain(acc[HF * X3Q_HT + t], Ah, Am, Al, Bh, Bm, Bl);
      if (SPLIT) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // one MFMA ...
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);     // ... then up to two VALU (an MFMA holds the vector issue for 8 of its 16 cycles)
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // One k-slab of 32; R = s % 2 at compile time (ring position of the raw fragments).
  //   half 0 (buffer 0): [s >= 1: DMA of half-slab 2 s + 1 into buffer 1 -- read last during slab s - 1's half 1, every wave is
  //           past that barrier]; at its end this wave's share of half-slab 2 s + 1 must be in LDS: it is the youngest -> vmcnt(0)
  //           (which also lands A(s + 1), issued half a slab earlier);
  //   half 1 (buffer 1): DMA of half-slab 2 s + 2 into buffer 0, then A(s + 2) into the raw registers slab s - 1 split from;
  //           A(s + 1) is split in the shadow of its first four tiles; at its end only A(s + 2) is younger than the DMA -> vmcnt(2).
  auto slab = [&](auto r_c, int s) {
    constexpr int R = decltype(r_c)::value;
    const bool has_next = s + 1 < nslab;
    if (s > 0) fetch_b(2 * s + 1);
    half_slab(std::integral_constant<int, 0>{}, std::false_type{}, xr[0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (has_next) fetch_b(2 * s + 2);
    load_a(s + 2, xr[R]);
    half_slab(std::integral_constant<int, 1>{}, std::true_type{}, xr[R ^ 1]);
    ch = nh; cm = nm; cl = nl;
    if (has_next) {
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  };
  int s = 0;
  for (; s + 1 < nslab; s += 2) {
    slab(std::integral_constant<int, 0>{}, s);
    slab(std::integral_constant<int, 1>{}, s + 1);
  }
  if (s < nslab) slab(std::integral_constant<int, 0>{}, s);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the tail's unused A fills: their registers must stay until they land
  asm volatile("" :: "v"(xr[0][0]), "v"(xr[0][1]), "v"(xr[1][0]), "v"(xr[1][1]));

  const int li = lane & 31, lh = lane >> 5;
  if constexpr (epi_sums(EPI)) {
    // the weight half-slabs are done with: once every wave has read its last fragments, LDS holds the waves' sums
    // ([4 waves][2 lane halves][2][224] doubles: 28 KB of the 42)
    double* sums = reinterpret_cast<double*>(smem_q);
    __syncthreads();
    gemm_epilogue_q<epi_base(EPI), true>(a, acc, roww, li, lh, row0 + X3Q_ROWS <= a.rows, sums + wave * (4 * X3Q_HT * 32));
    __syncthreads();
    gemm_colsum_flush<X3Q_HT * 32, 8>(sums, gemm_colsum(a), a.N, 0);
  } else {
    gemm_epilogue_q<EPI>(a, acc, roww, li, lh, row0 + X3Q_ROWS <= a.rows);
  }
}

inline bool x3q_eligible(const GemmArgs& a) { return x3_eligible(a) && a.rows > 0 && a.N <= X3Q_NT * 16 && !a.row_seg; }

// Bp: the split of B prepared by launch_bsplitq3
template <int EPI>
inline int launch_rowgemm_x3q(GemmArgs a, const void* Bp, hipStream_t st) {
  if (a.rows <= 0) return MRG_OK;
  if (!a.A2 || a.K2 == 0) { a.A2 = a.A1; a.K2 = 0; }
  const int gbm = X3Q_ROWS;
  if (a.grp.n > 0 && gemm_group_tiles(a.grp, gbm) == 0) return MRG_OK;     // grouped launch: nothing to do
  dim3 grid((unsigned)(a.grp.n > 0 ? a.grp.tile0[3] : (a.rows + gbm - 1) / gbm));
  const size_t lds = (size_t)2 * X3Q_CHUNK;
  if constexpr (EPI == EPI_SEGMAX || EPI == EPI_SEGSUM) {
    return MRG_E_SHAPE;                                   // the fused aggregators' epilogues stay on rowgemm_x3s_k (x3q_shape says so)
  } else {
    if (a.K2 > 0) return launch_kernel(rowgemm_x3q_k<EPI, true>, grid, dim3(256), lds, st, a, Bp);
    return launch_kernel(rowgemm_x3q_k<EPI, false>, grid, dim3(256), lds, st, a, Bp);
  }
}

}  // namespace mrg
