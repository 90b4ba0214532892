// Tall-skinny GEMM on the bf16 matrix pipe with f32-equivalent accuracy ("3-way split"): the wave-autonomous kernel.
//
//   C[rows, N] = epilogue( [A1 | A2][rows, K1+K2] * B[N, K1+K2]^T )          (same contract as gemm.hpp)
//
// The arithmetic (three bf16 planes per f32 operand, six cross terms per product), the weight split and every other part this
// kernel shares with its siblings are in x3_parts.hpp.
//   * B (a weight matrix, a few hundred KB) is split ONCE per call by bsplit_k into fragment order
//     ([k-slab][column tile][plane][lane][8 bf16], one 16-byte load per fragment and plane), and
//   * A (activations, read once from HBM as f32 by LDS-DMA) is split in registers right after its
//     fragment read: 44 VALU instructions per 16 k-columns per wave against 6*NT MFMAs.
// Geometry as gemm.hpp: 256 threads own 128 rows x NT*32 columns, wave w owns rows [32w, 32w+32); k walked in slabs of 16.
// The DMA writes LDS linearly (wave base + lane*16 B), so the A tile is swizzled by choosing WHICH global chunk each lane fetches:
// chunk (row, c) lives at 16-byte slot row*4 + (c ^ ((row >> 2) & 3)), which makes the fragment reads
// (8 consecutive k per lane = two ds_read_b128) bank-conflict free.
#pragma once
#include "x3_parts.hpp"

namespace mrg {

constexpr int X3_VPM = 3;     // VALU instructions the scheduler may place after each MFMA of a tile (lab sweep: 2 / 3 / 4 / 6)

constexpr int X3_THREADS = 256;     // 4 waves, one per SIMD
constexpr int X3_SLOTS = 4;         // per-wave LDS ring of A slabs

// Wave-autonomous kernel: a wave owns MT*32 rows x NT*32 columns and shares NOTHING with the other
// waves of its workgroup -- no barrier anywhere.
//   A: the wave's own [MT*32 rows x 16 k] f32 slab travels HBM -> LDS by DMA into a private 4-slot ring,
//      three slabs ahead; it is read back as fragments (2 ds_read_b128 per row tile) one slab ahead and
//      split into bf16 planes in the shadow of the current slab's MFMAs.
//   B: the pre-split fragments are read straight from global memory (L1/L2 resident: all waves of the chip
//      read the same few hundred KB) into the registers the MFMAs of the previous slab just released.
// With one wave per SIMD (MT = 2: 224 accumulator + ~200 other registers) every latency is covered
// inside the wave's own instruction stream: the in-order vmcnt counter is waited on with the exact number
// of younger operations (3 per column tile, 2*MT per A slab), never drained.
template <int NT, int MT, int EPI, bool DUAL>
__global__ __launch_bounds__(X3_THREADS, 1) void rowgemm_x3_k(GemmArgs a, const char* __restrict__ Bp, int ntile) {   // a and Bp are re-pointed by a grouped launch
  constexpr int WROWS = 32 * MT, GBM = WROWS * (X3_THREADS / 64);
  constexpr int SLOT_CH = WROWS * 4;          // 16-byte chunks per ring slot
  constexpr int NA = SLOT_CH / 64;            // DMA instructions per slab
  constexpr int NBL = 3 * NT;                 // B loads per slab
  constexpr int NPAIR = MT * 4;               // float pairs to split per slab and lane
  constexpr int PP = NT > 1 ? (NPAIR + NT - 2) / (NT - 1) : NPAIR;   // pairs split in the shadow of one column tile
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, lh = lane >> 5;
  MRG_GROUP_SELECT(GBM)                                // row0, Bq; a.rows / bias / scale / rowscale of a grouped launch's range
  const int64_t roww = row0 + wave * WROWS;
  const int col0 = blockIdx.y * (NT * 32);
  const int K = a.K1 + a.K2;
  const int nslab = (K + 15) >> 4;
  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // DMA sources: ring chunk f = lane + 64 i holds (row f/4, 4-float column c = (f%4) ^ ((f/16)&3)) of the slab
  const float* arow1[NA]; const float* arow2[NA]; int acol[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int f = lane + 64 * i;
    const int64_t row = roww + (f >> 2);
    int64_t rc = row < a.rows ? row : a.rows - 1;
    if (a.row_index) rc = a.row_index[rc];                 // gathered rows (EPI_SEGMAX: edges in destination order)
    arow1[i] = a.A1 + rc * a.K1;
    arow2[i] = a.A2 + rc * a.K2;
    acol[i] = 4 * ((f & 3) ^ ((f >> 4) & 3));
  }
  float* ring = smem + wave * a.wave_lds_floats;        // wave-private region: the A ring
  auto fetch_a = [&](int slab) {
    const int k0 = slab * 16;
    float* dst = ring + (slab % X3_SLOTS) * (SLOT_CH * 4);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int k = k0 + acol[i];
      const float* p = gemm_a_ptr<DUAL>(arow1[i], arow2[i], a.K1, a.K2, K, k);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)p, (lds_ptr_t)(dst + 64 * i * 4), 16, 0, 0);
    }
  };
  const unsigned lds_ring = (unsigned)(size_t)(lds_ptr_t)ring;
  unsigned a_off[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int r = 32 * m + li, sw = (r >> 2) & 3;
    a_off[m][0] = (unsigned)((r * 4 + ((2 * lh) ^ sw)) * 16);
    a_off[m][1] = (unsigned)((r * 4 + ((2 * lh + 1) ^ sw)) * 16);
  }
  v4f x[MT][2];                                   // raw fragments of the NEXT slab
  auto read_a = [&](int slab) {
    const unsigned base = lds_ring + (slab % X3_SLOTS) * (SLOT_CH * 16);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      asm volatile("ds_read_b128 %0, %1" : "=v"(x[m][0]) : "v"(base + a_off[m][0]));
      asm volatile("ds_read_b128 %0, %1" : "=v"(x[m][1]) : "v"(base + a_off[m][1]));
    }
  };

  // Asynchronous register fills: the asm statements below return at once, the data arrives later and is first
  // read behind the matching s_waitcnt.  This relies on hipcc keeping each u32x4 in the 4-register tuple the asm
  // wrote (it is exactly the MFMA operand tuple, so there is nothing to copy); a copy scheduled between the load and
  // the wait would read stale registers -- the float64 comparisons of tests/test_ops_gpu.py would catch that.
  u32x4 bq[NT][3];
  const unsigned voff = (unsigned)lane * 16u;
  const char* bcol = Bq + (int64_t)blockIdx.y * NT * 3072;
  auto load_b = [&](int n, int slab) {
    const char* sb = bcol + ((int64_t)slab * ntile + n) * 3072;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(bq[n][0]) : "v"(voff), "s"(sb));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(bq[n][1]) : "v"(voff), "s"(sb));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048" : "=v"(bq[n][2]) : "v"(voff), "s"(sb));
  };

  u32x4 ch[MT], cm[MT], cl[MT];                   // split planes of the CURRENT slab
  u32x4 nh[MT], nm[MT], nl[MT];                   // ... being produced for the next one
  auto split_one = [&](int j, u32x4 (&H)[MT], u32x4 (&M)[MT], u32x4 (&L)[MT]) {   // pair j of 4*MT
    split_pair_of(x[j >> 2], j & 3, H[j >> 2], M[j >> 2], L[j >> 2]);
  };

  // ---- prologue: A slabs 0..2 and B slab 0 in flight; slab 0 split
#pragma unroll
  for (int s = 0; s < 3; ++s)
    if (s < nslab) fetch_a(s);
#pragma unroll
  for (int n = 0; n < NT; ++n) load_b(n, 0);
  wait_vmcnt(NBL);                                // everything older than the B loads has landed
  read_a(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < NPAIR; ++j) split_one(j, ch, cm, cl);

  // One k-slab.  MODE fixes the number of younger vector-memory operations at every wait at compile time
  // (a run-time count costs scalar branches the single wave of a SIMD cannot hide):
  //   0 steady state (s + 3 < nslab)   1: s == nslab-3   2: s == nslab-2   3: s == nslab-1   -1: run-time counts
  auto slab = [&](auto mode_c, int s) {
    constexpr int MODE = decltype(mode_c)::value;
    const bool has_next = MODE < 0 ? (s + 1 < nslab) : (MODE != 3);
    const bool do_dma = MODE < 0 ? (s + 3 < nslab) : (MODE == 0);
    const int dma = do_dma ? NA : 0;
    if (has_next) {
      // A(s+1) was issued two slabs ago; younger: B(s-1) [NBL], A(s+2) [NA if any], B(s) [NBL]
      if (MODE < 0) { if (s >= 2) wait_vmcnt(2 * NBL + ((s + 2 < nslab) ? NA : 0)); }
      else if (MODE == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NBL) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NBL + NA) : "memory");
      read_a(s + 1);
    }
    if (do_dma) fetch_a(s + 3);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      // B(s) tile n: younger = rest of B(s), this slab's A DMA, the B(s+1) tiles issued so far
      if (MODE < 0) wait_vmcnt(3 * (NT - 1 - n) + dma + (has_next ? 3 * n : 0));
      else if (MODE == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (NT - 1) + NA) : "memory");
      else if (MODE == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (NT - 1 - n)) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (NT - 1)) : "memory");
      constexpr int N0 = NT > 1 ? 1 : 0;              // the splits start one tile late: the LDS reads issued at the top have landed by then
      if (n == N0 && has_next) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // raw fragments of the next slab
      __builtin_amdgcn_sched_barrier(0);
      if (has_next && n >= N0) {                      // VALU work for the shadow of this tile's MFMAs
#pragma unroll
        for (int j = (n - N0) * PP; j < (n - N0 + 1) * PP && j < NPAIR; ++j) split_one(j, nh, nm, nl);
      }
      const bf16x8 Bh = __builtin_bit_cast(bf16x8, bq[n][0]), Bm = __builtin_bit_cast(bf16x8, bq[n][1]),
                   Bl = __builtin_bit_cast(bf16x8, bq[n][2]);
      // row tiles interleaved; every accumulator takes its six terms in the order of x3_parts.hpp
      x3_chain_rows(acc, n, ch, cm, cl, Bh, Bm, Bl);
      if (has_next && n == NT - 1) {
#pragma unroll
        for (int m = 0; m < MT; ++m) { ch[m] = nh[m]; cm[m] = nm[m]; cl[m] = nl[m]; }
      }
      // spread the VALU instructions of this tile over the MFMA issue slots: 1 MFMA, then up to 3 VALU
#pragma unroll
      for (int i = 0; i < 6 * MT; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, X3_VPM, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (has_next) load_b(n, s + 1);
    }
  };
  // the host guarantees nslab >= 4 (x3_eligible)
  for (int s = 0; s + 3 < nslab; ++s) slab(std::integral_constant<int, 0>{}, s);
  slab(std::integral_constant<int, 1>{}, nslab - 3);
  slab(std::integral_constant<int, 2>{}, nslab - 2);
  slab(std::integral_constant<int, 3>{}, nslab - 1);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if constexpr (EPI == EPI_SEGMAX) gemm_epilogue_segmax<NT>(a, acc[m], roww + m * 32, col0, li, lh);
    else if constexpr (EPI == EPI_SEGSUM) gemm_epilogue_segsum<NT>(a, acc[m], roww + m * 32, col0, li, lh);
    else gemm_epilogue<NT, EPI>(a, acc[m], roww + m * 32, col0, li, lh, row0 + GBM <= a.rows);
  }
}

inline bool x3_eligible(const GemmArgs& a) {
  return (a.K1 % 4 == 0) && (a.K2 % 4 == 0) && a.K1 >= 4 && (a.K1 + a.K2) > 48 && (a.K2 == 0 || a.K2 >= 4) && aligned16(a.A1) && aligned16(a.A2);
}

// Bp: the split of B prepared by launch_bsplit(..., nt = gemm_pick_nt(a.N), ...)
template <int EPI>
inline int launch_rowgemm_x3(GemmArgs a, const void* Bp, hipStream_t st, int nt_force = 0) {
  if (a.rows <= 0) return MRG_OK;
  if (!a.A2 || a.K2 == 0) { a.A2 = a.A1; a.K2 = 0; }
  const int nt = nt_force > 0 ? nt_force : gemm_pick_nt(a.N);    // nt_force: narrower column blocks for few rows (gemm_dispatch.hpp: x3n_shape)
  const int ntile = x3_tiles(a.N, nt);
  const int mt = a.rows > 128 * 512 ? 2 : 1;            // short operands: more, smaller workgroups
  const int gbm = 32 * mt * (X3_THREADS / 64);
  if (a.grp.n > 0 && gemm_group_tiles(a.grp, gbm) == 0) return MRG_OK;     // grouped launch: nothing to do
  dim3 grid((unsigned)(a.grp.n > 0 ? a.grp.tile0[3] : (a.rows + gbm - 1) / gbm), (unsigned)(ntile / nt));
  const size_t ring_floats = (size_t)X3_SLOTS * 32 * mt * 16;
  a.wave_lds_floats = (int)ring_floats;
  const size_t lds = (size_t)(X3_THREADS / 64) * a.wave_lds_floats * sizeof(float);
#define MRG_GOX2(NTV, MTV, DV) return launch_kernel(rowgemm_x3_k<NTV, MTV, EPI, DV>, grid, dim3(X3_THREADS), lds, st, a, Bp, ntile)
#define MRG_GOX(NTV)                                                                                                  \
  do {                                                                                                                \
    if (mt == 2) { if (a.K2 > 0) MRG_GOX2(NTV, 2, true); else MRG_GOX2(NTV, 2, false); }                              \
    else { if (a.K2 > 0) MRG_GOX2(NTV, 1, true); else MRG_GOX2(NTV, 1, false); }                                      \
  } while (0)
  switch (nt) {
    case 1: MRG_GOX(1); break;
    case 2: MRG_GOX(2); break;
    case 4: MRG_GOX(4); break;
    default: MRG_GOX(7); break;
  }
#undef MRG_GOX
#undef MRG_GOX2
}

}  // namespace mrg
