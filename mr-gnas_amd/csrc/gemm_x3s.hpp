// Split-bf16 row GEMM with the weight operand staged through LDS: 128-row workgroups, two per CU.
//
// What rounds 2 and 3 measured on the wave-autonomous kernels (gemm_x3.hpp, gemm_x3w.hpp; profiles/r2_rowgemm_rounds.txt,
// profiles/r3_rowgemm_epilogue.txt): a wave that keeps the pre-split B fragments of a whole k-slab in registers (84 of them for
// seven column tiles) next to 224 accumulators owns its SIMD's register file, so a CU runs one workgroup whose prologue,
// k-loop and store tail never overlap (MFMA busy 36 % of the wave cycles); and every wave streams the whole weight
// (21 KB per slab) from L2 by itself -- 1.1 MB per 256-row block against 0.2 MB of activations.
//
// Here the four waves of a workgroup SHARE the weight slab: it travels L2 -> LDS once per workgroup by LDS-DMA (double
// buffered, one barrier per slab) and the MFMA operands are read from there (ds_read_b128, conflict free: the pre-split
// layout is already fragment order), so a wave needs only the fragments of the tile it is multiplying.  A wave owns 32 rows
// x NT column tiles (NT * 16 accumulators); the activations are read straight into registers in fragment order (two
// global_load_dwordx4 per slab and lane, two slabs ahead) and split in the shadow of the previous slab's MFMAs.  That is
// <= 256 registers and 3 * NT * 3 KB of LDS per workgroup (the weight slabs two ahead, the activations three ahead -- a
// wave's vector-memory operations complete in issue order, so the two depths are coupled): two workgroups share a CU, and
// while one waits at its barrier, for its first slabs or for its stores, the other multiplies.
// LDS-DMA addresses its destination through M0[15:0]: everything it writes lies below 64 KiB of the workgroup's LDS
// (3 x 21 KB here).
#pragma once
#include "gemm_x3.hpp"

// Tried and dropped, each bit-identical and measured equal (profiles/r4_rowgemm_phases.txt): the barrier that publishes slab s + 1 in
// front of slab s's last tile pair instead of behind it; a branch-free instance of the slab body with a running activation pointer for
// the slabs with s + 4 < nslab (0.407-0.414 vs 0.410-0.414 ms at rows 558 771).  A delayed start of the second workgroup of every CU
// changed nothing measurable either (LAB_NOTES.md).  The part-removal timings (no epilogue / A loads / B DMA / barriers / splits /
// fragment reads, paced stores) are in profiles/r3_rowgemm_lds_weight.txt, profiles/r4_rowgemm_phases.txt and profiles/r4_rowgemm_wide8.txt.

namespace mrg {

// Two waves per SIMD for every NT (three for NT <= 4, at most 168 registers, was tried in the lab).
template <int NT, int EPI, bool DUAL>
__global__ __launch_bounds__(256, 2) void rowgemm_x3s_k(GemmArgs a, const char* __restrict__ Bp, int ntile) {
  constexpr int GBM = 128;
  constexpr int NCH = NT * 3;                   // 1 KB chunks (64 lanes x 16 B) of one pre-split B slab of this column block
  constexpr int BSLAB = NCH * 1024;
  constexpr int NBW = (NCH + 3) / 4;            // DMA instructions per wave and slab
  extern __shared__ __align__(16) char smem_b[];     // [3][BSLAB]: 63 KB for seven column tiles, below the DMA's 64 KiB
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, lh = lane >> 5;
  MRG_GROUP_SELECT(GBM)                                // row0, Bq; a.rows / bias / scale / rowscale of a grouped launch's range
  const int64_t roww = row0 + wave * 32;
  const int col0 = (epi_diag(EPI) ? blockIdx.x : blockIdx.y) * (NT * 32);     // EPI_RANK_DIAG: row block x meets column block x
  const int K = a.K1 + a.K2;
  const int nslab = (K + 15) >> 4;

  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

  // ---- A: this lane's fragment of a slab = row li, k = slab * 16 + lh * 8 + {0..3, 4..7}: two 16-byte loads
  const float* ar1; const float* ar2;
  x3_a_row(a, roww + li, ar1, ar2);
  v4f xr[3][2];                                          // raw fragments: a ring of three slabs
  auto load_a = [&](int slab, v4f (&x)[2]) { x3_load_a<16, DUAL>(x, slab, nslab, lh, ar1, ar2, a.K1, a.K2, K); };
  // ---- B: the slab's NCH chunks, NBW per wave (the last wave repeats the last chunk: same bytes to the same place)
  const char* bcol = Bq + (int64_t)(epi_diag(EPI) ? blockIdx.x : blockIdx.y) * NT * 3072;
  auto fetch_b = [&](int slab, int buf) { x3_fetch_b<NCH>(bcol + (int64_t)slab * ntile * 3072, smem_b + buf * BSLAB, wave, lane); };
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem_b + (unsigned)lane * 16u;
  u32x4 bq2[2][2][3];                                    // [double buffer][tile of the pair][plane]
  auto read_b = [&](int n, int buf, u32x4 (&q)[3]) { x3_read_b(lds0 + (unsigned)(buf * BSLAB + n * 3072), q); };
  u32x4 ch, cm, cl, nh, nm, nl;
  auto nb_issued = [&](int j) { return (j >= -2 && j + 2 < nslab) ? NBW : 0; };   // B DMAs issued at the top of slab j (j < 0: prologue)
  constexpr int NP = (NT + 1) / 2;                          // column-tile pairs per slab

  // ---- prologue, in the steady state's issue order: A(0) | B(0) A(1) | B(1) A(2)
  load_a(0, xr[0]);
  fetch_b(0, 0);
  load_a(1, xr[1]);
  if (nslab > 1) fetch_b(1, 1);
  load_a(2, xr[2]);
  wait_vmcnt(2 + nb_issued(-1) + 2);                         // A(0) and this wave's share of B(0) have landed
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) split_pair_of(xr[0], q, ch, cm, cl);
  __builtin_amdgcn_s_barrier();                              // everybody's share of B(0) is in LDS

  // One k-slab; R = s % 3 at compile time (ring positions of the raw fragments and of the B buffers).
  // In-order vector-memory history of a wave at the top of slab s:  ... A(s+1) | B(s+1) A(s+2)      (B(s) in LDS: barrier)
  //   top: issue B(s+2) into buffer (s+2) % 3 -- read last during slab s-1, every wave is past that barrier -- and A(s+3) into
  //        the raw registers slab s-1 split from;
  //   the splits need A(s+1): younger = B(s+1) A(s+2) B(s+2) A(s+3);
  //   end: B(s+1) must be in LDS before the barrier: younger = A(s+2) B(s+2) A(s+3).
  auto slab = [&](auto r_c, int s) {
    constexpr int R = decltype(r_c)::value;
    const bool has_next = s + 1 < nslab;
    if (s + 2 < nslab) fetch_b(s + 2, (R + 2) % 3);
    load_a(s + 3, xr[R]);
    // Column tiles in PAIRS: the twelve MFMAs of a pair alternate between its two accumulators (a dependent MFMA issued back to
    // back waits for its predecessor's result; with another accumulator's MFMA in between the pipe stays busy) and the VALU
    // instructions of the A split are spread between them (sched_group_barrier: 1 MFMA, then up to 3 VALU) instead of
    // standing in front of the MFMAs.  Each accumulator still receives its six terms in the same order: bit-identical results.
    constexpr int SPP = (4 + NP - 1) / NP;                    // split pairs handled in the shadow of one tile pair
    read_b(0, R, bq2[0][0]);
    if (NT > 1) read_b(1, R, bq2[0][1]);
    if (has_next) wait_vmcnt(nb_issued(s - 1) + 2 + nb_issued(s) + 2);     // A(s+1) is split during this slab
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      const int n0 = 2 * pp, n1 = 2 * pp + 1;
      if (pp + 1 < NP) {
        read_b(n0 + 2, R, bq2[(pp + 1) & 1][0]);
        if (n1 + 2 < NT) {
          read_b(n1 + 2, R, bq2[(pp + 1) & 1][1]);
          asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");   // the reads just issued may still be in flight
        } else {
          asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
        }
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
      if (has_next) {
#pragma unroll
        for (int q = pp * SPP; q < (pp + 1) * SPP && q < 4; ++q) split_pair_of(xr[(R + 1) % 3], q, nh, nm, nl);
      }
      const bf16x8 Ah = __builtin_bit_cast(bf16x8, ch), Am = __builtin_bit_cast(bf16x8, cm), Al = __builtin_bit_cast(bf16x8, cl);
      const bf16x8 Bh0 = __builtin_bit_cast(bf16x8, bq2[pp & 1][0][0]), Bm0 = __builtin_bit_cast(bf16x8, bq2[pp & 1][0][1]),
                   Bl0 = __builtin_bit_cast(bf16x8, bq2[pp & 1][0][2]);
      if (n1 < NT) {
        const bf16x8 Bh1 = __builtin_bit_cast(bf16x8, bq2[pp & 1][1][0]), Bm1 = __builtin_bit_cast(bf16x8, bq2[pp & 1][1][1]),
                     Bl1 = __builtin_bit_cast(bf16x8, bq2[pp & 1][1][2]);
        x3_chain2(acc[n0], acc[n1], Ah, Am, Al, Bh0, Bm0, Bl0, Ah, Am, Al, Bh1, Bm1, Bl1);
      } else {
        x3_chain(acc[n0], Ah, Am, Al, Bh0, Bm0, Bl0);
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // one MFMA ...
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);     // ... then up to three VALU
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (NT < 4 && has_next) {
#pragma unroll
      for (int q = NT; q < 4; ++q) split_pair_of(xr[(R + 1) % 3], q, nh, nm, nl);
    }
    if (has_next) {
      ch = nh; cm = nm; cl = nl;
      wait_vmcnt(2 + nb_issued(s) + 2);                      // this wave's share of B(s+1) is in LDS
      __builtin_amdgcn_s_barrier();                          // ... and everybody's; all reads of this slab's buffer are done
    }
  };
  int s = 0;
  for (; s + 2 < nslab; s += 3) {
    slab(std::integral_constant<int, 0>{}, s);
    slab(std::integral_constant<int, 1>{}, s + 1);
    slab(std::integral_constant<int, 2>{}, s + 2);
  }
  if (s < nslab) { slab(std::integral_constant<int, 0>{}, s); ++s; }
  if (s < nslab) { slab(std::integral_constant<int, 1>{}, s); ++s; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the tail's unused A fills: their registers must stay until they land
  asm volatile("" :: "v"(xr[0][0]), "v"(xr[0][1]), "v"(xr[1][0]), "v"(xr[1][1]), "v"(xr[2][0]), "v"(xr[2][1]));

  constexpr int EPU = epi_unbiased(EPI);
  if constexpr (epi_col_bias(EPI)) gemm_add_col_bias<NT>(a, acc, col0, li);     // the sweeps under a per-entity score bias
  if constexpr (epi_sums(EPI)) {
    // the weight slabs are done with: once every wave has read its last fragments, LDS holds the waves' sums
    // ([4 waves][2 lane halves][2][NT * 32] doubles: 28 KB of the 63 for seven tiles)
    double* sums = reinterpret_cast<double*>(smem_b);
    __syncthreads();
    gemm_epilogue<NT, epi_base(EPI), true>(a, acc, roww, col0, li, lh, row0 + GBM <= a.rows, sums + wave * (4 * NT * 32));
    __syncthreads();
    gemm_colsum_flush<NT * 32, 8>(sums, gemm_colsum(a), a.N, col0);
  }
  else if constexpr (EPI == EPI_SEGMAX) gemm_epilogue_segmax<NT>(a, acc, roww, col0, li, lh);
  else if constexpr (EPI == EPI_SEGSUM) gemm_epilogue_segsum<NT>(a, acc, roww, col0, li, lh);
  else if constexpr (EPU == EPI_RANK) gemm_epilogue_rank<NT>(a, acc, roww, col0, li, lh);
  else if constexpr (EPU == EPI_RANK_DIAG) gemm_epilogue_rank_diag<NT>(a, acc, roww, wave, li, lh);
  else if constexpr (EPU == EPI_TOPK) gemm_epilogue_topk<NT>(a, acc, roww, col0, li, lh);
  else if constexpr (EPU == EPI_BCE) gemm_bce_flush(a, gemm_epilogue_bce<NT>(a, acc, roww, col0, li, lh), reinterpret_cast<double*>(smem_b));
  else if constexpr (EPU == EPI_BCE_GRAD) gemm_epilogue_bce_grad<NT>(a, acc, roww, col0, li, lh, row0 + GBM <= a.rows);
  else gemm_epilogue<NT, EPI>(a, acc, roww, col0, li, lh, row0 + GBM <= a.rows);
}

inline bool x3s_eligible(const GemmArgs& a) { return x3_eligible(a) && a.rows > 0; }

// Bp: the split of B prepared by launch_bsplit(..., nt = gemm_pick_nt(a.N), ...)
template <int EPI>
inline int launch_rowgemm_x3s(GemmArgs a, const void* Bp, hipStream_t st) {
  if (a.rows <= 0) return MRG_OK;
  if (!a.A2 || a.K2 == 0) { a.A2 = a.A1; a.K2 = 0; }
  const int nt = gemm_pick_nt(a.N);
  const int ntile = x3_tiles(a.N, nt);
  const int gbm = 128;
  if (a.grp.n > 0 && gemm_group_tiles(a.grp, gbm) == 0) return MRG_OK;     // grouped launch: nothing to do
  dim3 grid((unsigned)(a.grp.n > 0 ? a.grp.tile0[3] : (a.rows + gbm - 1) / gbm), (unsigned)(ntile / nt));
  size_t lds = (size_t)3 * nt * 3 * 1024;
#define MRG_GOS2(NTV, DV) return launch_kernel(rowgemm_x3s_k<NTV, EPI, DV>, grid, dim3(256), lds, st, a, Bp, ntile)
#define MRG_GOS(NTV) do { if (a.K2 > 0) MRG_GOS2(NTV, true); else MRG_GOS2(NTV, false); } while (0)
  switch (nt) {
    case 1: MRG_GOS(1); break;
    case 2: MRG_GOS(2); break;
    case 4: MRG_GOS(4); break;
    default: MRG_GOS(7); break;
  }
#undef MRG_GOS
#undef MRG_GOS2
}

// EPI_GATE_SUMS / EPI_SCALE_SUMS: the seven-tile column block (129..224 columns), accumulator-order epilogue; gemm_set_colsum(a, ...) done
template <int EPI>
inline int launch_rowgemm_x3s_colsum(GemmArgs a, const void* Bp, hipStream_t st) {
  static_assert(epi_sums(EPI), "the column-sum epilogues");
  if (a.rows <= 0) return MRG_OK;
  if (!a.A2 || a.K2 == 0) { a.A2 = a.A1; a.K2 = 0; }
  const int nt = gemm_pick_nt(a.N);
  if (nt != 7 || a.N > 7 * 32 || !gemm_colsum(a)) return MRG_E_SHAPE;
  const int ntile = x3_tiles(a.N, nt);
  if (a.grp.n > 0 && gemm_group_tiles(a.grp, 128) == 0) return MRG_OK;
  dim3 grid((unsigned)(a.grp.n > 0 ? a.grp.tile0[3] : (a.rows + 127) / 128), 1);
  const size_t lds = (size_t)3 * nt * 3 * 1024;
  if (a.K2 > 0) return launch_kernel(rowgemm_x3s_k<7, EPI, true>, grid, dim3(256), lds, st, a, Bp, ntile);
  return launch_kernel(rowgemm_x3s_k<7, EPI, false>, grid, dim3(256), lds, st, a, Bp, ntile);
}

}  // namespace mrg
