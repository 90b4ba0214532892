// The weight gradient of the dense linears (linear.hip holds their forward and input gradient): a split-over-rows GEMM.  Each
// workgroup reduces a chunk of rows into register-resident output tiles, the partial tiles are combined in a fixed order; software
// pipelined, optionally dual-source.
// Matrix cores: split bf16 by default (wgrad_x3v_k / wgrad_x3_k; shared arithmetic x3_parts.hpp), exact f32 (wgrad_dma_k / wgrad_k;
// their plan and the list of their instances: wgrad_plan.hpp) in mode 1 and for operands the split core cannot take.
#include "x3_parts.hpp"
#include "wgrad_plan.hpp"

static_assert(mrg::WGRAD_BLOCK == MRG_BLOCK, "wgrad_plan.hpp plans for workgroups of MRG_BLOCK threads");

namespace mrg {

// Weight gradient: partial[g][n][c] = sum over the workgroup's rows r of gY[r][n] * X'[r][c],
// X' = [X1 | X2 | 1] (the appended column of ones yields the bias gradient for free).  WBR rows per LDS tile.
struct WgradArgs {
  const float* gY; int Nout; int ldg;        // [rows][ldg], Nout valid columns (a column block of a wider gradient)
  const float* X1; const float* X2; int K1, K2;
  float* ws;
  int64_t rows, rows_per_block;
  int TM, TN, TNB;
  // grouped launch (wgrad_x3_k / wgrad_reduce3_k, gridDim.z = 3): row range, plan and partial-tile workspace of range z
  int ngrp;
  int64_t g_lo[3], g_hi[3], g_rpb[3], g_ws_off[3];      // g_ws_off in floats
  int g_G[3];
};

// X' = [X1 | X2 | 1 | 0...]: which tensor / local column a global column c maps to
struct XSel { const float* base; int ld, kk; };
__device__ __forceinline__ XSel wgrad_sel_x(const WgradArgs& a, int c) {
  const bool first = c < a.K1 || a.K2 == 0;
  XSel s;
  s.base = first ? a.X1 : a.X2;
  s.ld = first ? a.K1 : a.K2;
  s.kk = first ? c : c - a.K1;
  return s;
}

// Operands of any size and alignment: scalar loads with per-element source selection (16-byte rows go to wgrad_dma_k).
template <int TPW, int NPF>      // TPW accumulator tiles per wave, NPF prefetch float4 per thread
__global__ __launch_bounds__(MRG_BLOCK, 2) void wgrad_k(WgradArgs a) {      // TPW <= 7: 112 accumulator registers, two workgroups per CU
  extern __shared__ __align__(16) float smem[];
  const int tn0 = (int)(((int64_t)blockIdx.y * a.TN) / gridDim.y);                 // balanced split of the column tiles
  const int tnb = (int)(((int64_t)(blockIdx.y + 1) * a.TN) / gridDim.y) - tn0;
  const int ldg = a.TM * 32, ldx = tnb * 32, stage = WBR * (ldg + a.TNB * 32);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int ntiles = a.TM * tnb;
  const int g4 = ldg / 4, x4 = ldx / 4, nf4 = WBR * (g4 + x4);      // float4 per staged tile
  f32x16 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int64_t r_begin = (int64_t)blockIdx.x * a.rows_per_block;
  int64_t r_end = r_begin + a.rows_per_block;
  if (r_end > a.rows) r_end = a.rows;

  float4 pf[NPF];
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      int f = tid + i * MRG_BLOCK;
      // every lane issues ONE load from a clamped address; which operand it is, is a select
      const bool isg = f < WBR * g4;
      const int f2 = isg ? f : (f < nf4 ? f - WBR * g4 : 0);
      const int per = isg ? g4 : x4;
      const int r = f2 / per, c4 = f2 - r * per;
      const int64_t rc = r0 + r < r_end ? r0 + r : r_end - 1;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const XSel sx = wgrad_sel_x(a, tn0 * 32 + c4 * 4 + j);
        const float* base = isg ? a.gY : sx.base;
        const int ld = isg ? a.Nout : sx.ld;
        const int kk = isg ? c4 * 4 + j : sx.kk;
        v[j] = base[rc * ld + (kk < ld ? kk : ld - 1)];
      }
      pf[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
  };
  auto stash = [&](int buf, int64_t r0) {
    const int K = a.K1 + a.K2;
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      int f = tid + i * MRG_BLOCK;
      if (f < nf4) {
        const bool isg = f < WBR * g4;
        const int f2 = isg ? f : f - WBR * g4;
        const int per = isg ? g4 : x4;
        const int r = f2 / per, c4 = f2 - r * per;
        const int c = tn0 * 32 + c4 * 4;
        // columns are valid up to Nout (gY) or K (X'); the ones column is set below
        float4 v = gemm_mask4<false>(pf[i], r0 + r, r_end, isg ? c4 * 4 : c, isg ? a.Nout : K);
        if (!isg && r0 + r < r_end) {            // the appended column of ones
          if (c == K) v.x = 1.0f;
          if (c + 1 == K) v.y = 1.0f; if (c + 2 == K) v.z = 1.0f; if (c + 3 == K) v.w = 1.0f;
        }
        *reinterpret_cast<float4*>(&smem[buf * stage + f * 4]) = v;                    // Gs then Xs, both dense row-major
      }
    }
  };

  if (r_begin < r_end) {
    fetch(r_begin);
    stash(0, r_begin);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += WBR) {
    const bool more = r0 + WBR < r_end;
    if (more) fetch(r0 + WBR);
    const float* Gs = smem + cur * stage;
    const float* Xs = Gs + WBR * ldg;
#pragma unroll 1
    for (int t = 0; t < WBR / 2; ++t) {
      const float* grow = Gs + (2 * t + lh) * ldg + li;
      const float* xrow = Xs + (2 * t + lh) * ldx + li;
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int id = wave + 4 * i;
        if (id < ntiles) {
          const int m = id / tnb, n = id - m * tnb;
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[m * 32], xrow[n * 32], acc[i], 0, 0, 0);
        }
      }
    }
    if (more) {
      stash(cur ^ 1, r0 + WBR);
      __syncthreads();
      cur ^= 1;
    }
  }
  const int ldw = a.TN * 32;
  float* out = a.ws + (int64_t)blockIdx.x * ldg * ldw;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int id = wave + 4 * i;
    if (id < ntiles) {
      const int m = id / tnb, n = id - m * tnb;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        out[(int64_t)row * ldw + (tn0 + n) * 32 + li] = acc[i][r];
      }
    }
  }
}

// ---- LDS-DMA variant of the weight gradient (vector path) -------------------------------------
// Tiles go global -> LDS with global_load_lds_dwordx4 (no register staging, no ds_write); the DMA
// cannot synthesise values, so rows beyond the chunk and padding columns are sourced from a block
// of zeros and the appended bias column from a {1,0,0,0} constant.  MFMA operands are read with
// inline-asm ds_read_b32 so that hipcc does not drain the in-flight DMA before every LDS read.
static __device__ float mrg_zeros16[4] = {0.f, 0.f, 0.f, 0.f};
static __device__ float mrg_ones16[4] = {1.f, 0.f, 0.f, 0.f};

template <int TPW, int NPF>
__global__ __launch_bounds__(MRG_BLOCK, 2) void wgrad_dma_k(WgradArgs a) {
  extern __shared__ __align__(16) float smem[];
  const int tn0 = (int)(((int64_t)blockIdx.y * a.TN) / gridDim.y);
  const int tnb = (int)(((int64_t)(blockIdx.y + 1) * a.TN) / gridDim.y) - tn0;
  const int ldg = a.TM * 32, ldx = tnb * 32, stage = WBR * (ldg + a.TNB * 32);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int g4 = ldg / 4, x4 = ldx / 4, nf4 = WBR * (g4 + x4);
  const int K = a.K1 + a.K2;
  f32x16 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int64_t r_begin = (int64_t)blockIdx.x * a.rows_per_block;
  int64_t r_end = r_begin + a.rows_per_block;
  if (r_end > a.rows) r_end = a.rows;

  // loop-invariant DMA metadata of this thread's float4 slots
  const float* src[NPF]; int64_t stride[NPF]; int rr[NPF]; int kind[NPF];     // kind: 0 data, 1 ones, 2 zeros
#pragma unroll
  for (int i = 0; i < NPF; ++i) {
    const int f = tid + i * MRG_BLOCK;
    const bool isg = f < WBR * g4;
    const int f2 = isg ? f : (f < nf4 ? f - WBR * g4 : 0);
    const int per = isg ? g4 : x4;
    const int r = f2 / per, c = (f2 - r * per) * 4 + (isg ? 0 : tn0 * 32);
    rr[i] = r;
    if (isg) {
      kind[i] = c < a.Nout ? 0 : 2;
      src[i] = a.gY + (r_begin + r) * a.ldg + (c < a.Nout ? c : 0);
      stride[i] = (int64_t)WBR * a.ldg;
    } else {
      const XSel sx = wgrad_sel_x(a, c < K ? c : 0);
      kind[i] = c < K ? 0 : (c == K ? 1 : 2);
      src[i] = sx.base + (r_begin + r) * sx.ld + sx.kk;
      stride[i] = (int64_t)WBR * sx.ld;
    }
  }
  auto fetch = [&](int buf, int64_t r0, int64_t tile) {
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int f = tid + i * MRG_BLOCK;
      if (f - lane < nf4) {                                 // wave-uniform: this wave-instruction has work
        const bool rv = r0 + rr[i] < r_end;
        const float* p = (rv && kind[i] == 0) ? src[i] + tile * stride[i] : ((rv && kind[i] == 1) ? mrg_ones16 : mrg_zeros16);
        if (f < nf4)
          __builtin_amdgcn_global_load_lds((gbl_ptr_t)p, (lds_ptr_t)(smem + buf * stage + (f - lane) * 4), 16, 0, 0);
      }
    }
  };
  // per-tile LDS byte offsets of this lane's operands
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
  // wave w owns column tile n = w of the block (tnb <= 4) and every row tile m = i: one X' fragment read
  // feeds TM MFMAs (LDS delivers 64 B/clk per CU; two fragment reads per 64-cycle MFMA on 8 waves saturate it)
  unsigned goff[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) goff[i] = (unsigned)((lh * ldg + (i < a.TM ? i : 0) * 32 + li) * 4);
  const unsigned xoff = (unsigned)((WBR * ldg + lh * ldx + (wave < tnb ? wave : 0) * 32 + li) * 4);
  const bool active = wave < tnb;
  // 3-slot LDS ring: the DMA runs two 16-row tiles (~3 us of MFMA time) ahead; vmcnt is waited on with the
  // number of younger DMA instructions of this wave, never drained
  int per_tile = 0;
#pragma unroll
  for (int i = 0; i < NPF; ++i) per_tile += (wave * 64 + i * MRG_BLOCK < nf4) ? 1 : 0;
  if (r_begin < r_end) fetch(0, r_begin, 0);
  if (r_begin + WBR < r_end) fetch(1, r_begin + WBR, 1);
  int cur = 0;
  int64_t tile = 0;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += WBR, ++tile) {
    wait_vmcnt(r0 + WBR < r_end ? per_tile : 0);           // tile `tile` has landed (this wave's part) ...
    __builtin_amdgcn_s_barrier();                          // ... everyone's part; all reads of the previous tile are done
    if (r0 + 2 * WBR < r_end) fetch(cur >= 1 ? cur - 1 : 2, r0 + 2 * WBR, tile + 2);   // slot (tile + 2) % 3
    const unsigned base = lds0 + cur * stage * 4;
    // fragment reads of k-step t+1 are in flight while the MFMAs of k-step t issue
    float gv[2][TPW], xv[2];
    auto frag = [&](int b, int t) {
      asm volatile("ds_read_b32 %0, %1" : "=v"(xv[b]) : "v"(base + xoff + t * 2 * ldx * 4));
#pragma unroll
      for (int i = 0; i < TPW; ++i) asm volatile("ds_read_b32 %0, %1" : "=v"(gv[b][i]) : "v"(base + goff[i] + t * 2 * ldg * 4));
    };
    frag(0, 0);
#pragma unroll
    for (int t = 0; t < WBR / 2; ++t) {
      const int c = t & 1;
      if (t + 1 < WBR / 2) {
        frag(c ^ 1, t + 1);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TPW + 1) : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
      if (active) {
#pragma unroll
        for (int i = 0; i < TPW; ++i)
          if (i < a.TM) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[c][i], xv[c], acc[i], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    cur = cur == 2 ? 0 : cur + 1;
  }
  const int ldw = a.TN * 32;
  float* out = a.ws + (int64_t)blockIdx.x * ldg * ldw;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    if (active && i < a.TM) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        out[(int64_t)row * ldw + (tn0 + wave) * 32 + li] = acc[i][r];
      }
    }
  }
}

// ---- split-bf16 weight gradient (see gemm_x3.hpp for the arithmetic) ------------------------------
// Both operands are activations here, so both are split in registers.  512 threads = 8 waves (two per SIMD:
// the splits of one wave run under the MFMAs of the other); the workgroup owns all TM <= 7 row tiles of gW
// and KT = 8 (NG = 2) or 16 (NG = 1, TM <= 4) column tiles; wave (g, p) owns row tiles [4g, 4g+4) x column
// tiles {2p, 2p+1}: 6 fragments are split (264 VALU instructions) for 48 MFMAs per 16 rows.
// LDS: 4-slot ring (the DMA runs three tiles ahead) of [16 rows][A: 57 chunks | B: KT*8+1 chunks] (16-byte chunks; the odd pitch makes the
// transposed fragment reads -- 8 ds_read_b32, rows 8h..8h+7 of one column per lane -- conflict free).
constexpr int WX_THREADS = 512;
constexpr int WX_APITCH = 57 * 4;            // floats per A row in LDS (224 columns + one pad chunk)
// Tile shape and dynamic LDS of the split-core kernels, NG = 1 (TM <= 4) or 2 (TM <= 7): read by the kernels and by launch_wgrad_x3.
template <int NG>
struct WgradX3 {
  static constexpr int KP = 8 / NG, KT = 2 * KP;          // column-tile pairs / column tiles per workgroup
  // wgrad_x3_k: a ring of SLOTS raw f32 tiles (the DMA runs SLOTS-1 tiles ahead) of STAGE_CH 16-byte chunks
  static constexpr int SLOTS = NG == 2 ? 4 : 3, STAGE_CH = WBR * (WX_APITCH / 4) + WBR * (KT * 8 + 1);
  static constexpr size_t LDS_RAW = (size_t)SLOTS * STAGE_CH * 16;
  // wgrad_x3v_k: ASLOTS row-tile slots (TM <= 7 / <= 4), FPW fragments per wave and tile, each three bf16 planes of 1024 bytes; two buffers
  static constexpr int ASLOTS = NG == 2 ? 8 : 4, FPW = (ASLOTS + KT + 7) / 8, FRAG_BYTES = 3 * 1024;
  static constexpr unsigned BUF_BYTES = FPW * 8 * FRAG_BYTES;
  static constexpr size_t LDS_SPLIT = (size_t)2 * BUF_BYTES;
};

// wgrad_x3_k and wgrad_x3v_k share the arithmetic (x3_parts.hpp: split8, x3_chain, x3_chain2).  Their 40-line head (tile ownership,
// accumulator clear, row range of a grouped launch) and their 12-line store tail stay spelled out in both: as helpers (a struct
// returned by value, the accumulator array passed by reference) they compile to equivalent but not identical code, and
// wgrad_x3v_k, at 255 registers, spilled with the clear alone moved out.
template <int NG>
__global__ __launch_bounds__(WX_THREADS, 1) void wgrad_x3_k(WgradArgs a) {
  using X = WgradX3<NG>;
  constexpr int KP = X::KP, KT = X::KT, SLOTS = X::SLOTS, STAGE_CH = X::STAGE_CH;
  constexpr int BPITCH = (KT * 8 + 1) * 4;
  constexpr int ACH = WBR * 57;
  constexpr int NPF = (STAGE_CH + WX_THREADS - 1) / WX_THREADS;
  extern __shared__ __align__(16) float smem[];
  const int tn0 = (int)(((int64_t)blockIdx.y * a.TN) / gridDim.y);
  const int tnb = (int)(((int64_t)(blockIdx.y + 1) * a.TN) / gridDim.y) - tn0;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wg = wave / KP, wp = wave % KP;
  const int m0 = wg * 4;
  const int an = a.TM - m0 < 4 ? (a.TM - m0 > 0 ? a.TM - m0 : 0) : 4;      // row tiles of this wave
  const int kn = tnb - 2 * wp < 2 ? (tnb - 2 * wp > 0 ? tnb - 2 * wp : 0) : 2;   // column tiles of this wave
  const int K = a.K1 + a.K2;

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int64_t r_begin = (int64_t)blockIdx.x * a.rows_per_block;
  int64_t r_end = r_begin + a.rows_per_block;
  if (r_end > a.rows) r_end = a.rows;
  int64_t ws_off = 0;
  if (a.ngrp > 0) {                                       // one row range per blockIdx.z (constant indices: no scratch copy of the arguments)
    const int z = blockIdx.z;
#define MRG_PICKZ(F) (z == 0 ? a.F[0] : (z == 1 ? a.F[1] : a.F[2]))
    if ((int)blockIdx.x >= MRG_PICKZ(g_G)) return;          // workgroup-uniform, before any barrier
    const int64_t rpb = MRG_PICKZ(g_rpb), hi = MRG_PICKZ(g_hi);
    r_begin = MRG_PICKZ(g_lo) + (int64_t)blockIdx.x * rpb;
    r_end = r_begin + rpb < hi ? r_begin + rpb : hi;
    ws_off = MRG_PICKZ(g_ws_off);
#undef MRG_PICKZ
  }

  // loop-invariant DMA metadata of this thread's chunks
  const float* src[NPF]; int64_t stride[NPF]; int rr[NPF]; int kind[NPF];     // kind: 0 data, 1 ones, 2 zeros
#pragma unroll
  for (int i = 0; i < NPF; ++i) {
    const int f = tid + i * WX_THREADS;
    const bool isg = f < ACH;
    const int f2 = isg ? f : (f < STAGE_CH ? f - ACH : 0);
    const int per = isg ? 57 : KT * 8 + 1;
    const int r = f2 / per, c = (f2 - r * per) * 4;
    rr[i] = r;
    if (isg) {
      kind[i] = c < a.Nout ? 0 : 2;
      src[i] = a.gY + (r_begin + r) * a.ldg + (c < a.Nout ? c : 0);
      stride[i] = (int64_t)WBR * a.ldg;
    } else {
      const int cg = tn0 * 32 + c;
      const bool incol = c < tnb * 32;
      const XSel sx = wgrad_sel_x(a, (incol && cg < K) ? cg : 0);
      kind[i] = (incol && cg < K) ? 0 : ((incol && cg == K) ? 1 : 2);
      src[i] = sx.base + (r_begin + r) * sx.ld + sx.kk;
      stride[i] = (int64_t)WBR * sx.ld;
    }
  }
  int per_tile = 0;
#pragma unroll
  for (int i = 0; i < NPF; ++i) per_tile += (wave * 64 + i * WX_THREADS < STAGE_CH) ? 1 : 0;
  auto fetch = [&](int buf, int64_t r0, int64_t tile) {
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int f = tid + i * WX_THREADS;
      if (f - lane < STAGE_CH) {                            // wave-uniform
        const bool rv = r0 + rr[i] < r_end;
        const float* p = (rv && kind[i] == 0) ? src[i] + tile * stride[i] : ((rv && kind[i] == 1) ? mrg_ones16 : mrg_zeros16);
        if (f < STAGE_CH)
          __builtin_amdgcn_global_load_lds((gbl_ptr_t)p, (lds_ptr_t)(smem + (buf * STAGE_CH + (f - lane)) * 4), 16, 0, 0);
      }
    }
  };

  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
  const unsigned a_off = (unsigned)((8 * lh * WX_APITCH + m0 * 32 + li) * 4);
  const unsigned b_off = (unsigned)((ACH * 4 + 8 * lh * BPITCH + 2 * wp * 32 + li) * 4);
  // one fragment: rows 8h..8h+7 of one column, split into three bf16 planes
  auto frag = [&](unsigned addr, auto pitch_c, u32x4& H, u32x4& M, u32x4& L) {
    constexpr int PB = decltype(pitch_c)::value * 4;
    float v[8];
    asm volatile("ds_read_b32 %0, %1" : "=v"(v[0]) : "v"(addr));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[1]) : "v"(addr), "n"(PB));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[2]) : "v"(addr), "n"(2 * PB));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[3]) : "v"(addr), "n"(3 * PB));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[4]) : "v"(addr), "n"(4 * PB));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[5]) : "v"(addr), "n"(5 * PB));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[6]) : "v"(addr), "n"(6 * PB));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[7]) : "v"(addr), "n"(7 * PB));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    split8(v, H, M, L);
  };

  if (r_begin < r_end) fetch(0, r_begin, 0);
#pragma unroll
  for (int t = 1; t < SLOTS - 1; ++t)
    if (r_begin + t * WBR < r_end) fetch(t, r_begin + t * WBR, t);
  int cur = 0;
  int64_t tile = 0;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += WBR, ++tile) {
    {                                                      // younger DMA: the tiles already issued behind this one
      int64_t left = (r_end - r0 + WBR - 1) / WBR - 1;
      wait_vmcnt((int)(left < SLOTS - 2 ? left : SLOTS - 2) * per_tile);
    }
    __builtin_amdgcn_s_barrier();
    if (r0 + (SLOTS - 1) * WBR < r_end)                    // into the slot read during the previous tile
      fetch(cur == 0 ? SLOTS - 1 : cur - 1, r0 + (SLOTS - 1) * WBR, tile + SLOTS - 1);
    const unsigned base = lds0 + cur * (STAGE_CH * 16);
    if (an > 0 && kn > 0) {
      u32x4 bh[2], bm[2], bl[2];
      frag(base + b_off, std::integral_constant<int, BPITCH>{}, bh[0], bm[0], bl[0]);
      if (kn > 1) frag(base + b_off + 128, std::integral_constant<int, BPITCH>{}, bh[1], bm[1], bl[1]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < an) {
          u32x4 ah, am, al;
          frag(base + a_off + i * 128, std::integral_constant<int, WX_APITCH>{}, ah, am, al);
          const bf16x8 Ah = __builtin_bit_cast(bf16x8, ah), Am = __builtin_bit_cast(bf16x8, am), Al = __builtin_bit_cast(bf16x8, al);
          const bf16x8 Bh0 = __builtin_bit_cast(bf16x8, bh[0]), Bm0 = __builtin_bit_cast(bf16x8, bm[0]), Bl0 = __builtin_bit_cast(bf16x8, bl[0]);
          if (kn > 1) {                                    // two accumulators interleaved: no back-to-back dependent MFMAs
            const bf16x8 Bh1 = __builtin_bit_cast(bf16x8, bh[1]), Bm1 = __builtin_bit_cast(bf16x8, bm[1]), Bl1 = __builtin_bit_cast(bf16x8, bl[1]);
            x3_chain2(acc[i][0], acc[i][1], Ah, Am, Al, Bh0, Bm0, Bl0, Ah, Am, Al, Bh1, Bm1, Bl1);
          } else {
            x3_chain(acc[i][0], Ah, Am, Al, Bh0, Bm0, Bl0);
          }
        }
      }
    }
    cur = cur == SLOTS - 1 ? 0 : cur + 1;
  }
  const int ldw = a.TN * 32;
  float* out = a.ws + ws_off + (int64_t)blockIdx.x * (a.TM * 32) * ldw;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (i < an && j < kn) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (m0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          out[(int64_t)row * ldw + (tn0 + 2 * wp + j) * 32 + li] = acc[i][j][r];
        }
      }
}

// ---- the same weight gradient with every fragment split ONCE per workgroup ------------------------------------------------
// wgrad_x3_k stages raw f32 tiles in LDS and every wave splits the fragments it multiplies: a gY fragment is split by the four
// waves that share its row tiles, an X fragment by two -- 264 VALU instructions per wave and 16-row tile beside 48 MFMAs, and
// eight ds_read_b32 per fragment.  Here fragment f of a tile is produced by ONE wave (f % 8): eight coalesced global_load_dword
// straight into the MFMA operand layout (lane = column f*32 + lane%32, rows 8*(lane/32) .. +7 -- 128 contiguous bytes per row
// and half wave), one split, three ds_write_b128 (bf16 planes, lane-contiguous: conflict free); the consumers read three
// ds_read_b128 per fragment.  Per workgroup and tile: 15 splits instead of 48 (TM = 7, KT = 8).  Two LDS buffers, one barrier per
// tile; the loads of tile t + 2 are issued before the barrier of tile t and consumed (split) during the MFMAs of tile t + 1.
// Same operands, same products, same accumulation order per output element as wgrad_x3_k: bit-identical partial tiles.
// (where a tile's time goes, per wave and phase: profiles/r4_wgrad_phases.txt)

template <int NG>
__global__ __launch_bounds__(WX_THREADS, 1) void wgrad_x3v_k(WgradArgs a) {
  using X = WgradX3<NG>;
  constexpr int KP = X::KP, KT = X::KT, ASLOTS = X::ASLOTS, FPW = X::FPW;
  constexpr int NFRAG = ASLOTS + KT;
  extern __shared__ __align__(16) float smem[];
  const int tn0 = (int)(((int64_t)blockIdx.y * a.TN) / gridDim.y);
  const int tnb = (int)(((int64_t)(blockIdx.y + 1) * a.TN) / gridDim.y) - tn0;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wg = wave / KP, wp = wave % KP;
  const int m0 = wg * 4;
  const int an = a.TM - m0 < 4 ? (a.TM - m0 > 0 ? a.TM - m0 : 0) : 4;      // row tiles of this wave
  const int kn = tnb - 2 * wp < 2 ? (tnb - 2 * wp > 0 ? tnb - 2 * wp : 0) : 2;   // column tiles of this wave
  const int K = a.K1 + a.K2;

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int64_t r_begin = (int64_t)blockIdx.x * a.rows_per_block;
  int64_t r_end = r_begin + a.rows_per_block;
  if (r_end > a.rows) r_end = a.rows;
  int64_t ws_off = 0;
  if (a.ngrp > 0) {                                       // one row range per blockIdx.z (constant indices: no scratch copy of the arguments)
    const int z = blockIdx.z;
#define MRG_PICKZ(F) (z == 0 ? a.F[0] : (z == 1 ? a.F[1] : a.F[2]))
    if ((int)blockIdx.x >= MRG_PICKZ(g_G)) return;          // workgroup-uniform, before any barrier
    const int64_t rpb = MRG_PICKZ(g_rpb), hi = MRG_PICKZ(g_hi);
    r_begin = MRG_PICKZ(g_lo) + (int64_t)blockIdx.x * rpb;
    r_end = r_begin + rpb < hi ? r_begin + rpb : hi;
    ws_off = MRG_PICKZ(g_ws_off);
#undef MRG_PICKZ
  }

  // the fragments this wave produces: per lane one column, eight rows; constants (the bias column of ones, padding, fragments
  // that do not exist) come from a 4-float device array with row stride 0: the loads are the same straight-line code for every
  // wave and tile (a conditional load would make the compiler wait for it before the loop's back edge)
  const float* src[FPW]; int64_t ld[FPW]; bool live[FPW];
#pragma unroll
  for (int i = 0; i < FPW; ++i) {
    const int f = wave + 8 * i;
    live[i] = f < NFRAG && (f < ASLOTS ? f < a.TM : f - ASLOTS < tnb);
    const float* base = mrg_zeros16; int64_t l = 0;
    if (live[i]) {
      if (f < ASLOTS) {
        const int cg = f * 32 + li;
        if (cg < a.Nout) { base = a.gY + (r_begin + 8 * lh) * a.ldg + cg; l = a.ldg; }
      } else {
        const int cg = (tn0 + f - ASLOTS) * 32 + li;
        if (cg < K) {
          const XSel sx = wgrad_sel_x(a, cg);
          base = sx.base + (r_begin + 8 * lh) * sx.ld + sx.kk; l = sx.ld;
        } else if (cg == K) {
          base = mrg_ones16;
        }
      }
    }
    src[i] = base; ld[i] = l;
  }
  constexpr unsigned BUF_BYTES = X::BUF_BYTES;

  // Full 16-row tiles run through the pipelined loop with plain loads; a ragged last tile (nv < 16 rows) is one extra, unpipelined
  // trip: its k positions >= nv are loaded from the rows 16 ABOVE their own (inside the tensor: the host guarantees r_end >= 16) and
  // zeroed at the split -- in-bounds loads without masks, and exactly the operand wgrad_x3_k builds (valid rows first, zeros after):
  // bit-identical with it for any row count.
  const int64_t nfull = (r_end - r_begin) / WBR;
  const int nv_tail = (int)((r_end - r_begin) - nfull * WBR);
  const int kbase = 8 * lh;
  float raw[FPW][8];
  auto fetch = [&](int64_t t) {                            // a FULL tile (t clamped by the caller)
    const int64_t toff = t * WBR;
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
      const float* p = src[i] + toff * ld[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[i][j] = p[j * ld[i]];
    }
  };
  auto produce = [&](int buf, auto tail_c) {
    constexpr bool TAIL = decltype(tail_c)::value;
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
      if (live[i]) {                                        // wave-uniform
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (!TAIL || kbase + j < nv_tail) ? raw[i][j] : 0.f;
        u32x4 H, M, L;
        split8(x, H, M, L);
        const int f = wave + 8 * i;
        u32x4* dst = reinterpret_cast<u32x4*>(reinterpret_cast<char*>(smem) + buf * BUF_BYTES + f * X::FRAG_BYTES) + lane;
        dst[0] = H; dst[64] = M; dst[128] = L;
      }
    }
  };
  auto rdfrag = [&](int buf, int f, bf16x8& H, bf16x8& M, bf16x8& L) {
    const u32x4* p = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(smem) + buf * BUF_BYTES + f * X::FRAG_BYTES) + lane;
    H = __builtin_bit_cast(bf16x8, p[0]); M = __builtin_bit_cast(bf16x8, p[64]); L = __builtin_bit_cast(bf16x8, p[128]);
  };
  auto consume = [&](int cur) {
    if (an > 0 && kn > 0) {
      bf16x8 Bh0, Bm0, Bl0, Bh1, Bm1, Bl1;
      rdfrag(cur, ASLOTS + 2 * wp, Bh0, Bm0, Bl0);
      if (kn > 1) rdfrag(cur, ASLOTS + 2 * wp + 1, Bh1, Bm1, Bl1);
      else { Bh1 = Bh0; Bm1 = Bm0; Bl1 = Bl0; }
      bf16x8 An[3];                                        // the NEXT row tile's planes: read while this one's MFMAs run
      rdfrag(cur, m0, An[0], An[1], An[2]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < an) {
          const bf16x8 Ah = An[0], Am = An[1], Al = An[2];
          if (i + 1 < an) rdfrag(cur, m0 + i + 1, An[0], An[1], An[2]);
          if (kn > 1) {                                    // two accumulators interleaved: no back-to-back dependent MFMAs
            x3_chain2(acc[i][0], acc[i][1], Ah, Am, Al, Bh0, Bm0, Bl0, Ah, Am, Al, Bh1, Bm1, Bl1);
          } else {
            x3_chain(acc[i][0], Ah, Am, Al, Bh0, Bm0, Bl0);
          }
        }
      }
    }
  };

  if (nfull > 0) {
    fetch(0);
    produce(0, std::false_type{});
    fetch(nfull > 1 ? 1 : 0);
    __syncthreads();
    int cur = 0;
    for (int64_t t = 0; t < nfull; ++t) {
      consume(cur);
      // tile t + 1 (its loads were issued one tile ago) is split under this tile's MFMAs; then the loads of tile t + 2 (clamped:
      // past the end the last full tile is simply loaded again and never used)
      if (t + 1 < nfull) produce(cur ^ 1, std::false_type{});
      fetch(t + 2 < nfull ? t + 2 : nfull - 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  if (nv_tail > 0) {                                       // every wave is past the loop's last barrier: both buffers are free
    const int64_t toff = nfull * WBR;
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
      const float* p = src[i] + toff * ld[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[i][j] = p[(int64_t)(kbase + j >= nv_tail ? j - WBR : j) * ld[i]];
    }
    produce(0, std::true_type{});
    __syncthreads();
    consume(0);
  }
  const int ldw = a.TN * 32;
  float* out = a.ws + ws_off + (int64_t)blockIdx.x * (a.TM * 32) * ldw;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (i < an && j < kn) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (m0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          out[(int64_t)row * ldw + (tn0 + 2 * wp + j) * 32 + li] = acc[i][j][r];
        }
      }
}

// The split-core kernel of this launch: G row blocks on grid.x, balanced column blocks of KT tiles on grid.y, one row range per
// grid.z.  NG follows the row tiles; wgrad_x3v_k needs 16 rows that END at each range's end (its ragged last tile reads them).
static int launch_wgrad_x3(const WgradArgs& a, int G, int nrange, hipStream_t st) {
  bool v1 = gemm_switches().wgrad_variant == 1 && a.rows >= WBR;
  for (int i = 0; i < a.ngrp; ++i) v1 = v1 && !(a.g_hi[i] > a.g_lo[i] && a.g_hi[i] < WBR);
  auto go = [&](auto ng_c) {
    using X = WgradX3<decltype(ng_c)::value>;
    const dim3 grid(G, (a.TN + X::KT - 1) / X::KT, nrange);
    if (v1) return launch_kernel(wgrad_x3v_k<decltype(ng_c)::value>, grid, dim3(WX_THREADS), X::LDS_SPLIT, st, a);
    return launch_kernel(wgrad_x3_k<decltype(ng_c)::value>, grid, dim3(WX_THREADS), X::LDS_RAW, st, a);
  };
  return a.TM <= 4 ? go(std::integral_constant<int, 1>{}) : go(std::integral_constant<int, 2>{});
}

// gW[n][c] = sum_g ws[g][n][c] (c < K);  gbias[n] = sum_g ws[g][n][K]   -- fixed order:
// thread row ty sums the partial tiles g = ty, ty+16, ..., the 16 row sums are added in order.
// Up to three row ranges in one launch (blockIdx.z).
struct WgradReduce3 { const float* ws[3]; float* gW[3]; float* gbias[3]; int G[3]; };
__global__ void wgrad_reduce3_k(WgradReduce3 p, int K, int Nout, int ldg, int ldx) {
  __shared__ float part[16][64];
  const int z = blockIdx.z;
  const float* __restrict__ ws = z == 0 ? p.ws[0] : (z == 1 ? p.ws[1] : p.ws[2]);
  float* __restrict__ gW = z == 0 ? p.gW[0] : (z == 1 ? p.gW[1] : p.gW[2]);
  float* __restrict__ gbias = z == 0 ? p.gbias[0] : (z == 1 ? p.gbias[1] : p.gbias[2]);
  const int G = z == 0 ? p.G[0] : (z == 1 ? p.G[1] : p.G[2]);
  if (!gW) return;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  const int n = blockIdx.y;
  float acc = 0.f;
  if (c <= K)
    for (int g = ty; g < G; g += 16) acc += ws[((int64_t)g * ldg + n) * ldx + c];
  part[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && c <= K) {
    float tot = part[0][tx];
#pragma unroll
    for (int i = 1; i < 16; ++i) tot += part[i][tx];
    if (c < K) gW[(int64_t)n * K + c] = tot;
    else if (gbias) gbias[n] = tot;
  }
}

// the first nrange (1 or 3) ranges of red; TM, TN: the row / column tiles of the partial tiles
static int launch_wgrad_reduce(const WgradReduce3& red, int nrange, int K, int Nout, int TM, int TN, hipStream_t st) {
  hipLaunchKernelGGL(wgrad_reduce3_k, dim3((K + 1 + 63) / 64, Nout, nrange), dim3(1024), 0, st, red, K, Nout, TM * 32, TN * 32);
  MRG_LAUNCH_CHECK();
  return MRG_OK;
}

// Share-independent: a share above 1 only lowers gmax (256 / (ny * share) < 256 / ny, 16 < 32), so G,
// and with it the number of partial tiles, is at most the share-1 plan's -- that size bounds every share.
static int64_t wgrad_workspace_bytes(int64_t rows, int K, int Nout) {
  WgradPlan p = wgrad_plan(rows, K, Nout);
  return (int64_t)p.G * p.TM * 32 * p.TN * 32 * sizeof(float);
}

// The vector kernels (wgrad_dma_k, and with Nout <= 224 the split core) take these operands: 16-byte rows at 16-byte addresses.
// With NULL pointers: the answer for the shape alone.
static bool wgrad_vec_ok(const float* gY, int ldg, const float* X1, const float* X2, int K1, int K2, int Nout) {
  const bool shape = Nout >= 4 && Nout % 4 == 0 && ldg % 4 == 0 && K1 >= 4 && K1 % 4 == 0 && K2 >= 0 && K2 % 4 == 0;
  return shape && aligned16(gY) && aligned16(X1) && (!X2 || K2 == 0 || aligned16(X2));
}

// gW[Nout][K1+K2] = gY^T [X1 | X2], gbias = column sums of gY; gY: Nout <= 224 columns of rows ldg apart when the operands are vectors
static int launch_wgrad_one(const float* gY, int ldg, const float* X1, const float* X2, int K1, int K2, float* gW, float* gbias, void* ws,
                            int64_t rows, int Nout, int share, hipStream_t st) {
  const int K = K1 + K2;
  if (rows == 0) {
    hipError_t e = hipMemsetAsync(gW, 0, sizeof(float) * (size_t)Nout * K, st);
    if (e == hipSuccess && gbias) e = hipMemsetAsync(gbias, 0, sizeof(float) * (size_t)Nout, st);
    return (int)e;
  }
  const bool vec = Nout <= 224 && wgrad_vec_ok(gY, ldg, X1, X2, K1, K2, Nout);
  WgradPlan p = wgrad_plan(rows, K, Nout, vec, share);
  if (!p.ok) return MRG_E_SHAPE;
  WgradArgs a{};
  a.gY = gY; a.Nout = Nout; a.ldg = ldg; a.X1 = X1; a.X2 = X2; a.K1 = K1; a.K2 = K2; a.ws = (float*)ws;
  a.rows = rows; a.rows_per_block = p.rows_per_block; a.TM = p.TM; a.TN = p.TN; a.TNB = p.TNB;
  if (!X2 || K2 == 0) { a.X2 = X1; a.K2 = 0; }
  int rc = MRG_E_SHAPE;
  if (vec && gemm_switches().mode != 1) {                     // split-bf16 core
    rc = launch_wgrad_x3(a, p.G, 1, st);
  } else {
    const dim3 grid(p.G, (p.TN + p.TNB - 1) / p.TNB);      // y-blocks own ~TN/grid.y column tiles each (<= TNB)
    const int npf = wgrad_npf_class(p.npf);
    void (*kernel)(WgradArgs) = nullptr;                       // stays NULL for a (kernel, tpw, npf class) without an instance
#define MRG_WGRAD_DMA(T, F) if (vec && p.tpw == T && npf == F) kernel = wgrad_dma_k<T, F>;
#define MRG_WGRAD_PLAIN(T, F) if (!vec && p.tpw == T && npf == F) kernel = wgrad_k<T, F>;
    MRG_WGRAD_DMA_INSTANCES(MRG_WGRAD_DMA) MRG_WGRAD_PLAIN_INSTANCES(MRG_WGRAD_PLAIN)
#undef MRG_WGRAD_DMA
#undef MRG_WGRAD_PLAIN
    if (kernel) rc = launch_kernel(kernel, grid, dim3(MRG_BLOCK), p.lds, st, a);
  }
  if (rc != MRG_OK) return rc;
  const WgradReduce3 red{{(const float*)ws}, {gW}, {gbias}, {p.G}};
  return launch_wgrad_reduce(red, 1, K, Nout, p.TM, p.TN, st);
}

// The three row ranges [0, b0) [b0, b1) [b1, M) of mrg_linear_bwd_weight3: per range the plan when `share` ranges share the chip
// and the byte offset of its partial tiles in the workspace (sized for any share); total: the workspace's bytes.
struct Wgrad3Layout { int64_t lo[3], hi[3], off[3], total; WgradPlan plan[3]; };
static Wgrad3Layout wgrad3_layout(int64_t b0, int64_t b1, int64_t M, int K, int Nout, int share) {
  Wgrad3Layout L{{0, b0, b1}, {b0, b1, M}};
  for (int i = 0; i < 3; ++i) {
    L.plan[i] = wgrad_plan(L.hi[i] - L.lo[i], K, Nout, true, share);
    L.off[i] = L.total;
    L.total += (wgrad_workspace_bytes(L.hi[i] - L.lo[i], K, Nout) + 255) / 256 * 256;
  }
  return L;
}

}  // namespace mrg

using namespace mrg;

extern "C" int mrg_wgrad_set_variant(int variant) {
  if (variant != 0 && variant != 1) return MRG_E_ENUM;
  gemm_switches().wgrad_variant = variant;
  return MRG_OK;
}

// gW[s][Nout][K1+K2] = gY[lo_s:hi_s]^T [X1 | X2][lo_s:hi_s], gbias[s] = column sums, for the three row ranges in one launch
extern "C" int64_t mrg_linear_bwd_weight3_workspace_bytes(int64_t b0, int64_t b1, int64_t M, int K1, int K2, int Nout) {
  if (M < 0 || b0 < 0 || b1 < b0 || M < b1 || Nout > 224 || !wgrad_vec_ok(nullptr, Nout, nullptr, nullptr, K1, K2, Nout) || gemm_switches().mode == 1) return 0;
  return wgrad3_layout(b0, b1, M, K1 + K2, Nout, 1).total;
}

extern "C" int mrg_linear_bwd_weight3(const float* gY, const float* X1, const float* X2, float* const* gW_host, float* const* gb_host, void* ws,
                                      int64_t b0, int64_t b1, int64_t M, int K1, int K2, int Nout, void* stream) {
  if (M < 0 || b0 < 0 || b1 < b0 || M < b1 || Nout > 224 || !wgrad_vec_ok(nullptr, Nout, nullptr, nullptr, K1, K2, Nout)) return MRG_E_SHAPE;
  if (!gW_host) return MRG_E_NULLPTR;
  if (M > 0 && (!gY || !X1 || (K2 > 0 && !X2))) return MRG_E_NULLPTR;
  if (!ws) return MRG_E_WORKSPACE;
  if (!wgrad_vec_ok(gY, Nout, X1, X2, K1, K2, Nout)) return MRG_E_SHAPE;
  const int K = K1 + K2;
  const int64_t rows[3] = {b0, b1 - b0, M - b1};
  int nlive = 0;
  for (int i = 0; i < 3; ++i) nlive += (gW_host[i] != nullptr && rows[i] > 0) ? 1 : 0;
  const Wgrad3Layout L = wgrad3_layout(b0, b1, M, K, Nout, nlive < 1 ? 1 : nlive);
  if (!L.plan[0].ok) return MRG_E_SHAPE;
  WgradArgs a{};
  a.gY = gY; a.Nout = Nout; a.ldg = Nout; a.X1 = X1; a.X2 = K2 > 0 ? X2 : X1; a.K1 = K1; a.K2 = K2; a.ws = (float*)ws; a.rows = M;
  a.TM = L.plan[0].TM; a.TN = L.plan[0].TN; a.TNB = L.plan[0].TNB; a.ngrp = 3;       // the tiles depend on the shape alone
  WgradReduce3 red{};
  int maxG = 0;                                      // row blocks of the longest live range: grid.x
  for (int i = 0; i < 3; ++i) {
    const WgradPlan& p = L.plan[i];
    const bool live = gW_host[i] != nullptr;
    a.g_lo[i] = L.lo[i]; a.g_hi[i] = L.hi[i]; a.g_rpb[i] = p.rows_per_block; a.g_G[i] = live ? p.G : 0; a.g_ws_off[i] = L.off[i] / (int64_t)sizeof(float);
    red.ws[i] = (const float*)((const char*)ws + L.off[i]); red.gW[i] = gW_host[i]; red.gbias[i] = gb_host ? gb_host[i] : nullptr; red.G[i] = p.G;
    if (live && p.G > maxG) maxG = p.G;
  }
  if (maxG == 0) return MRG_OK;
  const int rc = launch_wgrad_x3(a, maxG, 3, (hipStream_t)stream);
  return rc != MRG_OK ? rc : launch_wgrad_reduce(red, 3, K, Nout, a.TM, a.TN, (hipStream_t)stream);
}

extern "C" int64_t mrg_linear_bwd_weight_workspace_bytes(int64_t rows, int K, int Nout) {
  if (rows < 0 || K <= 0 || Nout <= 0) return 0;
  return wgrad_workspace_bytes(rows, K, Nout);
}

// gW[Nout][K1+K2] = gY^T [X1 | X2] (X2 NULL / K2 = 0: single source), gbias[Nout] = column sums of gY (NULL ok)
extern "C" int mrg_linear_bwd_weight_share(const float* gY, const float* X1, const float* X2, float* gW, float* gbias, void* ws,
                                           int64_t rows, int K1, int K2, int Nout, int share, void* stream) {
  if (rows < 0 || K1 <= 0 || K2 < 0 || Nout <= 0) return MRG_E_SHAPE;
  if (share < 1 || share > 3) return MRG_E_ENUM;
  if (!gW) return MRG_E_NULLPTR;
  if (rows > 0 && (!gY || !X1 || (K2 > 0 && !X2))) return MRG_E_NULLPTR;
  if (rows > 0 && !ws) return MRG_E_WORKSPACE;
  if (K2 == 0) X2 = nullptr;
  // more than 7 row tiles of gW (Nout > 224, e.g. D = 256): balanced column blocks of gY, each a launch of the
  // <= 7-tile kernels (X is re-read per block); same workspace, stream ordered.  Everything else: one block of Nout columns.
  int cw = Nout;
  if (Nout > 224 && rows > 0 && wgrad_vec_ok(gY, Nout, X1, X2, K1, K2, Nout)) {
    const int nblk = (Nout + 223) / 224;
    cw = (((Nout + nblk - 1) / nblk) + 31) / 32 * 32;
  }
  for (int n0 = 0; n0 < Nout; n0 += cw) {
    const int nc = Nout - n0 < cw ? Nout - n0 : cw;
    int rc = launch_wgrad_one(gY + n0, Nout, X1, X2, K1, K2, gW + (int64_t)n0 * (K1 + K2), gbias ? gbias + n0 : nullptr, ws, rows, nc, share, (hipStream_t)stream);
    if (rc != MRG_OK) return rc;
  }
  return MRG_OK;
}

extern "C" int mrg_linear_bwd_weight(const float* gY, const float* X1, const float* X2, float* gW, float* gbias, void* ws,
                                     int64_t rows, int K1, int K2, int Nout, void* stream) {
  return mrg_linear_bwd_weight_share(gY, X1, X2, gW, gbias, ws, rows, K1, K2, Nout, 1, stream);
}
