// Software-pipelined tall-skinny GEMM core on the exact-f32 matrix pipe (v_mfma_f32_32x32x2_f32).
//
//   C[rows, N] = epilogue( [A1 | A2][rows, K1+K2] * B[N, K1+K2]^T )
//
// rows ~ 5e5, N and K ~ 2e2..4e2: 2*rows*K*N flop over 4*rows*(K+N) bytes is ~100 flop/B, far above
// the f32-MFMA ridge (157 TF/s / 8 TB/s ~ 20 flop/B), so the matrix pipe is the roofline.
//
// Geometry (wave = 64 lanes): a 256-thread workgroup owns 128 rows x NT*32 columns; wave w owns
// rows [32w, 32w+32) and all NT column tiles of 32x32 (NT*16 accumulator registers), so A is read
// from HBM exactly once.  Registers are held to <= 256 per lane so that TWO workgroups share a CU:
// one workgroup's prologue / epilogue overlaps the other's MFMA phase.
// K is walked in tiles of 16: while the 8*NT MFMAs (64 cycles each) of tile t run, the global
// loads of tile t+1 are already in flight into registers (issued branch-free from clamped
// addresses; masking happens when they are written to the other LDS buffer after the MFMAs),
// one barrier per tile.  LDS tiles are k-contiguous with a 4-float pad (row stride 20 floats):
// the ds_read_b128 fragment reads are bank-conflict free; one ds_read_b128 (4 consecutive k)
// feeds 4 MFMAs; the fragments of step t+1 are read while the MFMAs of step t issue.
// Measured (MI355X, rows 544k, K = N = 200): 66-68 TF/s (rocBLAS sgemm via torch: 38.6 TF/s);
// with 13 barriers per workgroup and lock-stepped partners the matrix pipe is ~55 % busy.
// "Dual source": the reduction dimension may be the concatenation of two row-major tensors
// (the reference's torch.cat([s, s_in], dim=1) is never materialised).
#pragma once
#include "common.hpp"

namespace mrg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;             // LDS-DMA destination / LDS byte address of a __shared__ object
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;       // LDS-DMA source

constexpr int GBM_MAX = 256;      // rows per workgroup = 128 * MT (MT row tiles of 32 per wave)

enum { EPI_BIAS_ACT = 0, EPI_GATE = 1, EPI_SCALE = 2, EPI_ACCUM = 3, EPI_SEGMAX = 4, EPI_SEGSUM = 5 };
// EPI_GATE / EPI_SCALE that also leave the column sums of the values they form (gemm_colsum(GemmArgs); gemm_epilogue's SUMS): kernel
// instances of their own, so that the plain ones stay what they are.  Split core, rowgemm_x3s_k<7, ...> and rowgemm_x3q_k only.
enum { EPI_GATE_SUMS = 6, EPI_SCALE_SUMS = 7 };
constexpr bool epi_sums(int epi) { return epi == EPI_GATE_SUMS || epi == EPI_SCALE_SUMS; }
constexpr int epi_base(int epi) { return epi == EPI_GATE_SUMS ? EPI_GATE : (epi == EPI_SCALE_SUMS ? EPI_SCALE : epi); }
// The counting epilogues of mrg_distmult_rank (rank.hip; gemm_epilogue_rank / gemm_epilogue_rank_diag below): rows are queries, columns
// are entities, nothing is stored.  EPI_RANK_DIAG multiplies row block x by COLUMN block x (the rows' gathered targets) and keeps the
// diagonal.  Kernel instances of their own, like the column-sum kinds.
enum { EPI_RANK = 8, EPI_RANK_DIAG = 9 };
constexpr bool epi_diag(int epi) { return epi == EPI_RANK_DIAG; }
// The loss epilogues of mrg_distmult_bce_fwd / mrg_distmult_bce_dlogit (bce.hip; gemm_epilogue_bce / gemm_epilogue_bce_grad below): rows
// are queries, columns are entities, the label of an element is looked up in the query's object list.  EPI_BCE stores nothing per
// element (one float64 partial per workgroup), EPI_BCE_GRAD stores the gradient with respect to the logits.  Kernel instances of their own.
enum { EPI_BCE = 10, EPI_BCE_GRAD = 11 };
// EPI_ACCUM with a second addend: C = (acc + Cin) + Cin2 -- the input-gradient GEMM of a reader that joins a running gradient fan-in
// sum (functional/fanin.py): its own term first, then the sum so far.  Cin2 may be C itself.  Kernel instances of their own.
enum { EPI_ACCUM2 = 12 };
constexpr bool epi_accum(int epi) { return epi == EPI_ACCUM || epi == EPI_ACCUM2; }
// The selecting epilogue of mrg_rows_topk (topk.hip defines gemm_epilogue_topk and what it reads): rows are queries, columns are
// entities, every (row, workgroup) leaves its k best unfiltered (value, id) pairs.  Kernel instances of their own.
enum { EPI_TOPK = 13 };
// The sweep epilogues under a per-entity score bias (CompGCN_ConvE: logit = acc + bias[column], GemmArgs::bias = the bias of the
// launch's column 0): gemm_add_col_bias puts the bias into the accumulators, one float32 add per element, and the unbiased kind's
// epilogue (epi_unbiased) runs on them -- nothing else changes.  Kernel instances of their own, so that the unbiased ones stay what
// they are.  The rank's target score needs no instance: rank.hip adds bias[target] to the diagonal's result (rank_bias_tscore_k).
enum { EPI_BCE_BIAS = 14, EPI_BCE_GRAD_BIAS = 15, EPI_RANK_BIAS = 16, EPI_TOPK_BIAS = 17 };
constexpr bool epi_col_bias(int epi) { return epi >= EPI_BCE_BIAS && epi <= EPI_TOPK_BIAS; }
constexpr int epi_unbiased(int epi) {
  return epi == EPI_BCE_BIAS ? EPI_BCE : (epi == EPI_BCE_GRAD_BIAS ? EPI_BCE_GRAD : (epi == EPI_RANK_BIAS ? EPI_RANK : (epi == EPI_TOPK_BIAS ? EPI_TOPK : epi)));
}
struct GemmArgs;
template <int NT>
__device__ __forceinline__ void gemm_epilogue_topk(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh);

// Up to three row ranges of ONE launch of the split-core row GEMM that share every tensor but differ in the weight matrix
// (the in / out / self direction segments of a dense filter: one launch instead of three).  Workgroup blocks
// [tile0[s], tile0[s+1]) own range s = rows [lo[s], hi[s]) (absolute row numbers of the shared tensors).
struct GemmGroups {
  int n;                              // 0: plain GEMM over rows [0, rows)
  int tile0[4];
  int64_t lo[3], hi[3];
  int64_t bp_stride;                  // range s reads the pre-split weight at Bp + s * bp_stride (launch_bsplit3)
  const float* bias[3];
  float scale[3];
  int use_rowscale[3];
};
// Host: blocks of range s follow those of range s - 1.  Fills tile0[] for gbm rows per workgroup; returns the number of workgroups.
inline int gemm_group_tiles(GemmGroups& g, int gbm) {
  g.tile0[0] = 0;
  for (int i = 0; i < 3; ++i) {
    const int64_t r = i < g.n && g.hi[i] > g.lo[i] ? g.hi[i] - g.lo[i] : 0;
    g.tile0[i + 1] = g.tile0[i] + (int)((r + gbm - 1) / gbm);
  }
  return g.tile0[3];
}

struct GemmArgs {
  const float* A1; const float* A2;   // [rows][K1], [rows][K2] row-major; A2 may be NULL (K2 = 0)
  int K1, K2;
  const float* B; int ldb;            // [N][ldb] row-major, columns [0, K1+K2) are used
  const float* bias;                  // [N] or NULL
  float* C; int ldc; int N;           // output [rows][ldc], N valid columns
  int64_t rows;
  int act;                            // EPI_BIAS_ACT: MRG_ACT_*
  const float* S; int ld_s;           // EPI_GATE: C = sigmoid(acc + bias) * S[row][col] * c_row
  const float* rowscale; float scale; // c_row = scale * (rowscale ? rowscale[row] : 1)     (EPI_GATE, EPI_SCALE)
  float* aux;                         // EPI_GATE: optional store of sigmoid(acc + bias), [rows][N]
  const float* Cin; int ld_cin;       // EPI_ACCUM: C = acc + Cin
  // split core only (gemm_x3.hpp): output row r reads A row row_index[r] (NULL: r itself)
  const int32_t* row_index;
  // EPI_SEGMAX (no C): seg_out[row_seg[row_index[r]] * N + col] = max over rows r of pack(ReLU(acc + bias), r), see gemm_epilogue_segmax
  const int32_t* row_seg;
  unsigned long long* seg_out;
  // EPI_SEGSUM (no C): run sums of ReLU(acc + bias) at seg_part[head position * N + col], ReLU bit mask at relu_bits, see gemm_epilogue_segsum
  // (EPI_GATE_SUMS / EPI_SCALE_SUMS have no run sums: their colsum pointer travels in this slot, gemm_colsum below)
  float* seg_part;
  unsigned* relu_bits; int bits_ld;
  int pad0;                           // never read; keeps wave_lds_floats and grp where the kernels' argument loads expect them
  int wave_lds_floats;                // split core, one-wave kernel: floats of a wave's private LDS region, the A ring; set by the launcher
  GemmGroups grp;                     // split core, one-wave kernel only
};

// EPI_GATE_SUMS / EPI_SCALE_SUMS: colsum[workgroup along x][2][N] float64, the workgroup's column sums and column sums of squares of
// its output values.  The pointer shares the slot of seg_part (EPI_SEGSUM only), so the argument block -- and with it the code of
// every other kernel instance -- stays what it was.
// EPI_ACCUM2: the second addend [rows][ld] travels in the slots of the gate's multiplicand (S, ld_s), which EPI_ACCUM does not use.
inline void gemm_set_cin2(GemmArgs& a, const float* cin2, int ld) { a.S = cin2; a.ld_s = ld; }
inline void gemm_set_colsum(GemmArgs& a, double* colsum) { a.seg_part = reinterpret_cast<float*>(colsum); }
__host__ __device__ __forceinline__ double* gemm_colsum(const GemmArgs& a) { return reinterpret_cast<double*>(a.seg_part); }

// The 4 floats at column k of the concatenated row [r1 (K1 floats) | r2 (K2 floats)] (DUAL) or of r1 alone (K floats), clamped
// into the row: beyond the end a chunk re-reads the row's last 4 floats -- any finite values, the weight's rows there are zero.
// Used by every kernel that fetches activations in 16-byte chunks (rowgemm_dma_k and the split-core kernels).
template <bool DUAL>
__device__ __forceinline__ const float* gemm_a_ptr(const float* r1, const float* r2, int K1, int K2, int K, int k) {
  if (DUAL) {
    const bool first = k < K1;
    const int kk = first ? k : k - K1, ld = first ? K1 : K2;
    return (first ? r1 : r2) + (kk + 4 <= ld ? kk : ld - 4);
  }
  return r1 + (k + 4 <= K ? k : K - 4);
}

// EPI_RANK / EPI_RANK_DIAG: what the counting epilogues read and write.  The pointers travel in slots of GemmArgs that these kinds do
// not otherwise use (S, aux, row_seg, Cin, rowscale, relu_bits), so the argument block -- and with it the code of every other
// kernel instance -- stays what it was.  row_index stays NULL.
struct RankEpi {
  const float* tscore;        // EPI_RANK: [rows] the target's score of each query, formed by EPI_RANK_DIAG on the same tile routine
  float* tscore_out;          // EPI_RANK_DIAG: where it goes
  const int32_t* qinfo;       // [rows][4]: target entity, begin and end of the query's filter list in members / gone_at, `when`
  const int32_t* members;     // filter lists: entity ids, ascending inside a list
  const int32_t* gone_at;     // per member: filtered iff gone_at > when
  unsigned* counts;           // [rows], zeroed: candidates that beat the target
};
inline void gemm_set_rank(GemmArgs& a, const RankEpi& r) {
  a.S = r.tscore; a.aux = r.tscore_out; a.row_seg = r.qinfo;
  a.Cin = reinterpret_cast<const float*>(r.members); a.rowscale = reinterpret_cast<const float*>(r.gone_at); a.relu_bits = r.counts;
}
__device__ __forceinline__ RankEpi gemm_rank(const GemmArgs& a) {
  return RankEpi{a.S, a.aux, a.row_seg, reinterpret_cast<const int32_t*>(a.Cin), reinterpret_cast<const int32_t*>(a.rowscale), a.relu_bits};
}

// acc[n][r] += bias[col0 + n * 32 + li]: the logit of a "dot" sweep with a per-entity bias (epi_col_bias kinds), formed before the
// epilogue looks at the accumulators.  A column beyond N is not read: its lane re-reads the last valid column and adds 0.
template <int NT>
__device__ __forceinline__ void gemm_add_col_bias(const GemmArgs& a, f32x16 (&acc)[NT], int col0, int li) {
  float bv[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = col0 + n * 32 + li;
    const float b = a.bias[col < a.N ? col : a.N - 1];
    bv[n] = col < a.N ? b : 0.f;
  }
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] += bv[n];
}

// ---- DistMult ranking: "how many columns beat this row's target" as the GEMM's epilogue (reference utils/utils_rgcn.py:212-380) --
// Candidate `col` of query `row` counts iff it exists, is not the target, is not filtered, and beats the target under the rule of
// mrg_rank_filtered: score greater, or equal with the lower entity id.  The comparison and the filter decision are taken on the SAME
// accumulator value, once per (query, candidate): a ballot per accumulator register turns the 32 x 32 comparisons of a tile into one
// 32-bit column mask per row, lane l < 32 collects the masks of row l, walks the slice of that row's ascending filter list that falls
// into the workgroup's column range (binary search for its start), clears the bits of the members still in force (gone_at > when),
// and publishes ONE integer atomicAdd per (row, workgroup).  Integer atomics only: the counts do not depend on their order.
// The target's score comes from gemm_epilogue_rank_diag: the same k-order and term order on the same operand values, so a
// duplicate of the target's entity row scores bit-identically and ties.
template <int NT>
__device__ __forceinline__ void gemm_epilogue_rank(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh) {
  if (rowbase >= a.rows) return;
  const RankEpi k = gemm_rank(a);
  float ts[16];
  int tg[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = rowbase + (r & 3) + 8 * (r >> 2) + 4 * lh;
    const int64_t rc = row < a.rows ? row : a.rows - 1;
    ts[r] = k.tscore[rc];
    tg[r] = k.qinfo[rc * 4];
  }
  const int lane = lh * 32 + li;
  unsigned word[NT];                                         // lane l < 32: the column masks of row rowbase + l
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = col0 + n * 32 + li;
    const bool cok = col < a.N;
    unsigned w = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float x = acc[n][r];
      const bool hit = cok && col != tg[r] && (x > ts[r] || (x == ts[r] && col < tg[r]));
      const unsigned long long ball = __ballot(hit);         // lanes 0-31: this register's row of half 0, lanes 32-63: of half 1
      const int rl = (r & 3) + 8 * (r >> 2);
      w = lane == rl ? (unsigned)ball : (lane == rl + 4 ? (unsigned)(ball >> 32) : w);
    }
    word[n] = w;
  }
  const int64_t row = rowbase + lane;
  if (lane >= 32 || row >= a.rows) return;
  const int4 qi = *reinterpret_cast<const int4*>(k.qinfo + row * 4);
  const int hi = qi.z, when = qi.w;
  if (qi.y < hi) {
    const int cend = col0 + NT * 32;
    int b = qi.y, e = hi;
    while (b < e) {                                          // first member >= col0
      const int mid = b + ((e - b) >> 1);
      if (k.members[mid] < col0) b = mid + 1; else e = mid;
    }
    for (; b < hi; ++b) {
      const int m = k.members[b];
      if (m >= cend) break;
      if (k.gone_at[b] > when) {
        const int d = m - col0;
#pragma unroll
        for (int n = 0; n < NT; ++n) word[n] &= ~((d >> 5) == n ? 1u << (d & 31) : 0u);
      }
    }
  }
  unsigned cnt = 0;
#pragma unroll
  for (int n = 0; n < NT; ++n) cnt += __popc(word[n]);
  if (cnt) atomicAdd(k.counts + row, cnt);
}

// EPI_RANK_DIAG: row block x against column block x, whose 128 columns are the gathered target rows of the block's 128 queries
// (NT = 4: wave w's rows meet their own targets in column tile w).  tscore_out[row] = the accumulator of (row, row's own column).
template <int NT>
__device__ __forceinline__ void gemm_epilogue_rank_diag(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int wave, int li, int lh) {
  static_assert(NT == 4, "the diagonal of a 128 x 128 block");
  if (rowbase >= a.rows) return;
  float* __restrict__ out = gemm_rank(a).tscore_out;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    if (n != wave) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (li == rl && rowbase + rl < a.rows) out[rowbase + rl] = acc[n][r];
    }
  }
}

// ---- DistMult 1-N loss: BCELoss(sigmoid(x), y) and its logit gradient as the GEMM's epilogue (reference models/operations_lp.py:115-127,
// train/mr_lp_train.py Network._loss; labels utils/data_set.py:21-33) ------------------------------------------------------------------
// EPI_BCE / EPI_BCE_GRAD: what the loss epilogues read and write.  Like RankEpi the values travel in slots of GemmArgs that these
// kinds do not otherwise use (row_seg, Cin, scale, act, bits_ld, seg_part, rowscale), so the argument block stays what it was.
// EPI_BCE_GRAD stores through C / ldc as every storing epilogue does.  row_index stays NULL.
struct BceEpi {
  const int32_t* qlist;       // [rows][2]: begin and end of the query's object list in objs (empty: every label is v_zero)
  const int32_t* objs;        // object lists: entity ids, ascending inside a list
  float v_zero, v_one;        // the two label values (label smoothing folded in by the caller)
  int c0;                     // entity id of the launch's column 0 (B points at that entity's row)
  double* partial;            // EPI_BCE: [gridDim.y][gridDim.x], the workgroup's sum of its elements' loss terms
  const float* gscale;        // EPI_BCE_GRAD: [1] on the device, upstream gradient / (B * N)
};
inline void gemm_set_bce(GemmArgs& a, const BceEpi& b) {
  a.row_seg = b.qlist; a.Cin = reinterpret_cast<const float*>(b.objs); a.scale = b.v_zero; a.act = __builtin_bit_cast(int, b.v_one);
  a.bits_ld = b.c0; a.seg_part = reinterpret_cast<float*>(b.partial); a.rowscale = b.gscale;
}
__device__ __forceinline__ BceEpi gemm_bce(const GemmArgs& a) {
  return BceEpi{a.row_seg, reinterpret_cast<const int32_t*>(a.Cin), a.scale, __builtin_bit_cast(float, a.act), a.bits_ld,
                reinterpret_cast<double*>(a.seg_part), a.rowscale};
}

// The labels of a wave's 32 rows x NT * 32 columns as bits: lane l < 32 walks the slice of row (rowbase + l)'s ascending object list
// that falls into the workgroup's column range (binary search for its start, as gemm_epilogue_rank does) and leaves one 32-bit column
// mask per tile; lanes 32-63 and rows beyond the launch leave zeros.
template <int NT>
__device__ __forceinline__ void gemm_bce_label_words(const BceEpi& k, int64_t rowbase, int64_t rows, int col0, int lane, unsigned (&word)[NT]) {
#pragma unroll
  for (int n = 0; n < NT; ++n) word[n] = 0u;
  const int64_t row = rowbase + lane;
  if (lane >= 32 || row >= rows) return;
  const int2 q = *reinterpret_cast<const int2*>(k.qlist + row * 2);
  if (q.x >= q.y) return;
  const int cbeg = k.c0 + col0, cend = cbeg + NT * 32;
  int b = q.x, e = q.y;
  while (b < e) {                                            // first member >= cbeg
    const int mid = b + ((e - b) >> 1);
    if (k.objs[mid] < cbeg) b = mid + 1; else e = mid;
  }
  for (; b < q.y; ++b) {
    const int m = k.objs[b];
    if (m >= cend) break;
    const int d = m - cbeg;
#pragma unroll
    for (int n = 0; n < NT; ++n) word[n] |= (d >> 5) == n ? 1u << (d & 31) : 0u;
  }
}
// the label of accumulator register r, tile word `w` (gemm_bce_label_words), of this lane: the mask lives in lane `row within the strip`
__device__ __forceinline__ float gemm_bce_label(unsigned w, int r, int li, int lh, float v_zero, float v_one) {
  const int rl = (r & 3) + 8 * (r >> 2);
  const unsigned w0 = (unsigned)__builtin_amdgcn_readlane((int)w, rl), w1 = (unsigned)__builtin_amdgcn_readlane((int)w, rl + 4);
  return (((lh ? w1 : w0) >> li) & 1u) ? v_one : v_zero;
}

// EPI_BCE: the sum over the wave's valid elements of  (y - 1) * max(log1p(-p), -100) - y * max(log p, -100),  p = sigmoid(x) in float32
// as EPI_BIAS_ACT forms it -- torch's binary_cross_entropy term for term, saturation included (p == 1: 100 (1 - y); p == 0: 100 y).
// A lane adds its NT * 16 terms in register order in float64, then the wave's lanes are added by a butterfly: a fixed order.  Every
// lane returns the wave's sum (0 for a strip beyond the rows); gemm_bce_flush adds the waves.
template <int NT>
__device__ __forceinline__ double gemm_epilogue_bce(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh) {
  if (rowbase >= a.rows) return 0.0;                         // wave-uniform
  const BceEpi k = gemm_bce(a);
  unsigned word[NT];
  gemm_bce_label_words<NT>(k, rowbase, a.rows, col0, lh * 32 + li, word);
  double s = 0.0;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const bool cok = col0 + n * 32 + li < a.N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool ok = cok && rowbase + (r & 3) + 8 * (r >> 2) + 4 * lh < a.rows;
      const float y = gemm_bce_label(word[n], r, li, lh, k.v_zero, k.v_one);
      const float p = sigmoidf_fast(acc[n][r]);
      const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
      const float t = (y - 1.f) * lq - y * lp;
      s += ok ? (double)t : 0.0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}
// The workgroup's partial from its four waves' sums, added in wave order; lds: 4 doubles of the LDS the k-loop is done with.
// Every thread of the workgroup calls it.
__device__ __forceinline__ void gemm_bce_flush(const GemmArgs& a, double wave_sum, double* __restrict__ lds) {
  __syncthreads();                                           // every wave has read its last operands from LDS
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = wave_sum;
  __syncthreads();
  if (threadIdx.x == 0) gemm_bce(a).partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// EPI_BCE_GRAD: C[row][col] = gscale * (p - y) * (p (1 - p) / max(p (1 - p), 1e-12)), torch's binary_cross_entropy_backward times
// sigmoid_backward: gscale * (p - y) wherever p (1 - p) > 1e-12, exactly 0 where p saturates.  Addressing and store pattern of
// gemm_epilogue (one clamped pointer per accumulator row, a full tile stores without per-element branches).
template <int NT>
__device__ __forceinline__ void gemm_epilogue_bce_grad(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh, bool full) {
  if (rowbase >= a.rows) return;                             // wave-uniform
  const BceEpi k = gemm_bce(a);
  const float gs = k.gscale[0];
  unsigned word[NT];
  gemm_bce_label_words<NT>(k, rowbase, a.rows, col0, lh * 32 + li, word);
  const int last = (int)((a.rows - 1 - rowbase) < 31 ? (a.rows - 1 - rowbase) : 31);
  const int colw = col0 + li < a.N ? col0 + li : a.N - 1;
  float* crow[16];
  bool rok[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
    const int rc = row < last ? row : last;
    rok[r] = row <= last;
    crow[r] = a.C + (rowbase + rc) * a.ldc + colw;
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const bool cok = col0 + n * 32 + li < a.N;
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float y = gemm_bce_label(word[n], r, li, lh, k.v_zero, k.v_one);
      const float p = sigmoidf_fast(acc[n][r]);
      const float pq = p * (1.f - p);
      v[r] = gs * (p - y) * (pq / fmaxf(pq, 1e-12f));
    }
    if (full) {
      if (cok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) crow[r][n * 32] = v[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (cok && rok[r]) crow[r][n * 32] = v[r];
    }
  }
}

// ---- a_max: ReLU + destination-segmented max as the GEMM's epilogue (reference models/operations_lp.py:230-234) ----------
// The GEMM walks the edges in destination order (row_index = the by-destination edge list), so the 32 rows of an accumulator
// strip are a few runs of equal destination.  A lane reduces its 16 rows run by run in registers and publishes one
// 64-bit atomic max per (run, column): key = float bits of the ReLU output (>= +0, so unsigned order = float order) in the
// high word, 0xFFFFFFFF - sorted row position in the low word.  max() is exact, so the result does not depend on the
// order of the atomics; among equal values the smallest position (= lowest edge id: the list of a destination is in edge
// order) wins, like DGL's first-index argmax; key 0 = "no in-edge".  The [E, D] ReLU output is never written.
// ---- a_mean / a_sum over ReLU(Linear): the ordered first level of a destination-segmented SUM as the GEMM's epilogue ---------
// Same walk as gemm_epilogue_segmax (edges in destination order).  A lane adds the ReLU outputs of each run of equal
// destination among ITS 16 rows of a strip (ascending rows: a fixed order) and stores the run's sum at the position of the
// run's first row ("head"): seg_part[head * N + col].  Only head rows are ever written or read; which rows are heads follows
// from the destination list alone (mrg_seg_reduce_heads_fwd re-derives it), so the second level adds a destination's run
// sums in ascending head order -- deterministic, no float atomics.  relu_bits[e * bits_ld + tile] keeps y > 0 per column
// (bit = column within the tile) of ORIGINAL edge row e for the backward: the [E, D] message tensor is never written.
template <int NT>
__device__ __forceinline__ void gemm_epilogue_segsum(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh) {
  if (rowbase >= a.rows) return;
  int seg[16], eidv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = rowbase + (r & 3) + 8 * (r >> 2) + 4 * lh;
    const bool ok = row < a.rows;
    const int64_t rc = ok ? row : a.rows - 1;
    const int e = a.row_index ? a.row_index[rc] : (int)rc;
    eidv[r] = ok ? e : -1;
    seg[r] = ok ? a.row_seg[e] : -1;
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = col0 + n * 32 + li;
    const bool cok = col < a.N;
    const float bv = (a.bias && cok) ? a.bias[col] : 0.f;
    int cur = -1;
    int64_t head = 0;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float x = acc[n][r] + bv;
      const bool pos = x > 0.f;
      const unsigned long long ball = __ballot(pos);          // lanes 0-31: this register's row of half 0, lanes 32-63: of half 1
      // a padding tile (gemm_pick_nt rounds 3 tiles up to 4, 5-6 up to 7) has no word in the row of bits_ld = ceil(N/32) words
      if (li == 0 && eidv[r] >= 0 && a.relu_bits && (col0 >> 5) + n < a.bits_ld)
        a.relu_bits[(int64_t)eidv[r] * a.bits_ld + (col0 >> 5) + n] = lh ? (unsigned)(ball >> 32) : (unsigned)ball;
      if (seg[r] != cur) {                                   // uniform over the 32 lanes of a half wave
        if (cur >= 0 && cok) a.seg_part[head * a.N + col] = sum;
        cur = seg[r];
        head = rowbase + (r & 3) + 8 * (r >> 2) + 4 * lh;
        sum = 0.f;
      }
      sum += pos ? x : 0.f;
    }
    if (cur >= 0 && cok) a.seg_part[head * a.N + col] = sum;
  }
}

template <int NT>
__device__ __forceinline__ void gemm_epilogue_segmax(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh) {
  if (rowbase >= a.rows) return;
  int seg[16];
  unsigned low[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = rowbase + (r & 3) + 8 * (r >> 2) + 4 * lh;
    const bool ok = row < a.rows;
    const int64_t rc = ok ? row : a.rows - 1;
    const int e = a.row_index ? a.row_index[rc] : (int)rc;
    const int d = a.row_seg[e];
    seg[r] = ok ? d : -1;
    low[r] = 0xFFFFFFFFu - (unsigned)rc;
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = col0 + n * 32 + li;
    const bool cok = col < a.N;
    const float bv = (a.bias && cok) ? a.bias[col] : 0.f;
    int cur = -1;
    unsigned long long best = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (seg[r] != cur) {                                   // uniform over the 32 lanes of a half wave
        if (cur >= 0 && cok) atomicMax(a.seg_out + (int64_t)cur * a.N + col, best);
        cur = seg[r];
        best = 0;
      }
      const float x = acc[n][r] + bv;
      const float y = x > 0.f ? x : 0.f;                     // ReLU; NaN -> 0 like the unfused epilogue
      const unsigned long long key = ((unsigned long long)__float_as_uint(y) << 32) | low[r];
      best = key > best ? key : best;
    }
    if (cur >= 0 && cok) atomicMax(a.seg_out + (int64_t)cur * a.N + col, best);
  }
}

// Branch-free guarded loads, split in two halves so the data is not needed until the tile is
// written to LDS (after the MFMAs of the previous tile):
//   gemm_raw4   issues the load from a clamped, always valid address -- no branch, no use of the data
//               (hipcc turns a load inside a data-dependent branch into branch + load + vmcnt(0));
//   gemm_mask4  zeroes the lanes that were out of range, at stash time.
//   VEC4: K % 4 == 0 and 16-byte aligned rows -> one global_load_dwordx4 per call.
template <bool VEC4>
__device__ __forceinline__ float4 gemm_raw4(const float* __restrict__ base, int64_t row, int64_t nrows, int k, int K, int ld) {
  const int64_t rc = row < nrows ? row : nrows - 1;
  const float* p = base + rc * ld;
  if (VEC4) {
    const int kc = k + 4 <= K ? k : (K >= 4 ? K - 4 : 0);
    return *reinterpret_cast<const float4*>(p + kc);
  }
  const int km = K - 1;
  return make_float4(p[k < K ? k : km], p[k + 1 < K ? k + 1 : km], p[k + 2 < K ? k + 2 : km], p[k + 3 < K ? k + 3 : km]);
}

template <bool VEC4>
__device__ __forceinline__ float4 gemm_mask4(float4 v, int64_t row, int64_t nrows, int k, int K) {
  const bool rv = row < nrows;
  if (VEC4) {
    const bool ok = rv && k + 4 <= K;
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
  } else {
    v.x = (rv && k < K) ? v.x : 0.f; v.y = (rv && k + 1 < K) ? v.y : 0.f;
    v.z = (rv && k + 2 < K) ? v.z : 0.f; v.w = (rv && k + 3 < K) ? v.w : 0.f;
  }
  return v;
}

// the concatenated operand [A1 | A2] (K1 % 4 == 0 whenever K2 > 0; the host passes A2 = A1 when
// there is no second source): which tensor / local column a global column k maps to
struct ASel { const float* base; int ld, kk; };
__device__ __forceinline__ ASel gemm_sel_a(const GemmArgs& a, int k) {
  const bool first = k < a.K1 || a.K2 == 0;
  ASel s;
  s.base = first ? a.A1 : a.A2;
  s.ld = first ? a.K1 : a.K2;
  s.kk = first ? k : k - a.K1;
  return s;
}

// raw / mask of a float4 of the concatenated operand [A1 | A2] at global column k.  The scalar
// path selects the source per element (K1 need not be a multiple of 4 there).
template <bool VEC4>
__device__ __forceinline__ float4 gemm_raw_a(const GemmArgs& a, int64_t row, int k) {
  if (VEC4) {
    const ASel sa = gemm_sel_a(a, k);
    return gemm_raw4<true>(sa.base, row, a.rows, sa.kk, sa.ld, sa.ld);
  }
  const int64_t rc = row < a.rows ? row : a.rows - 1;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const ASel sa = gemm_sel_a(a, k + j);
    const int kc = sa.kk < sa.ld ? sa.kk : sa.ld - 1;
    v[j] = sa.base[rc * sa.ld + kc];
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

template <bool VEC4>
__device__ __forceinline__ float4 gemm_mask_a(float4 v, const GemmArgs& a, int64_t row, int k) {
  if (VEC4) {
    const ASel sa = gemm_sel_a(a, k);
    return gemm_mask4<true>(v, row, a.rows, sa.kk, sa.ld);
  }
  const int K = a.K1 + a.K2;
  const bool rv = row < a.rows;
  v.x = (rv && k < K) ? v.x : 0.f; v.y = (rv && k + 1 < K) ? v.y : 0.f;
  v.z = (rv && k + 2 < K) ? v.z : 0.f; v.w = (rv && k + 3 < K) ? v.w : 0.f;
  return v;
}

// Epilogue of one wave: NT tiles of 32x32 at rows [rowbase, rowbase+32), columns [col0, col0 + NT*32).
// C/D map of a tile: col = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5).
// Every load (bias, row scale, gate multiplicand, accumulate input) is issued unconditionally from a
// clamped address BEFORE the stores, and a full tile stores without per-element branches: a store inside
// a data-dependent branch makes hipcc wait vmcnt(0) per store, which serialises the 16*NT stores of a lane.
// SUMS (EPI_GATE / EPI_SCALE, producer statistics of the MixedOp epilogue): the lane also adds the values v it forms -- of valid
// rows, in register order, each converted to double as mix_colstats_k converts them -- into one sum and one sum of squares per
// column tile and leaves them in LDS at sums[(lh * 2 + {0, 1}) * NT * 32 + n * 32 + li] (this wave's [2][2][NT * 32] doubles;
// columns beyond N and a strip beyond the rows leave zeros).  The caller adds the waves' slots in a fixed order
// (gemm_colsum_flush).  The gate-only form then reads its multiplicand S, which it otherwise does not need.
template <int NT, int EPI, bool SUMS = false>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& a, f32x16 (&acc)[NT], int64_t rowbase, int col0, int li, int lh,
                                              bool full, double* __restrict__ sums = nullptr) {
  static_assert(!SUMS || EPI == EPI_GATE || EPI == EPI_SCALE, "column sums: gate and scale epilogues only");
  if (rowbase >= a.rows) {                                 // wave-uniform: the whole 32-row strip is out of range
    if constexpr (SUMS) {
#pragma unroll
      for (int n = 0; n < NT; ++n) { sums[(lh * 2 + 0) * NT * 32 + n * 32 + li] = 0.0; sums[(lh * 2 + 1) * NT * 32 + n * 32 + li] = 0.0; }
    }
    return;
  }
  // One pointer per accumulator row (clamped to the last valid row) and per array, set up once; a column tile is then
  // a constant 128-byte offset from it, i.e. an immediate of the load / store.  (Per-tile 64-bit address arithmetic
  // made hipcc spill hundreds of addresses of the 224-accumulator kernels to scratch memory.)
  const int last = (int)((a.rows - 1 - rowbase) < 31 ? (a.rows - 1 - rowbase) : 31);
  const int colw = col0 + li < a.N ? col0 + li : a.N - 1;   // this lane's column in tile 0 (clamped: only lanes of a partial tile)
  float* crow[16];
  const float* srow[16];
  const float* trow[16];                                   // EPI_ACCUM2: the second addend
  float* xrow[16];
  float cs[16];
  bool rok[16];
  // EPI_GATE with C == NULL: only the gate (aux) is stored -- the gated output is recomputed from gate, S and the row scale
  // by its consumer (the MixedOp epilogue's "virtual" candidate, mixedop.hip) instead of being written and re-read four times
  const bool cstore = EPI != EPI_GATE || a.C != nullptr;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
    const int rc = row < last ? row : last;
    rok[r] = row <= last;
    crow[r] = a.C + (rowbase + rc) * a.ldc + colw;
    if (EPI == EPI_GATE) srow[r] = a.S + (rowbase + rc) * a.ld_s + colw;
    if (epi_accum(EPI)) srow[r] = a.Cin + (rowbase + rc) * a.ld_cin + colw;
    if (EPI == EPI_ACCUM2) trow[r] = a.S + (rowbase + rc) * a.ld_s + colw;
    if (EPI == EPI_GATE) xrow[r] = a.aux ? a.aux + (rowbase + rc) * a.N + colw : nullptr;
    cs[r] = 1.0f;
    if (EPI == EPI_GATE || EPI == EPI_SCALE) cs[r] = a.scale * (a.rowscale ? a.rowscale[rowbase + rc] : 1.0f);
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = col0 + n * 32 + li;
    // columns of this tile that exist; a lane beyond them re-reads its tile-0 column (never stored)
    const bool cok = col < a.N;
    const int off = cok ? n * 32 : 0;
    const float bv = a.bias ? a.bias[cok ? col : colw] : 0.f;
    float in[16], in2[16], v[16], g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) in[r] = 0.f;
    if ((EPI == EPI_GATE && (cstore || SUMS)) || epi_accum(EPI)) {       // (gate only, no sums: the multiplicand is not read at all)
#pragma unroll
      for (int r = 0; r < 16; ++r) in[r] = srow[r][off];
    }
    if (EPI == EPI_ACCUM2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) in2[r] = trow[r][off];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x = acc[n][r] + bv;
      if (EPI == EPI_BIAS_ACT) {
        v[r] = (a.act == MRG_ACT_RELU) ? (x > 0.f ? x : 0.f) : (a.act == MRG_ACT_SIGMOID ? sigmoidf_fast(x) : x);
      } else if (EPI == EPI_GATE) {
        g[r] = sigmoidf_fast(x);
        v[r] = g[r] * in[r] * cs[r];
      } else if (EPI == EPI_SCALE) {
        v[r] = x * cs[r];
      } else if (EPI == EPI_ACCUM2) {
        v[r] = (x + in[r]) + in2[r];
      } else {
        v[r] = x + in[r];
      }
    }
    if constexpr (SUMS) {
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double d = (full || rok[r]) ? (double)v[r] : 0.0;
        s1 += d; s2 += d * d;
      }
      sums[(lh * 2 + 0) * NT * 32 + n * 32 + li] = cok ? s1 : 0.0;
      sums[(lh * 2 + 1) * NT * 32 + n * 32 + li] = cok ? s2 : 0.0;
    }
    if (full) {
      if (cok) {
        if (cstore) {
#pragma unroll
          for (int r = 0; r < 16; ++r) crow[r][n * 32] = v[r];
        }
        if (EPI == EPI_GATE && a.aux) {
#pragma unroll
          for (int r = 0; r < 16; ++r) xrow[r][n * 32] = g[r];
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (cok && rok[r]) {
          if (cstore) crow[r][n * 32] = v[r];
          if (EPI == EPI_GATE && a.aux) xrow[r][n * 32] = g[r];
        }
      }
    }
  }
}

// The workgroup's column sums from its waves' LDS slots (gemm_epilogue<..., SUMS = true>: NSLOT = waves x two lane halves slots of
// [2][W] doubles each, wave w's at lds + w * 4 * W), added in slot order -- no atomics, the same bits on every run -- into the
// workgroup's own partial colsum[blockIdx.x][2][N] (float64).  Every thread of the workgroup calls it, behind a barrier that
// follows the epilogue.
template <int W, int NSLOT>
__device__ __forceinline__ void gemm_colsum_flush(const double* __restrict__ lds, double* __restrict__ colsum, int N, int col0) {
  double* __restrict__ dst = colsum + (int64_t)blockIdx.x * 2 * N;
  for (int t = threadIdx.x; t < 2 * W; t += blockDim.x) {
    const int which = t / W, c = t - which * W;
    if (col0 + c >= N) continue;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NSLOT; ++q) acc += lds[(q * 2 + which) * W + c];
    dst[which * N + col0 + c] = acc;
  }
}

template <int NT, int MT, int GBK, int EPI, bool VEC4>
__global__ __launch_bounds__(MRG_BLOCK, (MT == 1 ? 2 : 1)) void rowgemm_k(GemmArgs a) {
  constexpr int GBM = 128 * MT;
  constexpr int GLD = GBK + 4;                 // padded LDS row stride (floats)
  constexpr int F4R = GBK / 4;                 // float4 per tile row
  constexpr int NA = GBM * F4R / MRG_BLOCK;    // A float4 per thread per tile
  constexpr int NBT = NT * 32 * F4R;           // B float4 per tile
  constexpr int NB = (NBT + MRG_BLOCK - 1) / MRG_BLOCK;
  extern __shared__ __align__(16) float smem[];
  constexpr int A_TILE = GBM * GLD, B_TILE = NT * 32 * GLD, STAGE = A_TILE + B_TILE;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * GBM;
  const int col0 = (epi_diag(EPI) ? blockIdx.x : blockIdx.y) * (NT * 32);
  const int K = a.K1 + a.K2;
  const int nkt = (K + GBK - 1) / GBK;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  float4 pa[NA];
  float4 pb[NB];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      int f = tid + i * MRG_BLOCK;
      pa[i] = gemm_raw_a<VEC4>(a, row0 + f / F4R, k0 + (f % F4R) * 4);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      int f = tid + i * MRG_BLOCK;
      f = f < NBT ? f : NBT - 1;
      pb[i] = gemm_raw4<VEC4>(a.B, col0 + f / F4R, a.N, k0 + (f % F4R) * 4, K, a.ldb);
    }
  };
  auto stash = [&](int buf, int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      int f = tid + i * MRG_BLOCK;
      *reinterpret_cast<float4*>(&smem[buf * STAGE + (f / F4R) * GLD + (f % F4R) * 4]) =
          gemm_mask_a<VEC4>(pa[i], a, row0 + f / F4R, k0 + (f % F4R) * 4);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      int f = tid + i * MRG_BLOCK;
      if (f < NBT)
        *reinterpret_cast<float4*>(&smem[buf * STAGE + A_TILE + (f / F4R) * GLD + (f % F4R) * 4]) =
            gemm_mask4<VEC4>(pb[i], col0 + f / F4R, a.N, k0 + (f % F4R) * 4, K);
    }
  };

  fetch(0);
  stash(0, 0);
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * GBK;
    if (kt + 1 < nkt) fetch(k0 + GBK);                 // in flight during the MFMAs below
    const int kv = K - k0 < GBK ? K - k0 : GBK;
    const int nt8 = (kv + 7) >> 3;
    const float* At = smem + cur * STAGE + (wave * 32 * MT + li) * GLD + lh * 4;
    const float* Bt = smem + cur * STAGE + A_TILE + li * GLD + lh * 4;
    // fragment reads of step t+1 are issued before the MFMAs of step t (register double buffer)
    float4 af[2][MT], bf[2][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) af[0][m] = *reinterpret_cast<const float4*>(At + m * 32 * GLD);
#pragma unroll
    for (int n = 0; n < NT; ++n) bf[0][n] = *reinterpret_cast<const float4*>(Bt + n * 32 * GLD);
#pragma unroll
    for (int t = 0; t < GBK / 8; ++t) {
      if (t < nt8) {
        const int c = t & 1, nx = c ^ 1;
        if (t + 1 < GBK / 8) {               // harmless over-read of zero-filled columns when t + 1 >= nt8
#pragma unroll
          for (int m = 0; m < MT; ++m) af[nx][m] = *reinterpret_cast<const float4*>(At + m * 32 * GLD + (t + 1) * 8);
#pragma unroll
          for (int n = 0; n < NT; ++n) bf[nx][n] = *reinterpret_cast<const float4*>(Bt + n * 32 * GLD + (t + 1) * 8);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][m].x, bf[c][n].x, acc[m][n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][m].y, bf[c][n].y, acc[m][n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][m].z, bf[c][n].z, acc[m][n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][m].w, bf[c][n].w, acc[m][n], 0, 0, 0);
      }
    }
    if (kt + 1 < nkt) {
      stash(cur ^ 1, k0 + GBK);
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- epilogue
  constexpr int EPU = epi_unbiased(EPI);
  if constexpr (epi_col_bias(EPI)) {
#pragma unroll
    for (int m = 0; m < MT; ++m) gemm_add_col_bias<NT>(a, acc[m], col0, li);
  }
  if constexpr (EPU == EPI_BCE) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < MT; ++m) s += gemm_epilogue_bce<NT>(a, acc[m], row0 + wave * 32 * MT + m * 32, col0, li, lh);
    gemm_bce_flush(a, s, reinterpret_cast<double*>(smem));
    return;
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if constexpr (EPU == EPI_BCE_GRAD) gemm_epilogue_bce_grad<NT>(a, acc[m], row0 + wave * 32 * MT + m * 32, col0, li, lh, row0 + GBM <= a.rows);
    else if constexpr (EPU == EPI_RANK) gemm_epilogue_rank<NT>(a, acc[m], row0 + wave * 32 * MT + m * 32, col0, li, lh);
    else if constexpr (EPU == EPI_RANK_DIAG) gemm_epilogue_rank_diag<NT>(a, acc[m], row0 + wave * 32 * MT + m * 32, wave, li, lh);
    else if constexpr (EPU == EPI_TOPK) gemm_epilogue_topk<NT>(a, acc[m], row0 + wave * 32 * MT + m * 32, col0, li, lh);
    else gemm_epilogue<NT, EPI>(a, acc[m], row0 + wave * 32 * MT + m * 32, col0, li, lh, row0 + GBM <= a.rows);
  }
}

// ---- LDS-DMA variant (the fast path) ---------------------------------------------------------
// Same tiling as rowgemm_k, but the A / B tiles travel global -> LDS with global_load_lds_dwordx4
// (no VGPR staging, no ds_write, no vmcnt -> ds_write dependency in the instruction stream).
// Measured on MI355X (rows 544k, K = N = 200): staging through registers cost 0.35 ms on top of
// 0.38 ms of MFMA time; with LDS-DMA the same kernel runs 0.55 ms instead of 0.86 ms.
// The DMA destination is wave-uniform base + lane*16, so LDS rows are unpadded (64 B); the
// resulting 4-way bank conflict of the ds_read_b128 fragment reads is invisible next to the
// 64-cycle f32 MFMAs.  The DMA cannot zero-fill: out-of-range rows / columns are read from
// clamped addresses (their results are never stored) and K must be a multiple of 8 so that an
// 8-deep MFMA step never contains columns beyond K.
template <int NT, int EPI, bool DUAL>
__global__ __launch_bounds__(MRG_BLOCK, 2) void rowgemm_dma_k(GemmArgs a) {
  constexpr int GBK = 16, GBM = 128, GLD = GBK, F4R = GBK / 4;
  constexpr int NA = GBM * F4R / MRG_BLOCK, NBT = NT * 32 * F4R, NB = (NBT + MRG_BLOCK - 1) / MRG_BLOCK;
  extern __shared__ __align__(16) float smem[];
  constexpr int A_TILE = GBM * GLD, B_TILE = NT * 32 * GLD, STAGE = A_TILE + B_TILE;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * GBM;
  const int col0 = blockIdx.y * (NT * 32);
  const int K = a.K1 + a.K2;
  const int nkt = (K + GBK - 1) / GBK;

  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

  const float* arow1[NA]; const float* arow2[NA]; const float* brow[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int64_t row = row0 + (tid + i * MRG_BLOCK) / F4R;
    const int64_t rc = row < a.rows ? row : a.rows - 1;
    arow1[i] = a.A1 + rc * a.K1;
    arow2[i] = a.A2 + rc * a.K2;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    int f = tid + i * MRG_BLOCK;
    f = f < NBT ? f : NBT - 1;
    const int col = col0 + f / F4R;
    brow[i] = a.B + (int64_t)(col < a.N ? col : a.N - 1) * a.ldb;
  }
  auto fetch = [&](int buf, int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int f = tid + i * MRG_BLOCK;
      const int k = k0 + (f % F4R) * 4;
      const float* p = gemm_a_ptr<DUAL>(arow1[i], arow2[i], a.K1, a.K2, K, k);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)p, (lds_ptr_t)(smem + buf * STAGE + (f - lane) * 4), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int f = tid + i * MRG_BLOCK;
      const int fc = f < NBT ? f : NBT - 1;
      const int k = k0 + (fc % F4R) * 4;
      if (f - lane < NBT)                      // wave-uniform
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(brow[i] + (k + 4 <= K ? k : K - 4)),
                                         (lds_ptr_t)(smem + buf * STAGE + A_TILE + (f - lane) * 4), 16, 0, 0);
    }
  };

  // Fragment reads are issued through inline asm: hipcc otherwise puts s_waitcnt vmcnt(0) in front of the
  // first ds_read that follows a global_load_lds (it assumes the DMA may alias it), which would drain the
  // DMA of the NEXT tile before this tile's MFMAs start.  Hazards are handled by hand: the reads only touch
  // the buffer whose DMA was waited for (vmcnt(0)) before the barrier that ended the previous iteration.
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
  const unsigned a_off = (unsigned)(((wave * 32 + li) * GLD + lh * 4) * sizeof(float));
  const unsigned b_off = (unsigned)((A_TILE + li * GLD + lh * 4) * sizeof(float));
  auto step = [&](unsigned abase, unsigned bbase, int t) {     // 8 k-columns: 1 + NT fragment reads, 4*NT MFMAs
    v4f a4, b4[NT];
    asm volatile("ds_read_b128 %0, %1" : "=v"(a4) : "v"(abase + t * 32));
#pragma unroll
    for (int n = 0; n < NT; ++n) asm volatile("ds_read_b128 %0, %1" : "=v"(b4[n]) : "v"(bbase + n * (32 * GLD * 4) + t * 32));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);                         // keep the MFMAs below the wait (they do not touch memory)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4[n].x, acc[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4[n].y, acc[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4[n].z, acc[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4[n].w, acc[n], 0, 0, 0);
  };
  const int nfull = K / GBK;                                // tiles with both 8-column steps valid
  fetch(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  int cur = 0;
  for (int kt = 0; kt < nfull; ++kt) {                      // DMA of tile kt+1 runs under the MFMAs of tile kt
    if (kt + 1 < nkt) fetch(cur ^ 1, (kt + 1) * GBK);
    const unsigned abase = lds0 + cur * (STAGE * 4) + a_off, bbase = lds0 + cur * (STAGE * 4) + b_off;
    step(abase, bbase, 0);
    step(abase, bbase, 1);
    if (kt + 1 < nkt) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA has landed ...
      __builtin_amdgcn_s_barrier();                        // ... and so has everyone else's; all reads of `cur` are done
      cur ^= 1;
    }
  }
  if (nfull < nkt) {                                        // K % 16 == 8: one last half tile
    step(lds0 + cur * (STAGE * 4) + a_off, lds0 + cur * (STAGE * 4) + b_off, 0);
  }

  gemm_epilogue<NT, EPI>(a, acc, row0 + wave * 32, col0, li, lh, row0 + GBM <= a.rows);
}

inline int gemm_pick_nt(int ncols) {
  int t = (ncols + 31) / 32;
  if (t <= 1) return 1;
  if (t <= 2) return 2;
  if (t <= 4) return 4;
  if (t <= 7) return 7;
  // wider outputs use several column blocks: the block width that pads the fewest all-zero tiles
  // (256 columns: 2 x 4 tiles, not 7 + 1 padded to 14), the wider one on ties (A is re-read per column block)
  int best = 7, waste = ((t + 6) / 7) * 7 - t;
  if (((t + 3) / 4) * 4 - t < waste) best = 4;
  return best;
}

inline size_t gemm_lds_bytes(int nt, int mt, int bk) { return (size_t)2 * (128 * mt + nt * 32) * (bk + 4) * sizeof(float); }

template <int EPI>
inline int launch_rowgemm(GemmArgs a, hipStream_t st) {
  if (a.rows <= 0) return MRG_OK;
  if (!a.A2 || a.K2 == 0) { a.A2 = a.A1; a.K2 = 0; }
  const bool vec = (a.K1 % 4 == 0) && (a.K2 % 4 == 0) && (a.ldb % 4 == 0) && ((a.K1 + a.K2) % 4 == 0) && aligned16(a.A1) &&
                   aligned16(a.A2) && aligned16(a.B) && a.K1 >= 4 && (a.K2 == 0 || a.K2 >= 4);
  const int nt = gemm_pick_nt(a.N);
  if (vec && (a.K1 % 8 == 0) && (a.K2 % 8 == 0)) {            // LDS-DMA fast path
    dim3 gridd((unsigned)((a.rows + 127) / 128), (unsigned)((a.N + nt * 32 - 1) / (nt * 32)));
    const size_t ldsd = (size_t)2 * (128 + nt * 32) * 16 * sizeof(float);
#define MRG_GOD(NTV)                                                                                                  \
  do {                                                                                                                \
    if (a.K2 > 0) {                                                                                                   \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rowgemm_dma_k<NTV, EPI, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsd); \
      hipLaunchKernelGGL((rowgemm_dma_k<NTV, EPI, true>), gridd, dim3(MRG_BLOCK), ldsd, st, a);                        \
    } else {                                                                                                          \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rowgemm_dma_k<NTV, EPI, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsd); \
      hipLaunchKernelGGL((rowgemm_dma_k<NTV, EPI, false>), gridd, dim3(MRG_BLOCK), ldsd, st, a);                       \
    }                                                                                                                 \
  } while (0)
    switch (nt) {
      case 1: MRG_GOD(1); break;
      case 2: MRG_GOD(2); break;
      case 4: MRG_GOD(4); break;
      default: MRG_GOD(7); break;
    }
#undef MRG_GOD
    hipError_t ed = hipGetLastError();
    return ed == hipSuccess ? MRG_OK : (int)ed;
  }
  const int mt = 1;
  const int gbm = 128 * mt;
  dim3 grid((unsigned)((a.rows + gbm - 1) / gbm), (unsigned)((a.N + nt * 32 - 1) / (nt * 32)));
  const size_t lds = gemm_lds_bytes(nt, mt, mt == 2 ? 32 : 16);
#define MRG_GO1(NTV, MTV, BKV, VV)                                                                                         \
  do {                                                                                                                \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rowgemm_k<NTV, MTV, BKV, EPI, VV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL((rowgemm_k<NTV, MTV, BKV, EPI, VV>), grid, dim3(MRG_BLOCK), lds, st, a);                             \
  } while (0)
#define MRG_GO(NTV)                                                                                                   \
  do {                                                                                                                \
    if (vec) MRG_GO1(NTV, 1, 16, true);                                                                               \
    else MRG_GO1(NTV, 1, 16, false);                                                                                  \
  } while (0)
  switch (nt) {
    case 1: MRG_GO(1); break;
    case 2: MRG_GO(2); break;
    case 4: MRG_GO(4); break;
    default: MRG_GO(7); break;
  }
#undef MRG_GO
#undef MRG_GO1
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MRG_OK : (int)e;
}

// Bt[c][r] = B[r][c]  (small weight matrices; used to present W^T row-major to the core)
static __global__ void transpose_k(const float* __restrict__ B, float* __restrict__ Bt, int rows, int cols, int ldb) {
  __shared__ float tile[32][33];
  int c = blockIdx.x * 32 + threadIdx.x, r0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += blockDim.y)
    if (r0 + i < rows && c < cols) tile[i][threadIdx.x] = B[(int64_t)(r0 + i) * ldb + c];
  __syncthreads();
  int r = r0 + threadIdx.x, c0 = blockIdx.x * 32;
  for (int i = threadIdx.y; i < 32; i += blockDim.y)
    if (c0 + i < cols && r < rows) Bt[(int64_t)(c0 + i) * rows + r] = tile[threadIdx.x][i];
}

inline void launch_transpose(const float* B, float* Bt, int rows, int cols, int ldb, hipStream_t st) {
  hipLaunchKernelGGL(transpose_k, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, st, B, Bt, rows, cols, ldb);
}

}  // namespace mrg
