/*
 * mrgnas.h -- C ABI of libmrgnas_hip.so: the MI355X (gfx950) implementation of
 * MR-GNAS's relational message-passing hot path.
 *
 * The reference (Amanda-Zheng/MR-GNAS) is pure Python on PyTorch + DGL and has
 * no FFI of its own; each entry point below replaces the ATen/DGL kernel
 * sequence that one reference operator launches.  The citation on each
 * function is the reference interface it stands in for (paths relative to the
 * reference repository root).  INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *  - float tensors are float32, row-major, contiguous (leading dimension == D);
 *  - graph index arrays are int32;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); every
 *    call only enqueues work on that stream -- no allocation, no
 *    synchronisation, safe to capture into a hipGraph;
 *  - scratch memory is caller-owned: ask mrg_*_workspace_bytes(), pass `ws`;
 *  - return value: 0 = success, < 0 = argument error (MRG_E_*), > 0 = the
 *    hipError_t of the failed launch.  mrg_error_string() explains either.
 *  - row layout of every [M, D] edge tensor, M = E + N: rows [0, b0) original
 *    direction ("in") edges, [b0, b1) inverse ("out") edges, [b1, M) one
 *    self-loop row per node (reference models/model_lp.py:126-129,
 *    models/model_search_lp.py:135-139).  The reference always has b0 = E/2,
 *    b1 = E; relation-block shards pass their local boundaries.
 */
#ifndef MRGNAS_H
#define MRGNAS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRG_ABI_VERSION 23   /* 23 (addition, no bump): mrg_unrolled_virtual_step, mrg_unrolled_radius, mrg_unrolled_shift, mrg_unrolled_alpha_grad (the parameter passes of the second-order DARTS architect step over the pointer tables of mrg_clip_sgd_step); 23 (addition, no bump): mrg_rows_bias_bce_fwd / _dlogit, mrg_rows_bias_rank, mrg_rows_bias_topk, mrg_cols_sum (the "dot" sweeps under a per-entity score bias: CompGCN_ConvE without a [B, N] tensor); 23 (addition, no bump): mrg_linear_bwd_input_acc2, mrg_linear_bwd_input3_acc2, mrg_linear_bwd_input3_pair_acc2, mrg_segmax_bwd_input_chain, mrg_gate_row_bwd_acc (the gradient fan-in chain: a reader adds the running sum of the other readers' gradients in its own last store); 23 (addition, no bump): mrg_rows_rank, mrg_transe_bce_fwd / _dlogit / _workspace_bytes, mrg_transe_dist_bwd, mrg_transe_rank / _workspace_bytes (1-N loss and ranks of ConvE and TransE without [B, N] tensors); 23 (addition, no bump: nothing existing changed, and tests pin the number): mrg_distmult_rank, mrg_distmult_rank_workspace_bytes (raw / filtered DistMult ranks as a row GEMM with a counting epilogue); 23: mrg_gemm_set_epilogue removed (the row-order and transposed-accumulator store orders of the split-core row GEMM, measured slower, left the library; accumulator-order stores remain), mrg_gemm_set_wide8 and mrg_gemm_set_small take 0 or 1 only; 22: mrg_cand_linear_fwd, mrg_cand_linear_bwd_input, mrg_cand_linear_colsum_blocks, mrg_cand_linear_workspace_bytes (the candidate Linears of one node-classification MixedOp in one launch, BatchNorm sums included); 21: mrg_adam_step (multi-tensor Adam over the pointer tables of mrg_clip_sgd_step, two launches; per-tensor step counts and lr in device memory); 20: BatchNorm sums formed by a candidate's producer: mrg_gated_branch.given / given_n / given_stride (mrg_mix_stats_coef skips the sweep over such a candidate), mrg_dense_filter3_colsum_blocks, mrg_dense_filter_fwd3_colsum, mrg_gate_row_colsum_blocks, mrg_gate_row_fwd_colsum; 19: mrg_seg_std_workspace_bytes, mrg_seg_std_fwd, mrg_seg_std_bwd (a_std, the standard-deviation aggregator of the node-classification task); 18: mrg_conve_* (the ConvE feature path: BN0 statistics, conv, BN1, split-K fc and their gradients, stacked or interleaved image layout); 17: mrg_ccorr_rows, mrg_ccorr_matrix, mrg_ccorr_matrix_grad (standalone circular correlation: per-row kernel, and the circulant of a shared row with its gradient fold for the row GEMM); 16: mrg_set_stream_blocks, mrg_gate_collapse and mrg_gate_param_grad removed (the streaming grid bound is fixed; the three-segment forms remain); 15: mrg_gated_branch.valid_rows and the valid_rows argument of mrg_mix_finalize_bwd / mrg_zero_* except colstats (the device row count of a static step graph, passed per call instead of the process-wide registry of 13), mrg_linear_bwd_weight_share (the weight gradient of one range of a grouped launch, instead of the process-wide setter of 14); 14: mrg_clip_sgd_step, mrg_optim_chunk (clip_grad_norm_ + SGD with momentum over every parameter tensor in three launches), mrg_gated_branch.act (tanh behind the BatchNorm: CompGraphConv's tail on the epilogue kernels), mrg_gemm_set_small (few-row products on two-tile column blocks), a weight-gradient share setter, mrg_segmax_bwd_input (a_max's input gradient without a dense product); 13: a registry of device-side row counts (the sampled search step as one replayable HIP graph), mrg_seg_reduce_bwd_ordered (aggregator backward walked in destination order), mrg_gemm_set_q (the 16 x 16 x 32 row GEMM at three workgroups per CU for 129..224 output columns); 12: mrg_act_grad_transpose (the [B, N] scorer's output gradient, activation folded in, as [N, B] rows); 11: mrg_gemm_set_wide8 (eight-tile column block for D = 256); 10: mrg_gemm_set_epilogue(2) (transposed accumulators: a tested comparison point); 9: mrg_gated_branch (the MixedOp epilogue recomputes f_dense_comp's output from its gate and f_sparse_comp's from its row factor), mrg_gate_row_fwd / _bwd, mrg_sum_rows_gather, mrg_wgrad_set_variant, mrg_dense_filter_fwd3 out == NULL; 8: mrg_zero_* (cell-zero MixedOp recomputed from the tables), mrg_linear_bwd_input3_pair, mrg_sample_edge_neighborhood; 7: mrg_gemm_set_epilogue (row-order stores of the split-core row GEMM), mrg_set_stream_blocks, mrg_gemm_set_mode(2); 6: fused a_mean (run-sum epilogue, heads reducer, bit-mask backward), mrg_mix_stats_coef; 5: three-segment dense filter entry points; 4: mrg_linear_relu_segmax_fwd (fused a_max); 3: device graph / plan builders, samplers, [B, N] scorers, ranking; 2: GEMM workspaces, span_gcs ext_scal */

#define MRG_OK            0
#define MRG_E_NULLPTR    -1   /* a required pointer is NULL */
#define MRG_E_SHAPE      -2   /* negative size, or a size the kernels do not cover: D > 1024, or D > 256 with D % 4 != 0, or D > 256
                                * with a row pointer (inputs, output, workspace) that is not 16-byte aligned -- the scalar lanes
                                * that serve such rows cover 256 columns */
#define MRG_E_ENUM       -3   /* unknown op / mode / act code */
#define MRG_E_WORKSPACE  -4   /* workspace pointer missing */

/* compose codes (a1) */
#define MRG_COMPOSE_MULT 0
#define MRG_COMPOSE_SUB  1
#define MRG_COMPOSE_ADD  2
/* reducer codes (a4-a6) */
#define MRG_REDUCE_SUM   0
#define MRG_REDUCE_MEAN  1
#define MRG_REDUCE_MAX   2
/* compose codes of mrg_fused_gcs: x = X[xi[e]], y = Y[yi[e]], s = scal[e] (1 if scal is NULL) */
#define MRG_GCS_SUB      0   /* x - y*s                          CompGCN 'sub'  (u_sub_e)            */
#define MRG_GCS_MUL      1   /* x * (y*s)                        CompGCN 'mul'  (u_mul_e)            */
#define MRG_GCS_COPY     2   /* x*s                (Y unused)    gather backward, d/dh of 'sub'       */
#define MRG_GCS_NEGS     3   /* -(x*s)             (Y unused)    d/dr of 'sub'                        */
#define MRG_GCS_CCORR    4   /* sum_i x[i] * y[(i+k)%D] * s      CompGCN 'ccorr' and its d/dh         */
#define MRG_GCS_CCONV    5   /* s * sum_i x[i] * y[(k-i)%D]      d/dr of 'ccorr'                      */
/* activation codes for mrg_linear_fwd */
#define MRG_ACT_NONE     0
#define MRG_ACT_RELU     1
#define MRG_ACT_SIGMOID  2   /* the [B, N] score functions: sigmoid((sub * rel) all_ent^T) */

int mrg_abi_version(void);
const char *mrg_error_string(int code);
/* Name of the code object's target, e.g. "gfx950". */
const char *mrg_target_arch(void);

/* ---- a1: compose ops ---------------------------------------------------
 * pre_mult_op / pre_sub_op / pre_add_op .forward(g, src_emb, hr)
 * reference models/operations_lp.py:71-98.   out = s (*|-|+) hr, [rows, D]. */
int mrg_compose_fwd(int op, const float *s, const float *hr, float *out,
                    int64_t rows, int D, void *stream);
/* autograd of the above: gs/ghr may be NULL when not needed. */
int mrg_compose_bwd(int op, const float *gout, const float *s, const float *hr,
                    float *gs, float *ghr, int64_t rows, int D, void *stream);

/* ---- G + a1: gather feeding the compose ----------------------------------
 * all_ent_emb[src_id_final] (op) rel_embed[edge_type_final]
 * reference models/model_lp.py:126-131, models/model_search_lp.py:135-145.
 * out[i,:] = ent[ent_idx[i],:] (op) rel[rel_idx[i],:];  op = -1 copies ent rows
 * only (plain gather, rel ignored). Bit-exact. */
int mrg_gather_compose_fwd(int op, const float *ent, const float *rel,
                           const int32_t *ent_idx, const int32_t *rel_idx,
                           float *out, int64_t rows, int D, void *stream);

/* floats per (u, v, c) slot of a gate: u at [0, D), v at [D, 2D), c at index
 * in_dim (2D with s_in, D without); padded so every slot stays 16-byte aligned. */
#define MRG_GATE_LD(D) (2 * (D) + 4)

/* ---- a2 / a3: collapsed scalar gates --------------------------------------
 * f_sparse_op_comp.forward  reference models/operations_lp.py:317-343
 * f_sparse_op_last.forward  reference models/operations_lp.py:412-416
 *
 * a_x(W_x [s ; s_in] + b_x) has no non-linearity inside, so it equals
 * u_x . s + v_x . s_in + c_x with  [u_x ; v_x] = W_x^T a_x,  c_x = a_x . b_x.
 *
 * mrg_gate_collapse3:   uvc[0 .. in_dim) = W^T a,  uvc[in_dim] = a . b
 *   W [D, in_dim] (nn.Linear weight), b [D] or NULL, a [D] (nn.Linear(D,1).weight).
 * mrg_gate_param_grad3: the chain rule back to the nn.Linear parameters,  d_uvc [in_dim+1] ->
 *   gW [D, in_dim] = a (x) d_uv,  gb [D] = a * d_c (NULL ok),  ga [D] = W d_uv + b d_c.
 * Both cover the three direction segments (in, out, self) of one operator in one launch: *_host are
 * HOST arrays of 3 device pointers, NULL for an absent segment; uvc / d_uvc are [3][MRG_GATE_LD(D)].
 * fold != 0 (both operands of the operator are the same rows, reference models/cell_lp.py:95-104: op(g, h_in, h_in)): the
 * parameters are nn.Linear(2D, D) but the gate is u.s + v.s = (u + v).s -- uvc holds u + v at [0, D) and c at index D
 * (the layout of a gate without a second operand), and the parameter gradient spreads d(u + v) over both weight halves. */
int mrg_gate_collapse3(const float *const *W_host, const float *const *b_host, const float *const *a_host, float *uvc,
                       int D, int in_dim, int fold, void *stream);
int mrg_gate_param_grad3(const float *const *W_host, const float *const *b_host, const float *const *a_host,
                         const float *d_uvc, float *const *gW_host, float *const *gb_host, float *const *ga_host,
                         int D, int in_dim, int fold, void *stream);
/* The same fold for the dense filters: Wt [3][D][D], Wt_i = W_i[:, :D] + W_i[:, D:] (W_i is [D][2D]); and its adjoint
 * gW_i = [gWt_i | gWt_i] (gWt_host: 3 device pointers to [D][D]; a NULL source gives a zero gradient). */
int mrg_fold_halves3(const float *const *W_host, float *Wt, int D, void *stream);
int mrg_unfold_halves3(const float *const *gWt_host, float *const *gW_host, int D, void *stream);

/* out[i,:] = sigmoid(u_x.s_i + v_x.s_in_i + c_x) * s_i * scale * (i < b1 ? norm[i] : 1)
 *   x = segment of row i (0: i < b0, 1: b0 <= i < b1, 2: i >= b1)
 *   uvc  [3][MRG_GATE_LD(D)]  (u, v, c per segment); s_in NULL => v ignored (f_sparse_last)
 *   norm [b1] or NULL (=> 1).  f_sparse_comp: scale = 1/3; f_sparse_last: b0 = b1 = 0, scale = 1. */
int mrg_gate_fwd(const float *s, const float *s_in, const float *norm, const float *uvc,
                 float *out, int64_t b0, int64_t b1, int64_t M, int D, float scale, void *stream);
int64_t mrg_gate_bwd_workspace_bytes(int64_t M, int D);
/* gs, gs_in [M, D] (gs_in NULL allowed iff s_in NULL); d_uvc [3][MRG_GATE_LD(D)] receives
 * d(loss)/d(u, v, c) per segment (deterministic two-stage reduction, no atomics). */
int mrg_gate_bwd(const float *gout, const float *s, const float *s_in, const float *norm,
                 const float *uvc, float *gs, float *gs_in, float *d_uvc, void *ws,
                 int64_t b0, int64_t b1, int64_t M, int D, float scale, void *stream);
/* f_sparse_op_comp as a row factor: the candidate y = s * fvec[r] is recomputed by the MixedOp epilogue (mrg_gated_branch.row_k)
 * instead of being stored.  fvec[r] = sigmoid(u.s + v.s_in + c0) * t_r is mrg_gate_fwd's factor (same expression and dot order:
 * s * fvec[r] equals its output bit for bit); hvec[r] = t_r * gate * (1 - gate).  fvec, hvec: [M]. */
int mrg_gate_row_fwd(const float *s, const float *s_in, const float *norm, const float *uvc, float *fvec, float *hvec,
                     int64_t b0, int64_t b1, int64_t M, int D, float scale, void *stream);
/* mrg_gate_row_fwd that also leaves the float64 column sums of the two MixedOp candidates that are functions of the rows it streams
 * (f_identity: s; the row factor: the float32 product s[r][c] * fvec[r]) for mrg_gated_branch.given: colsum
 * [blocks][2 (s, s * f)][2 (sum, sum of squares)][D], blocks = mrg_gate_row_colsum_blocks(b0, b1, M, D, vec4) with vec4 = (D % 4 == 0
 * and s, s_in, uvc 16-byte aligned); 0 = not available (D beyond one 16-byte step per lane: the caller keeps the statistics pass).
 * colsum_blocks: what the caller sized colsum for (MRG_E_SHAPE when the launch would write another number).  Deterministic. */
int64_t mrg_gate_row_colsum_blocks(int64_t b0, int64_t b1, int64_t M, int D, int vec4);
int mrg_gate_row_fwd_colsum(const float *s, const float *s_in, const float *norm, const float *uvc, float *fvec, float *hvec,
                            int64_t b0, int64_t b1, int64_t M, int D, float scale, void *stream, double *colsum, int64_t colsum_blocks);
/* q [M] (mrg_mix_bwd_apply's row_dq: the gradient w.r.t. fvec), dz_r = q_r * hvec[r] -> gs_in [M, D] = dz_r * v (s_in != NULL)
 * and d_uvc [3][MRG_GATE_LD(D)] for mrg_gate_param_grad3; the gradient w.r.t. s was added by the epilogue.
 * ws: mrg_gate_bwd_workspace_bytes(M, D). */
int mrg_gate_row_bwd(const float *q, const float *hvec, const float *s, const float *s_in, const float *uvc, float *gs_in, float *d_uvc,
                     void *ws, int64_t b0, int64_t b1, int64_t M, int D, void *stream);
/* The same as a member of a running gradient fan-in sum (see "gradient fan-in chain" below): gs_in = total + dz_r * v instead of
 * dz_r * v.  s_in and total [M, D] must be given; total may be gs_in itself (in place). */
int mrg_gate_row_bwd_acc(const float *q, const float *hvec, const float *s, const float *s_in, const float *uvc, float *gs_in, float *d_uvc,
                         void *ws, int64_t b0, int64_t b1, int64_t M, int D, void *stream, const float *total);

/* ---- a4 / a5 / a6: destination-segmented reducers --------------------------
 * block.update_all(fn.copy_edge('msg_e','m'), fn.max|sum|mean('m','h')) + residual
 * reference models/operations_lp.py:232-234, 247-249, 261-263  (DGL 0.5.3 gspmm).
 *
 * The in-edges of node v are eid[rowptr[v] .. rowptr[v+1]) (edge ids in the
 * caller's order, ascending).  Long lists are cut into chunks:
 *   chunk c covers CSR positions [chunk_start[c], chunk_end[c]) of node chunk_node[c];
 *   every node has >= 1 chunk (an empty one if it has no in-edge);
 *   chunk_slot[c] = -1 if the chunk is its node's whole list (result written
 *   straight to out), else the index of its partial result in the workspace;
 *   nodes with > 1 chunk are listed in hub_node[], their partial slots are
 *   hub_first[j] .. hub_first[j] + hub_count[j] - 1 (consecutive, list order).
 * out[v,:] = reduce_{e in N(v)} msg[e,:]  (+ self_rows[v,:] if not NULL); rows
 * without in-edges reduce to 0.  arg [N, D] (max only) = the lowest edge id
 * attaining the max, -1 where there is no in-edge. */
int64_t mrg_seg_reduce_workspace_bytes(int64_t n_slots, int D);
int mrg_seg_reduce_fwd(int mode, const float *msg, const float *self_rows,
                       const int32_t *eid,
                       const int32_t *chunk_node, const int32_t *chunk_start, const int32_t *chunk_end,
                       const int32_t *chunk_slot, int64_t n_chunks,
                       const int32_t *hub_node, const int32_t *hub_first, const int32_t *hub_count, int64_t n_hubs,
                       int64_t n_slots, const int32_t *in_degree,
                       float *out, int32_t *arg, void *ws,
                       int64_t N, int D, void *stream);
/* gmsg [E, D]: sum  gmsg[e] = gout[dst[e]];  mean  gout[dst[e]] / max(deg,1);
 * max  gmsg[e,c] = (arg[dst[e],c] == e) ? gout[dst[e],c] : 0.
 * gself [N, D] = gout (skipped when NULL).  relu_src [E, D] (NULL ok): the messages were ReLU
 * outputs (a_max / a_mean), gmsg is additionally zeroed where relu_src <= 0. */
int mrg_seg_reduce_bwd(int mode, const float *gout, const int32_t *dst, const int32_t *in_degree,
                       const int32_t *arg, float *gmsg, float *gself, const float *relu_src,
                       int64_t E, int64_t N, int D, void *stream);
/* The same (relu_src [E, D] or relu_bits [E, ceil(D / 32)] or neither) with the edges WALKED in destination order: order [E] = the edge
 * ids sorted by destination (the eid list of mrg_chunk_plan_build; NULL = edge-id order).  Same values; the gathered rows of the [N, D]
 * tables gout / arg are then re-used from cache by consecutive edges instead of being fetched per edge (C5: 5.05 -> see DESIGN.md). */
int mrg_seg_reduce_bwd_ordered(int mode, const float *gout, const int32_t *dst, const int32_t *in_degree, const int32_t *arg,
                               float *gmsg, float *gself, const float *relu_src, const unsigned *relu_bits, const int32_t *order,
                               int64_t E, int64_t N, int D, void *stream);
/* ABI 14.  a_max's backward without the dense input-gradient product (reference models/operations_lp.py:230-235): the gradient w.r.t.
 * the messages has one non-zero per (node, column) -- the arg-max edge, where the maximum is positive -- so
 *   gmsg[e][c] = (arg[dst[e]][c] == e && (mx == NULL || mx[dst[e]][c] > 0)) ? gout[dst[e]][c] : 0        [E, D]  (NULL: not written)
 *   gx[e][k]   = sum_c gmsg[e][c] * W[c][k]                                                             [E, Kin]
 * in ONE pass per edge row: the rows W[c, :] of the columns an edge won are added from a copy of W in LDS.  W [D, Kin] row-major must
 * fit 160 KB (mrg_segmax_bwd_input_ok); D, Kin multiples of 4, at most 256.  order: NULL or the edge ids sorted by destination.
 * Deterministic; exact f32 arithmetic. */
int mrg_segmax_bwd_input_ok(int D, int Kin);
int mrg_segmax_bwd_input(const float *gout, const float *mx, const int32_t *dst, const int32_t *arg, const float *W, float *gmsg,
                         float *gx, const int32_t *order, int64_t E, int64_t N, int D, int Kin, void *stream);
/* The same as the member of a gradient fan-in chain that closes it: gx has E + N rows (D == Kin) and leaves as
 *   gx[e]     = (gh[dst[e]] + total[e]) + sum_c gmsg[e][c] * W[c][k]      e < E
 *   gx[E + n] = (gself[n] + total[E + n]) + gout[n]                       n < N   (the aggregator's residual self rows)
 * total [E + N, Kin]: the running sum of the other readers' gradients; gh / gself [N, Kin]: a_sum's gradient left as a gather (what
 * mrg_sum_rows_gather reads; gself needs gh).  Each may be NULL: the term is left out.  The additions run in mrg_sum_rows_gather's
 * order (gather, then the buffers), so the result equals that launch over {total, this kernel's plain output} element for element
 * (up to the sign of a zero).  total may be gx itself. */
int mrg_segmax_bwd_input_chain(const float *gout, const float *mx, const int32_t *dst, const int32_t *arg, const float *W, float *gmsg,
                               float *gx, const int32_t *order, int64_t E, int64_t N, int D, int Kin, void *stream,
                               const float *total, const float *gh, const float *gself);

/* ---- a_std: destination-segmented standard deviation (ABI 19) ------------------------------------------------------------
 * The node-classification aggregator of reference models/operations.py:168-190, update_all(copy_edge, reduce_std) on a block:
 *   out[v,c] = sqrt(relu(mean_e x[e,c]^2 - (mean_e x[e,c])^2) + 1e-5)   over the in-edges e of v;  0 where v has no in-edge.
 * msg [E, D]; the chunk plan (eid, chunk_*, hub_*, n_slots, in_degree) is the one of mrg_seg_reduce_fwd; ws: at least
 * mrg_seg_std_workspace_bytes(n_slots, D) bytes when n_slots > 0.  Besides out [N, D] the forward writes, per (node, column),
 * mean [N, D] (the mean of the messages) and coef [N, D] = [u > 0] / (deg * out), u the variance before the ReLU (0 where
 * deg == 0).  Sums of x and x^2 in float64 in list order (partials of split lists added in slot order): no atomics,
 * bit-reproducible.  The backward is the exact derivative of the formula, ReLU mask included:
 *   gmsg[e,c] = gout[v,c] * coef[v,c] * (msg[e,c] - mean[v,c]),  v = dst[e]
 * one independent row per edge; order [E] (NULL: edge-id order) = the edge ids sorted by destination, the walk that keeps
 * the gathered [N, D] rows in cache.  Same D limits as mrg_seg_reduce_fwd; no host synchronisation, no allocation. */
int64_t mrg_seg_std_workspace_bytes(int64_t n_slots, int D);
int mrg_seg_std_fwd(const float *msg, const int32_t *eid, const int32_t *chunk_node, const int32_t *chunk_start,
                    const int32_t *chunk_end, const int32_t *chunk_slot, int64_t n_chunks, const int32_t *hub_node,
                    const int32_t *hub_first, const int32_t *hub_count, int64_t n_hubs, int64_t n_slots,
                    const int32_t *in_degree, float *out, float *mean, float *coef, void *ws, int64_t N, int D, void *stream);
int mrg_seg_std_bwd(const float *gout, const float *msg, const int32_t *dst, const float *mean, const float *coef,
                    const int32_t *order, float *gmsg, int64_t E, int64_t N, int D, void *stream);

/* ---- a9: fused gather -> compose -> segmented sum ------------------------------
 * CompGraphConv.forward steps 1-3, reference models/compgcn.py:58-87:
 *   g.edata['h'] = r_feats[etype] * norm;  apply_edges(u_sub_e | u_mul_e | ccorr);
 *   mask + scatter (in/out edges);  update_all(copy_e, sum)
 * (the per-direction linears W_O / W_I commute with the sum and run on the [N, D] result).
 *   out[seg,:] = sum_{e in list(seg)} combine(mode, X[xi[e],:], Y[yi[e],:], scal[e])
 * Segment lists use the chunk plan of mrg_seg_reduce_fwd (eid = element ids grouped by
 * segment; seg_len[nseg] = list lengths).  The same entry point with other index arrays is
 * the backward (segments keyed by src / by etype) and the backward of row gathers. */
int mrg_fused_gcs(int mode, const float *X, const int32_t *xi, const float *Y, const int32_t *yi,
                  const float *scal, const int32_t *eid,
                  const int32_t *chunk_node, const int32_t *chunk_start, const int32_t *chunk_end,
                  const int32_t *chunk_slot, int64_t n_chunks,
                  const int32_t *hub_node, const int32_t *hub_first, const int32_t *hub_count, int64_t n_hubs,
                  int64_t n_slots, const int32_t *seg_len,
                  float *out, void *ws, int64_t nseg, int D, void *stream);

/* Span form of the elementwise modes (SUB, MUL, COPY, NEGS) of mrg_fused_gcs: the elements are
 * pre-sorted by segment and packed as int32x4 {seg, xi, yi, float-bits of scal} in `meta` [E];
 * every lane group reduces `span` consecutive sorted elements (perfect load balance, 8 gathered
 * rows in flight).  span_slot [n_spans][2] = workspace slot of the first / last run of a span
 * when that run does not cover its whole segment (-1 otherwise); hub_* list the segments made
 * of partial runs (consecutive slots, list order) AND, with hub_count 0, the segments that have
 * no element at all, so that every row of `out` [nseg, D] is written.
 * ext_scal (NULL ok): when given, meta.w is an element index and the scale is ext_scal[meta.w]
 * (per-call scales, e.g. upstream gradients, without rebuilding the packed metadata). */
int mrg_span_gcs(int mode, const float *X, const float *Y, const void *meta, const float *ext_scal, int64_t E, int span,
                 const int32_t *span_slot, const int32_t *span_start, int64_t n_spans,
                 const int32_t *hub_seg, const int32_t *hub_first, const int32_t *hub_count, int64_t n_hubs,
                 int64_t n_slots, const int32_t *seg_len,
                 float *out, void *ws, int64_t nseg, int D, void *stream);

/* ---- gradient fan-in -------------------------------------------------------------------
 * A state read by several candidate operators (MixedOp, reference models/cell_lp.py:25-33; h_in read by
 * every MixedOp of a cell, models/cell_lp.py:150-186) receives one gradient per reader:
 *   out[i] = (accumulate ? out[i] : 0) + sum_k xs_host[k][i],  i < n,  1 <= K <= 8
 * xs_host: HOST array of K device pointers.  Order of summation k = 0..K-1. */
int mrg_sum_buffers(const float *const *xs_host, int K, float *out, int64_t n, int accumulate, void *stream);
/* out[r] = sum_k xs[k][r] + (r < E ? gather_edge[dst[r]] : gather_self[r - E]),  rows of D floats, 0 <= K <= 8.
 * The fan-in of a state read by a_sum_op (reference models/operations_lp.py:252-264) among others: a_sum's gradient w.r.t. the
 * [M, D] state is a gather of the [N, D] node gradient (edge rows: gather_edge = g * dropout mask, self rows: gather_self = g,
 * NULL = zero), so it is read from that tensor instead of from a materialised [M, D] copy. */
int mrg_sum_rows_gather(const float *const *xs_host, int K, const float *gather_edge, const float *gather_self,
                        const int32_t *dst, int64_t E, int64_t rows, int D, float *out, void *stream);

/* ---- DistMult scores (the step after the path) ---------------------------------------
 * Network.calc_score, reference models/model_search_lp.py:169-176:
 *   score[t] = sum_c ent[s_t, c] * rel[r_t, c] * ent[o_t, c]
 * without materialising the three [T, D] gathers; backward = three mrg_span_gcs (mode MUL, ext_scal = dscore). */
int mrg_distmult_score(const float *ent, const float *rel, const int32_t *s_idx, const int32_t *r_idx,
                       const int32_t *o_idx, float *score, int64_t T, int D, void *stream);

/* ---- X: MixedOp epilogue  out = sum_k w_k * ReLU(BatchNorm_k(y_k)) -----------------
 * MixedOp.forward / op_forward, reference models/cell_lp.py:25-33, with nn.BatchNorm1d in
 * training mode (:21).  K <= 8 operator outputs y_k [rows, D]; a NULL y_k is an all-zero
 * output (f_zero).  *_host arguments are HOST arrays of K DEVICE pointers.
 *   mrg_mix_colstats      sums[k][0|1][c] = sum_r y_k, sum_r y_k^2        (float64 [K][2][D])
 *   mrg_mix_finalize_fwd  coef[k][0..3] = scale (gamma*invstd), shift (beta - mean*scale),
 *                         invstd, mean*invstd; updates running_mean / running_var like torch
 *                         (momentum, unbiased variance) when their pointers are given.
 *                         `total_rows` = rows of the whole (possibly sharded) tensor.
 *   mrg_mix_fwd           out = sum_k w[k] * relu(y_k * scale_k + shift_k)
 *   mrg_mix_bwd_reduce    red[k][0] = sum_r gr, [1] = sum_r gr*xhat, [2] = sum_r g*relu(z),
 *                         gr = w[k] * g * [z > 0]                         (float32 [K][3][D])
 *   mrg_mix_finalize_bwd  coef2[k][0|1] = red[k][0|1] / total_rows; dw[k] = sum_c red[k][2][c];
 *                         optional dgamma_k = red[k][1], dbeta_k = red[k][0]
 *   mrg_mix_bwd_apply     gy_k = (gr - coef2[k][0] - xhat * coef2[k][1]) * scale_k  (NULL gy_k skipped)
 * Statistics may be all-reduced between colstats/finalize (and reduce/finalize) when rows
 * are sharded over GPUs.  Needs K*6*D*4 <= 64 KiB of LDS. */
int64_t mrg_mix_workspace_bytes(int K, int D);
/* valid_rows (ABI 15): the field of the epilogue's descriptor (mrg_gated_branch below: mrg_mix_stats_coef, mrg_mix_fwd,
 * mrg_mix_bwd_reduce, mrg_mix_bwd_apply), or the argument immediately before `stream` of the entry points without one
 * (mrg_mix_finalize_bwd, mrg_zero_stats_coef, mrg_zero_fwd, mrg_zero_bwd_reduce, mrg_zero_bwd_apply).  NULL, or a
 * DEVICE int32 [1] holding the number of valid rows of the launch -- a static step graph (round 5) padded to a host-known node
 * capacity, so that the whole search step can be replayed from ONE captured HIP graph (reference search/mr_lp_search.py:187-214,
 * utils/utils_rgcn.py:79-118).  Rows at and beyond *valid_rows are PADDING: left out of the BatchNorm statistics and of every
 * gradient reduction, not counted in the statistics' row total, and written as zeros by mrg_mix_fwd / mrg_zero_fwd and by the
 * gradient stores.  Zero rows stay zero through every operator of the search space (a zero state row yields a zero candidate), so
 * no other entry point needs the count.  The kernels read it at run time (a captured launch re-reads it on every replay).  With a
 * non-NULL valid_rows, total_rows must be the launch's own row count (`rows` where the entry point has it, a whole number in
 * mrg_mix_finalize_bwd), never a sharded total: MRG_E_SHAPE otherwise.  The colstats / mrg_mix_finalize_fwd pair takes no count
 * (mrg_mix_colstats: MRG_E_SHAPE for a descriptor that carries one): it serves the sharded path, whose row totals are host-known. */

/* ---- the step's tail: gradient clipping + SGD -------------------------------------------
 * torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.SGD(momentum, weight_decay, dampening 0, no Nesterov).step()
 * (reference search/mr_lp_search.py:118-119,243-245) over ALL parameter tensors in three launches: chunked sum of squares (double),
 * one-workgroup ordered total -> norm_coef[0] = total 2-norm, norm_coef[1] = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0),
 * then per element g = coef * grad + weight_decay * p; buf = momentum * buf + g; p -= lr * buf.
 * params / grads / bufs: DEVICE arrays of n_tensors device pointers (float32, contiguous); a null gradient pointer leaves that
 * tensor (and its momentum buffer) untouched, like torch's skip of parameters without a gradient.  Momentum buffers start at zero
 * (torch initialises buf = g on the first step: the same value).  The tensors are cut into chunks of mrg_optim_chunk() elements by
 * the caller: chunk b covers elements [chunk_off[b], chunk_off[b] + chunk_len[b]) of tensor chunk_tensor[b] (device arrays; shapes
 * never change, so they are built once).  partial: n_chunks doubles of workspace.  Deterministic.  MRG_E_NULLPTR for a missing
 * table, MRG_E_SHAPE for more than 2^31 - 1 chunks. */
int mrg_optim_chunk(void);
int mrg_clip_sgd_step(void *const *params, const void *const *grads, void *const *bufs, const int32_t *chunk_tensor,
                      const int64_t *chunk_off, const int32_t *chunk_len, int64_t n_chunks, double *partial, float *norm_coef,
                      float max_norm, float lr, float momentum, float weight_decay, void *stream);
/* ABI 21.  torch.optim.Adam(betas, eps, weight_decay, amsgrad False, maximize False).step() (the reference's architect,
 * models/architect_lp.py:20-22, and its training driver, train/mr_lp_train.py:140) over ALL tensors of a parameter list in two
 * launches, through the pointer tables and chunks of mrg_clip_sgd_step (exp_avg / exp_avg_sq: DEVICE arrays of n_tensors pointers).
 *   tick (one thread per tensor with a gradient): s = ++step[t];  scal[2t] = lr[0] / (1 - beta1^s);  scal[2t+1] = 1 / sqrt(1 - beta2^s)
 *        -- formed in double.  step [n_tensors] float32 (torch's state['step']), scal [n_tensors][2] float32, lr [1] float32: DEVICE
 *        memory, so a step captured into a HIP graph advances its own bias correction on every replay and follows a schedule.
 *   update (one chunk per workgroup): g += weight_decay * p;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *        p -= scal[2t] * m / (sqrt(v) * scal[2t+1] + eps).
 * Step counts are per tensor, as torch's are per parameter: a tensor with a null gradient pointer is left untouched -- parameter,
 * moments and count -- and lags behind the others afterwards.  A chunk whose four addresses are 16-byte aligned is read and written
 * 16 bytes per lane (pad each tensor's moment slot to a multiple of 64 elements), any other chunk and every tail 4 bytes per lane.
 * Nothing to do (n_chunks or n_tensors <= 0): MRG_OK.  MRG_E_NULLPTR, MRG_E_SHAPE (a count beyond 2^31 - 1).  Deterministic. */
int mrg_adam_step(void *const *params, const void *const *grads, void *const *exp_avg, void *const *exp_avg_sq, int64_t n_tensors,
                  const int32_t *chunk_tensor, const int64_t *chunk_off, const int32_t *chunk_len, int64_t n_chunks, float *step,
                  float *scal, const float *lr, double beta1, double beta2, float eps, float weight_decay, void *stream);
/* ABI 23 (addition).  The parameter passes of the second-order (unrolled) DARTS architect step (reference models/architect_lp.py:26-35
 * and :88-103, models/architect.py:23-32 and :84-99) over the pointer tables and chunks of mrg_clip_sgd_step.  One launch each (the
 * radius: two); the sweeps run on at most 2048 workgroups that stride over the chunks.  eta [1] float32 and scal [3] float32 are DEVICE
 * memory: nothing here needs a host value of the learning rate or of the norm.  Deterministic.  A chunk whose addresses are all 16-byte
 * aligned moves 16 bytes per lane, any other chunk (a gradient may be a contiguous view inside a larger buffer) 4 bytes per lane.
 *   mrg_unrolled_virtual_step   backup = p;  p = p - eta * (momentum * buf + (g + weight_decay * p))   -- the reference's order,
 *        `moment + dtheta`; NOT clipped (the reference's virtual step is not, even where the real step is).  bufs == NULL or a null
 *        entry: a zero moment (the reference's `except:` branch); a null gradient entry: a zero gradient.
 *   mrg_unrolled_radius         partial[b] = sum of squares of chunk b of the tensor list vecs (double; a null entry counts as zero);
 *        one workgroup folds them in fixed order:  scal = { |v|, R = r / |v|, 1 / (2 R) }.  DEPARTS from the reference, which divides
 *        by zero when |v| == 0: then R = 0 and 1 / (2 R) is stored as 0, so that the implicit term comes out as zero.  partial: n_chunks
 *        doubles.  r > 0 (MRG_E_SHAPE otherwise).
 *   mrg_unrolled_shift          p = backup + sign * R * v, R = scal[1], sign in {+1, -1, 0} (MRG_E_ENUM otherwise): always formed from
 *        backup, never accumulated; sign 0 is a plain copy (vecs and scal may be NULL), so the parameters come back bit for bit.  A
 *        null entry of vecs: p = backup.
 *   mrg_unrolled_alpha_grad     ig = (gp - gn) * scal[2];  out = dalpha - eta * ig   over the architecture parameters' own tables.  A
 *        null gp / gn entry (an alpha without a gradient) leaves out and ig untouched; a null dalpha entry counts as zero; ig may be
 *        NULL.
 * Nothing to do (n_chunks <= 0): MRG_OK (mrg_unrolled_radius still writes scal = {0, 0, 0}).  MRG_E_NULLPTR for a missing table,
 * MRG_E_SHAPE for more than 2^31 - 1 chunks. */
int mrg_unrolled_virtual_step(void *const *params, const void *const *grads, const void *const *bufs, void *const *backup,
                              const int32_t *chunk_tensor, const int64_t *chunk_off, const int32_t *chunk_len, int64_t n_chunks,
                              const float *eta, float momentum, float weight_decay, void *stream);
int mrg_unrolled_radius(const void *const *vecs, const int32_t *chunk_tensor, const int64_t *chunk_off, const int32_t *chunk_len,
                        int64_t n_chunks, double *partial, float r, float *scal, void *stream);
int mrg_unrolled_shift(void *const *params, const void *const *backup, const void *const *vecs, const int32_t *chunk_tensor,
                       const int64_t *chunk_off, const int32_t *chunk_len, int64_t n_chunks, const float *scal, int sign, void *stream);
int mrg_unrolled_alpha_grad(void *const *out, void *const *ig, const void *const *dalpha, const void *const *gp, const void *const *gn,
                            const int32_t *chunk_tensor, const int64_t *chunk_off, const int32_t *chunk_len, int64_t n_chunks,
                            const float *eta, const float *scal, void *stream);
/* `gated` (HOST pointer, NULL or k < 0 = none) of the five entry points that read the candidates: candidate k is the gated
 * filter f_dense_op_comp (reference models/operations_lp.py:356-390) and is NOT stored -- y_host[k] holds its gate
 * sigmoid(W [s ; s_in] + b) (mrg_dense_filter_fwd3 with out == NULL) and its value is recomputed wherever it is read as
 *   y_k[r][c] = gate[r][c] * s[r][c] * rowscale[r]
 * -- the expression and the order of the row GEMM's gate epilogue, so coefficients, output and gradients are those of the
 * stored form bit for bit.  rowscale covers ALL rows: the caller expands scale_edge * norm[r] on edge rows and scale_self on
 * self rows once per graph (in float32, as the epilogue multiplies them).  One [rows, D] write per MixedOp and two reads of its
 * backward less; s is the MixedOp's input state.
 * In mrg_mix_bwd_apply, when rs_on[k] == 2 for this k, fold_s[k] must be `s` and fold_gate[k] must be y_host[k]. */
#define MRG_MIX_MAX_CANDIDATES 8     /* K of the mrg_mix_* entry points is at most this */
typedef struct mrg_gated_branch {
  int32_t k;               /* the gated candidate, < 0: none */
  const float *s;          /* [rows, D] device */
  const float *rowscale;   /* [rows] device */
  /* The ROW-SCALED candidate (f_sparse_op_comp, reference models/operations_lp.py:304-343: a scalar gate per row), never stored
   * either: y_row_k[r][c] = s[r][c] * row_f[r] with row_f from mrg_gate_row_fwd (bit for bit mrg_gate_fwd's output);
   * y_host[row_k] must be `s` itself.  row_k < 0: none. */
  int32_t row_k;
  const float *row_f;      /* [rows] device */
  /* mrg_mix_bwd_apply only (the other entry points ignore them).  The candidate gets NO gradient tensor (gy_host[row_k] must be
   * NULL): with gy its gradient w.r.t. y, the kernel writes row_dq[r] = sum_c gy * s -- the gradient w.r.t. row_f[r], which
   * mrg_gate_row_bwd turns into the parameter and s_in gradients -- and, with dz_r = row_dq[r] * row_h[r], ADDS the gradient
   * w.r.t. s, gy * row_f[r] + dz_r * u_seg[c], into fold_gs[k] of the gated candidate k (required: rs_on[k] == 2; both are
   * gradients w.r.t. the rows s).
   * row_uvc: mrg_gate_collapse3's [3][row_ld] vectors; rows [0, b0) use segment 0, [b0, b1) 1, [b1, rows) 2.  D <= 256. */
  const float *row_h;      /* [rows] device */
  const float *row_uvc;
  int32_t row_ld;
  int64_t b0, b1;
  float *row_dq;           /* [rows] device, out */
  /* ABI 14: the activation behind the BatchNorm in mrg_mix_fwd / _bwd_reduce / _bwd_apply: 0 = ReLU (the MixedOp, reference
   * models/cell_lp.py:25-33), 1 = tanh (CompGraphConv's BatchNorm -> tanh tail, reference models/compgcn.py:100-111).  A descriptor
   * with k < 0 and row_k < 0 carries only this field (s may then be NULL); tanh needs exactly that (no recomputed candidate)
   * and K <= 5, else MRG_E_SHAPE. */
  int32_t act;
  /* ABI 15: the launch's device row count (valid_rows above), NULL = every row is valid.  Like act, it may be the only thing a
   * descriptor with k < 0 and row_k < 0 carries. */
  const int32_t *valid_rows;
  /* ABI 20, mrg_mix_stats_coef only (mrg_mix_colstats: MRG_E_SHAPE; the other entry points ignore them): BatchNorm sums that the
   * PRODUCER of candidate q formed while it had the values in registers (mrg_dense_filter_fwd3_colsum: f_dense_comp's and f_comp's
   * output; mrg_gate_row_fwd_colsum: s itself and s * row_f[r]).  given[q]: NULL, or given_n[q] >= 1 partial sums
   * [2][D] float64 (column sums, then column sums of squares, of the float32 values the candidate has -- all `rows` rows),
   * given_stride[q] >= 2 D doubles apart.  The statistics kernel skips such a candidate -- when every non-zero candidate is given
   * it does not run and no [rows, D] tensor is read -- and the partials are added in index order (deterministic).  Not with
   * valid_rows (MRG_E_SHAPE).  Like act, they may be all a descriptor with k < 0 and row_k < 0 carries. */
  const double *given[MRG_MIX_MAX_CANDIDATES];
  int32_t given_n[MRG_MIX_MAX_CANDIDATES];
  int64_t given_stride[MRG_MIX_MAX_CANDIDATES];
} mrg_gated_branch;
int mrg_mix_colstats(const float *const *y_host, int K, int64_t rows, int D, double *sums, void *ws,
                     const mrg_gated_branch *gated, void *stream);
int mrg_mix_finalize_fwd(const double *sums, const float *const *gamma_host, const float *const *beta_host,
                         float *const *rmean_host, float *const *rvar_host, int K, double total_rows, int D,
                         float eps, float momentum, float *coef, void *stream);
/* mrg_mix_colstats + mrg_mix_finalize_fwd in two launches instead of three (the ordered reduction of the per-block
 * statistics and the finalize step are one kernel): for callers without a collective between the two -- the single-GPU
 * step.  Bit-identical coefficients and running statistics.  ws: mrg_mix_workspace_bytes(K, D). */
int mrg_mix_stats_coef(const float *const *y, const float *const *gamma, const float *const *beta,
                       float *const *running_mean, float *const *running_var, int K, int64_t rows, double total_rows,
                       int D, float eps, float momentum, float *coef, void *ws, const mrg_gated_branch *gated, void *stream);
/* out = (addend ? addend : 0) + sum_k w[k] ReLU(y_k scale_k + shift_k).  addend (may be NULL, may NOT alias out): the output
 * of the MixedOp this one is summed with -- a state fed by several MixedOps (reference models/cell_lp.py:104-113) is
 * accumulated here instead of by separate full-size add kernels. */
int mrg_mix_fwd(const float *const *y_host, int K, const float *coef, const float *w, const float *addend, float *out,
                int64_t rows, int D, const mrg_gated_branch *gated, void *stream);
int mrg_mix_bwd_reduce(const float *g, const float *const *y_host, int K, const float *coef, const float *w,
                       float *red, void *ws, int64_t rows, int D, const mrg_gated_branch *gated, void *stream);
int mrg_mix_finalize_bwd(const float *red, int K, double total_rows, int D, float *coef2,
                         float *const *dgamma_host, float *const *dbeta_host, float *dw, const int32_t *valid_rows, void *stream);
/* rs_on (HOST int[K], may be NULL = none): candidate k's output gradient is written already multiplied by its consumer's row
 * scale, gy_k[r] *= r < rs_edge_rows[k] ? rs_scale[k] * (rs[k] ? rs[k][r] : 1) : rs_self[k] -- exactly the `dz = g * c` pass of
 * f_comp_op's backward (mrg_dense_filter_dz, kind 1), which the caller then skips (bit-identical values). */
/* rs_on[k] == 2: the gated form, mrg_dense_filter_dz kind 0 of f_dense_op_comp's backward: with gc = gy * c, gy_k receives
 * dz = gc * s * gate * (1 - gate) and fold_gs[k] the direct term gc * gate (fold_s / fold_gate / fold_gs: HOST arrays of K
 * device pointers, used for those k only). */
int mrg_mix_bwd_apply(const float *g, const float *const *y_host, float *const *gy_host, int K,
                      const float *coef, const float *coef2, const float *w, const float *const *rs, const float *rs_scale,
                      const float *rs_self, const int64_t *rs_edge_rows, const int *rs_on, const float *const *rs_full,
                      const float *const *fold_s,
                      const float *const *fold_gate, float *const *fold_gs, const int *fold_add_from, int64_t rows, int D,
                      const mrg_gated_branch *gated, void *stream);
/* rs_full (HOST array of K device pointers, NULL or NULL entries = none): candidate k's multiplier expanded over ALL rows
 * (rs_scale[k] * rs[k][r] on the edge rows, rs_self[k] on the others), which the kernel then loads with the candidates' rows
 * instead of deriving it from rs / rs_scale / rs_self / rs_edge_rows between the arithmetic and the stores. */
/* fold_add_from (HOST array of K ints, NULL = none): for a gated candidate k (rs_on[k] == 2), the index q of the candidate
 * whose OUTPUT is k's operand s (f_identity of the same MixedOp: y_host[q] == fold_s[k]); its gradient gy_q is added to
 * fold_gs[k] and gy_host[q] may be NULL -- both are gradients w.r.t. the same rows. */

/* ---- Cell zero: the MixedOp over the compose candidates, recomputed from the tables ---------------------------------------------
 * reference models/cell_lp.py:53-68 (Cell_Zero: ONE MixedOp over PRE_OPS), :25-33 (MixedOp.forward / op_forward),
 * models/operations_lp.py:71-98 (pre_mult / pre_sub / pre_add) and the gather feeding them, models/model_search_lp.py:135-145:
 *   out[r] = sum_k w[k] * ReLU(BN_k(ent[ent_idx[r]] (op_k) rel[rel_idx[r]]))          ops: MRG_COMPOSE_*, 1 <= K <= 3
 * The candidates are elementwise functions of two cache-resident table rows, so no candidate output is ever stored: the
 * statistics, combine and gradient passes recompute them, and the backward writes the two combined per-row gradients
 *   g_ent_rows[r] = sum_k gy_k * d y_k / d ent-row,   g_rel_rows[r] = sum_k gy_k * d y_k / d rel-row
 * which two mrg_span_gcs(COPY) launches turn into the table gradients.  The entry points mirror mrg_mix_colstats /
 * mrg_mix_stats_coef / mrg_mix_fwd / mrg_mix_bwd_reduce / mrg_mix_bwd_apply (same workspaces, same coef / red / coef2 layouts,
 * mrg_mix_finalize_fwd / _bwd in between, statistics may be all-reduced when the rows are sharded; ws: mrg_zero_workspace_bytes(D)).
 * Same values as the stored form; the statistics are summed over more, smaller blocks (their order differs in the last bits).  ops: HOST array of K codes. */
int64_t mrg_zero_workspace_bytes(int D);      /* ws of mrg_zero_colstats / _stats_coef / _bwd_reduce (up to 2048 blocks of partials) */
int mrg_zero_colstats(const float *ent, const float *rel, const int32_t *ent_idx, const int32_t *rel_idx, const int *ops, int K,
                      int64_t rows, int D, double *sums, void *ws, void *stream);
int mrg_zero_stats_coef(const float *ent, const float *rel, const int32_t *ent_idx, const int32_t *rel_idx, const int *ops, int K,
                        const float *const *gamma, const float *const *beta, float *const *running_mean,
                        float *const *running_var, int64_t rows, double total_rows, int D, float eps, float momentum,
                        float *coef, void *ws, const int32_t *valid_rows, void *stream);
int mrg_zero_fwd(const float *ent, const float *rel, const int32_t *ent_idx, const int32_t *rel_idx, const int *ops, int K,
                 const float *coef, const float *w, float *out, int64_t rows, int D, const int32_t *valid_rows, void *stream);
int mrg_zero_bwd_reduce(const float *g, const float *ent, const float *rel, const int32_t *ent_idx, const int32_t *rel_idx,
                        const int *ops, int K, const float *coef, const float *w, float *red, void *ws, int64_t rows, int D,
                        const int32_t *valid_rows, void *stream);
int mrg_zero_bwd_apply(const float *g, const float *ent, const float *rel, const int32_t *ent_idx, const int32_t *rel_idx,
                       const int *ops, int K, const float *coef, const float *coef2, const float *w, float *g_ent_rows,
                       float *g_rel_rows, int64_t rows, int D, const int32_t *valid_rows, void *stream);


/* ---- dense linear on edge / node rows (fp32 MFMA) ---------------------------
 * nn.Linear inside a_max_op / a_mean_op (reference models/operations_lp.py:228,231,246)
 * and the post-aggregation linears of CompGraphConv (reference models/compgcn.py:77-78,100,103).
 * Y[rows, Nout] = act(X[rows, K] W[Nout, K]^T + bias)
 *
 * Two matrix cores serve every tall-skinny product of the library (this one, mrg_linear_bwd_input,
 * mrg_dense_filter_fwd):
 *   - split core: each f32 operand is written as the sum of three bf16 numbers (error <= 2^-26 relative) and the
 *     product is accumulated in f32 from the six leading cross terms on the bf16 matrix pipe -- same error class
 *     as an f32 FMA chain (tests pin it against float64 next to the exact core), 2-3x the throughput.  Needs a
 *     workspace of mrg_gemm_workspace_bytes(K, Nout) bytes for the pre-split weight, K % 4 == 0, K > 48 and
 *     16-byte aligned rows;
 *   - exact core: v_mfma_f32_32x32x2_f32; taken when ws == NULL, the operands do not qualify, or after
 *     mrg_gemm_set_mode(1).
 * ws: NULL, or mrg_gemm_workspace_bytes(K, Nout) bytes of device memory private to this call. */
int64_t mrg_gemm_workspace_bytes(int K, int Nout);
/* 0 (default): split core where possible, on the kernel that shares the pre-split weight slabs of a 128-row workgroup through
 * LDS (two workgroups per CU); 1: exact-f32 core only; 2: split core on the wave-autonomous one-wave-per-SIMD kernel (the
 * default of rounds 1-2; also what mode 0 falls back to for operands the LDS-weight kernel does not take): a tested comparison
 * point with bit-identical results.  Modes 3 / 4 of rounds 2-3 (persistent and two-waves-per-SIMD kernels)
 * left the library in round 4 (tools/lab/).  Process-wide. */
int mrg_gemm_set_mode(int mode);
/* 1 (default): a split-core row GEMM whose output is eight 32-column tiles wide (225 .. 256 columns: D = 256) and that has no
 * direction groups, a single source and no gate epilogue runs as ONE column block (128 accumulator registers per lane, a weight ring of
 * two slabs): the activation operand is read once.  0: two four-tile column blocks (rounds 1-3).  Bit-identical.  Other values: MRG_E_ENUM.  Process-wide. */
int mrg_gemm_set_wide8(int on);
/* 1 (default, round 5): a split-core row GEMM of 129 .. 224 output columns over a reduction dimension K > 224 (D = 200: the dense
 * filters of models/operations_lp.py:266-288,356-390 forward on two operands, K = 2 D, and the paired input gradient of a MixedOp's
 * two dense candidates) whose epilogue is not a fused aggregator runs on rowgemm_x3q_k (csrc/gemm_x3q.hpp): 16 x 16 x 32 MFMA tiles,
 * 16 rows per wave, 64-row workgroups at THREE per CU.  2 (lab, tests): every K > 48.  0: rowgemm_x3s_k for all of them (rounds 3-4:
 * 32 x 32 x 16 tiles, two workgroups per CU).  Same six cross terms in the same order per accumulator; sums over k are formed 32 at a
 * time instead of 16, so the two agree to rounding (both pinned <= 1.5 x the exact-f32 core's error against float64).  Measured:
 * -5 .. -12 % per launch at K = 400, equal at K = 200 (profiles/r5_rowgemm_q.txt).  Process-wide. */
int mrg_gemm_set_q(int on);
/* ABI 14.  1 (default): split-core products of at most 16 384 rows (a sampled step graph, a rank's node chunk) run on the wave-
 * autonomous kernel with two-tile column blocks -- 3.5 x more waves with a 3.5 x shorter instruction chain each; same k-order per
 * output element, bit-identical results.  0: one kernel for every row count.  Other values: MRG_E_ENUM. */
int mrg_gemm_set_small(int on);
/* The split-core weight gradient (mrg_linear_bwd_weight / _weight3): 1 (default) = every 32-column x 16-row operand fragment is
 * split into its bf16 planes ONCE per workgroup and shared through LDS (wgrad_x3v_k), 0 = by every wave that multiplies it
 * (wgrad_x3_k, rounds 1-2).  Same operands and products in the same order: bit-identical gradients for any shape. */
int mrg_wgrad_set_variant(int variant);
int mrg_linear_fwd(const float *X, const float *W, const float *bias, float *Y, void *ws,
                   int64_t rows, int K, int Nout, int act, void *stream);
/* a_max_op.forward as ONE GEMM (reference models/operations_lp.py:230-235; SURVEY section 2b K_lin_relu_segmax):
 *   out[v] = max over in-edges e of v of ReLU(X[e] W^T + bias)  + self_rows[v]        (0 + self row without in-edge)
 * The split-core GEMM walks the edge rows in destination order (eid = the by-destination edge list of the chunk plan,
 * dst[e] = destination of edge e) and its epilogue reduces ReLU(acc + bias) over the runs of equal destination in
 * registers, publishing 64-bit atomic maxima of (value bits, 0xFFFFFFFF - list position): exact, order-independent,
 * lowest edge id among equal values (DGL's argmax).  The [E, Nout] message tensor is never written.
 * arg [N, Nout] int32 (winning edge id, -1 without in-edge) and mx [N, Nout] (the maximum itself: the backward's ReLU
 * mask is mx > 0) are optional.  ws: mrg_linear_relu_segmax_workspace_bytes(N, K, Nout) bytes; that function returns 0
 * when the split core cannot take the shape (K <= 48 or K % 4 != 0): use mrg_linear_fwd + mrg_seg_reduce_fwd then. */
int64_t mrg_linear_relu_segmax_workspace_bytes(int64_t N, int K, int Nout);
int mrg_linear_relu_segmax_fwd(const float *X, const float *W, const float *bias, const int32_t *eid, const int32_t *dst,
                               const float *self_rows, float *out, int32_t *arg, float *mx, void *ws,
                               int64_t E, int64_t N, int K, int Nout, void *stream);
/* a_mean_op.forward (reference models/operations_lp.py:245-250; SURVEY section 2b K_lin_relu_segmean) without the [E, Nout]
 * message tensor, in two launches:
 *   1. mrg_linear_relu_segsum_fwd: the split-core GEMM over the edges in destination order; its epilogue adds
 *      ReLU(X[e] W^T + bias) over the runs of equal destination inside each lane's 16 rows of a 32-row strip (a fixed
 *      order) and stores a run's sum at the position of its first row: part [E, Nout], only those "head" rows are written.
 *      relu_bits [E, ceil(Nout / 32)] keeps y > 0 per element of ORIGINAL edge row e (bit = column % 32) for the backward.
 *   2. mrg_seg_reduce_heads_fwd: out[v] = (sum of v's head rows, ascending) / max(deg, 1) + self_rows[v] (MRG_REDUCE_MEAN;
 *      MRG_REDUCE_SUM without the division) over the chunk plan; rowptr [N + 1] = list starts.  Which rows are heads
 *      follows from the list positions alone.  Deterministic: no float atomics.
 * Backward of the reducer with the bit mask: mrg_seg_reduce_bwd_bits.  Shapes as mrg_linear_relu_segmax_fwd. */
int mrg_linear_relu_segsum_fwd(const float *X, const float *W, const float *bias, const int32_t *eid, const int32_t *dst,
                               float *part, unsigned *relu_bits, void *ws, int64_t E, int K, int Nout, void *stream);
int mrg_seg_reduce_heads_fwd(int mode, const float *part, const float *self_rows, const int32_t *rowptr,
                             const int32_t *chunk_node, const int32_t *chunk_start, const int32_t *chunk_end,
                             const int32_t *chunk_slot, int64_t n_chunks, const int32_t *hub_node, const int32_t *hub_first,
                             const int32_t *hub_count, int64_t n_hubs, int64_t n_slots, const int32_t *in_degree, float *out,
                             void *ws, int64_t N, int D, void *stream);
int mrg_seg_reduce_bwd_bits(int mode, const float *gout, const int32_t *dst, const int32_t *in_degree, float *gmsg, float *gself,
                            const unsigned *relu_bits, int64_t E, int64_t N, int D, void *stream);
/* gX[rows, K] (+)= gY[rows, Nout] W[:, 0:K]   (gY already masked by the activation).  W is
 * [Nout][ldw] row-major, ldw >= K (a column block of a wider weight, e.g. one half of an
 * nn.Linear(2D, D)); accumulate != 0 adds into gX.  ws (mandatory) holds the split / transposed block. */
int64_t mrg_linear_bwd_input_workspace_bytes(int K, int Nout);
int mrg_linear_bwd_input(const float *gY, const float *W, float *gX, void *ws,
                         int64_t rows, int K, int Nout, int ldw, int accumulate, void *stream);
/* Gradient fan-in chain.  A tensor with several readers receives the sum of their gradients; instead of one [rows, K] tensor per
 * reader and a K-way pass (mrg_sum_buffers), every reader but the first adds the running sum `total` [rows, K] in the store of
 * its own last kernel.  For the input-gradient GEMMs (this one, mrg_linear_bwd_input3 and mrg_linear_bwd_input3_pair):
 *   accumulate != 0:  gX = (gY W[:, 0:K] + gX) + total     (an epilogue kind of its own; total must not be gX)
 *   accumulate == 0:  gX = gY W[:, 0:K] + total            (total may be gX: in place)
 * i.e. what the plain call followed by mrg_sum_buffers({its output, total}) leaves, element for element (up to the sign of a zero). */
int mrg_linear_bwd_input_acc2(const float *gY, const float *W, float *gX, void *ws,
                              int64_t rows, int K, int Nout, int ldw, int accumulate, void *stream, const float *total);
/* gW[Nout, K1+K2] = gY^T [X1 | X2]  (X2 NULL / K2 = 0: single source; the reference's
 * torch.cat([s, s_in], 1) is never materialised),  gbias[Nout] = column sums of gY (NULL ok). */
int64_t mrg_linear_bwd_weight_workspace_bytes(int64_t rows, int K, int Nout);
int mrg_linear_bwd_weight(const float *gY, const float *X1, const float *X2, float *gW, float *gbias, void *ws,
                          int64_t rows, int K1, int K2, int Nout, void *stream);
/* ABI 15.  mrg_linear_bwd_weight for ONE of `share` ranges of a grouped launch being reproduced range by range: share 1 = the range
 * runs alone (mrg_linear_bwd_weight itself); 2..3 = mrg_linear_bwd_weight3 sized the row blocks of that many ranges so that they
 * TOGETHER get about one workgroup per CU, and this launch uses the same row blocks -- the SAME partial sums, bit for bit.  Else
 * MRG_E_ENUM.  Same workspace (mrg_linear_bwd_weight_workspace_bytes does not depend on share). */
int mrg_linear_bwd_weight_share(const float *gY, const float *X1, const float *X2, float *gW, float *gbias, void *ws,
                                int64_t rows, int K1, int K2, int Nout, int share, void *stream);

/* ---- dense (per-feature) filters, one direction segment per call ------------------
 * f_dense_op_comp / f_comp_op / f_dense_op_last / f_dense_op .forward,
 * reference models/operations_lp.py:356-390, 266-288, 392-401, 345-354.
 *   z = [s | s_in] W^T + bias        (s_in NULL: z = s W^T + bias; W is [D, 2D] or [D, D])
 *   kind 0:  out = sigmoid(z) * s * c      (gate [rows, D] receives sigmoid(z) for the backward)
 *   kind 1:  out = z * c
 *   c = scale * (rowscale ? rowscale[row] : 1)     (the reference's 1/3 and edge norm)
 * torch.cat([s, s_in], 1) is never materialised: the GEMM reads both sources; gate, scale and
 * norm are applied in its epilogue.  ws: NULL or mrg_gemm_workspace_bytes(K, D) bytes, K = D or 2D (see mrg_linear_fwd). */
int mrg_dense_filter_fwd(int kind, const float *s, const float *s_in, const float *W, const float *bias,
                         const float *rowscale, float scale, float *out, float *gate, void *ws,
                         int64_t rows, int D, void *stream);
/* The three direction segments of one dense filter in ONE launch each (weight split + grouped row GEMM) instead of three:
 * rows [0, b0) use W[0] / bias[0], [b0, b1) W[1] / bias[1] (edge rows: c = scale_edge * norm[row]), [b1, M) W[2] / bias[2]
 * (self rows: c = scale_self).  W / bias: HOST arrays of three device pointers (bias entries may be NULL).  Split core
 * only: mrg_dense_filter3_workspace_bytes(D, K) returns 0 when the shape does not qualify (then use the per-segment
 * entry point).  Same arithmetic per row as mrg_dense_filter_fwd: results are bit-identical.
 * kind 0 with out == NULL: only the gate is stored; the MixedOp epilogue recomputes the output (mrg_gated_branch). */
int64_t mrg_dense_filter3_workspace_bytes(int D, int K);
int mrg_dense_filter_fwd3(int kind, const float *s, const float *s_in, const float *const *W, const float *const *bias,
                          const float *norm, float scale_edge, float scale_self, float *out, float *gate, void *ws,
                          int64_t b0, int64_t b1, int64_t M, int D, void *stream);
/* mrg_dense_filter_fwd3 that also leaves the float64 column sums of its output (kind 0: of gate * s * c, whether out is stored or
 * not -- then the multiplicand s is read by the epilogue) for mrg_gated_branch.given: colsum [blocks][2 (sum, sum of squares)][D],
 * one partial per workgroup, added inside the workgroup in a fixed order (no atomics).  blocks =
 * mrg_dense_filter3_colsum_blocks(kind, b0, b1, M, D, K); 0 = the kernel this launch would take has no such form (exact-f32 core,
 * few rows, D outside 132..224): the caller keeps the statistics pass.  colsum_blocks: what the
 * caller sized colsum for (MRG_E_SHAPE when the launch would write another number). */
int64_t mrg_dense_filter3_colsum_blocks(int kind, int64_t b0, int64_t b1, int64_t M, int D, int K);
int mrg_dense_filter_fwd3_colsum(int kind, const float *s, const float *s_in, const float *const *W, const float *const *bias,
                                 const float *norm, float scale_edge, float scale_self, float *out, float *gate, void *ws,
                                 int64_t b0, int64_t b1, int64_t M, int D, void *stream, double *colsum, int64_t colsum_blocks);
/* dz (and the direct term of gs) for all M rows of the three segments in one launch: rows [0, b1) c = scale_edge * norm[row],
 * rows [b1, M) c = scale_self (see mrg_dense_filter_dz). */
int mrg_dense_filter_dz3(int kind, const float *g, const float *s, const float *gate, const float *norm, float scale_edge,
                         float scale_self, float *dz, float *gs, int64_t b1, int64_t M, int D, void *stream);
/* mrg_linear_bwd_input / mrg_linear_bwd_weight for the three row ranges [0, b0) [b0, b1) [b1, M) with their own weights
 * W[0..2] (HOST array of device pointers, each [Nout][ldw]) in one launch each.  The *_workspace_bytes queries return 0
 * when the split core cannot take the shape or mrg_gemm_set_mode(1) is active: use the per-range entry points then. */
int64_t mrg_linear_bwd_input3_workspace_bytes(int K, int Nout);
int mrg_linear_bwd_input3(const float *gY, const float *const *W, float *gX, void *ws, int64_t b0, int64_t b1, int64_t M,
                          int K, int Nout, int ldw, int accumulate, void *stream);
/* The input gradient of TWO candidates that read the same rows as one product over the concatenated reduction dimension:
 * gX rows of range s (+)= [gY1 | gY2] [W1[s][:, 0:K] ; W2[s][:, 0:K]] -- f_dense_comp and f_comp of one MixedOp (reference
 * models/cell_lp.py:95-113; models/operations_lp.py:266-288, 356-390) leave ONE gradient w.r.t. their shared operand instead
 * of two that a fan-in pass would add.  gY1, gY2: [M, Nout]; W1, W2: HOST arrays of three device pointers, each [Nout][ldw].
 * Split core only (the workspace query returns 0 otherwise). */
int64_t mrg_linear_bwd_input3_pair_workspace_bytes(int K, int Nout);
int mrg_linear_bwd_input3_pair(const float *gY1, const float *gY2, const float *const *W1, const float *const *W2, float *gX,
                               void *ws, int64_t b0, int64_t b1, int64_t M, int K, int Nout, int ldw, int accumulate,
                               void *stream);
/* The two grouped input gradients joined to a running gradient fan-in sum (see mrg_linear_bwd_input_acc2); same workspaces. */
int mrg_linear_bwd_input3_acc2(const float *gY, const float *const *W, float *gX, void *ws, int64_t b0, int64_t b1, int64_t M,
                               int K, int Nout, int ldw, int accumulate, void *stream, const float *total);
int mrg_linear_bwd_input3_pair_acc2(const float *gY1, const float *gY2, const float *const *W1, const float *const *W2, float *gX,
                                    void *ws, int64_t b0, int64_t b1, int64_t M, int K, int Nout, int ldw, int accumulate,
                                    void *stream, const float *total);
int64_t mrg_linear_bwd_weight3_workspace_bytes(int64_t b0, int64_t b1, int64_t M, int K1, int K2, int Nout);
int mrg_linear_bwd_weight3(const float *gY, const float *X1, const float *X2, float *const *gW, float *const *gbias, void *ws,
                           int64_t b0, int64_t b1, int64_t M, int K1, int K2, int Nout, void *stream);
/* backward, step 1:  kind 0: dz = g*s*c*gate*(1-gate), gs = g*c*gate (direct term);  kind 1: dz = g*c.
 * Steps 2-3 are mrg_linear_bwd_input (gs += dz W[:, :D]; gs_in = dz W[:, D:]) and
 * mrg_linear_bwd_weight (gW = dz^T [s | s_in], gbias = column sums of dz). */
int mrg_dense_filter_dz(int kind, const float *g, const float *s, const float *gate, const float *rowscale,
                        float scale, float *dz, float *gs, int64_t rows, int D, void *stream);

/* ---- f2: graph construction, edge ordering and index plans on the device ------------------
 * build_graph_from_triplets + comp_deg_norm  reference utils/utils_rgcn.py:120-158
 * node_norm_to_edge_norm                     reference search/mr_lp_search.py:30-36
 * build_graph                                reference train/mr_lp_train.py:77-89
 * Integer work: bit-exact with the reference's numpy formulation.
 *
 * mrg_build_graph: triples [T][3] int64 (s, r, o) -> E = 2T directed edges (e < T: s -> o with relation r; e >= T:
 * o -> s with r + R).  sorted != 0: edges ordered by (relation, dst, src) like `sorted(zip(rel, dst, src))`
 * (utils_rgcn.py:151); sorted == 0: the train driver's un-sorted halves.  in_degree [N] counts edges per destination.
 * norm[e] = deg_norm_table[in_degree[dst]] * deg_norm_table[in_degree[src]] where the HOST supplies
 * deg_norm_table[d] = float32(d) ** float32(-0.5), 0 for d = 0 (numpy's own values: a device pow / rsqrt may differ
 * in the last bit); the caller must make table_len exceed the largest in-degree (max_degree [1] reports it).
 * src32 / dst32 / etype32 (NULL ok): int32 copies for the kernels.  norm NULL skips the norm (and the int32 copies). */
int64_t mrg_build_graph_workspace_bytes(int64_t T);
int mrg_build_graph(const int64_t *triples, int64_t T, int64_t N, int R, int sorted,
                    const float *deg_norm_table, int64_t table_len,
                    int64_t *src, int64_t *dst, int64_t *etype, float *norm, int32_t *in_degree,
                    int32_t *src32, int32_t *dst32, int32_t *etype32, int32_t *max_degree,
                    void *ws, int64_t ws_bytes, void *stream);

/* Span plan of mrg_span_gcs for segment ids seg [E] in [0, nseg): perm [E] = stable argsort, seg_sorted [E],
 * seg_len [nseg], span_slot [2 * n_spans] (n_spans = ceil(E / span)), hub_seg / hub_first / hub_count with capacity
 * 2 * n_spans + nseg, counts [2] = {n_hubs, n_slots} (device memory; the host reads it once).  Same results as the
 * tensor formulation it replaces (mr-gnas_amd/graph.py:span_plan), which stays as the test's cross-check. */
int64_t mrg_plan_workspace_bytes(int64_t E, int64_t nseg, int span);
int mrg_span_plan_build(const int32_t *seg, int64_t E, int64_t nseg, int span, int snap,
                        int32_t *perm, int32_t *seg_sorted, int32_t *seg_len, int32_t *span_slot, int32_t *span_start,
                        int32_t *hub_seg, int32_t *hub_first, int32_t *hub_count, int32_t *counts,
                        void *ws, int64_t ws_bytes, void *stream);
/* span_start [n_spans + 1] (ABI 8): span i covers sorted elements [span_start[i], span_start[i + 1]).  A cut is nominally
 * i * span; where that position falls inside a segment it moves to the nearer end of that segment if that is at most `snap`
 * (0 .. span / 4; 0 = fixed spans) elements away, so segments up to 2 * snap long are never split over spans (no partial runs,
 * workspace slots or hub-pass work for them) and every span stays within +- 2 * snap of the nominal length.  The last span may
 * be empty. */
/* meta[j] = {seg_sorted[j], xi[perm[j]] (perm[j] if xi NULL), yi[perm[j]] (0 if NULL), w} with w = float bits of
 * scal[perm[j]] (1.0f if scal NULL), or perm[j] itself when w_is_index != 0 (external per-call scales). */
int mrg_span_meta_pack(const int32_t *perm, const int32_t *seg_sorted, const int32_t *xi, const int32_t *yi,
                       const float *scal, int w_is_index, void *meta, int64_t E, void *stream);

/* Chunk plan of mrg_seg_reduce_fwd / mrg_fused_gcs (CSR by destination, lists cut into chunks of `chunk`):
 * eid [E], rowptr [N + 1], in_degree [N], chunk_* with capacity N + E / chunk + 1, hub_* with capacity
 * E / chunk + 1, counts [3] = {n_chunks, n_hubs, n_slots}. */
int64_t mrg_chunk_plan_workspace_bytes(int64_t E, int64_t N);
int mrg_chunk_plan_build(const int32_t *dst, int64_t E, int64_t N, int chunk,
                         int32_t *eid, int32_t *rowptr, int32_t *in_degree,
                         int32_t *chunk_node, int32_t *chunk_start, int32_t *chunk_end, int32_t *chunk_slot,
                         int32_t *hub_node, int32_t *hub_first, int32_t *hub_count, int32_t *counts,
                         void *ws, int64_t ws_bytes, void *stream);

/* ---- f4: sampling-side data preparation on the device ----------------------------------------
 * Random draws are inputs (the host draws them on the device; tests replay numpy's), so each call is deterministic and
 * bit-exact with the reference for the same draws.
 *
 * negative_sampling, reference utils/utils_rgcn.py:191-204: samples [(rate+1) B][3]: rows [0, B) = pos (label 1), row
 * B + j = pos[j % B] with the subject (choices[j] > 0.5) or the object replaced by values[j] (label 0). */
int mrg_negative_sampling(const int64_t *pos, int64_t B, int rate, const int64_t *values, const double *choices,
                          int64_t *samples, float *labels, void *stream);
/* `uniq_v, edges = np.unique((src, dst), return_inverse=True)`, reference utils/utils_rgcn.py:97-101: uniq [<= min(2n,
 * num_nodes)] = the distinct node ids in ascending order, new_src / new_dst their ranks, count [1] (device) = len(uniq). */
/* sample_edge_neighborhood (reference utils/utils_rgcn.py:30-71; `--edge_sampler neighbor`, search/mr_lp_search.py:323-324):
 * sample_size dependent picks by neighbourhood expansion in ONE launch of one persistent workgroup.  Adjacency in the
 * reference's append order (get_adj_and_degrees, :18-28) as a CSR: rowptr [N + 1], adj_edge / adj_other [2 T] (triple id and the
 * vertex at its other end), degrees [N].  Draws are inputs: u_vertex [sample_size] float64 uniforms for the vertex picks
 * (inverse cdf over sample_counts * seen), and EITHER tries [n_tries] -- the reference's own sequence of tried adjacency slots,
 * rejected ones included (replay: bit-exact) -- OR u_edge [sample_size] float64 uniforms (one draw per pick selects uniformly
 * among the vertex's unpicked entries: the reference's distribution without its rejection loop).  edges [sample_size] int32.
 * status [3] int64: picks made, tries consumed, failure code (0 ok; 1 graph exhausted; 2 / 3 bad or missing tries).
 * ws: mrg_sample_neighborhood_workspace_bytes(N, T). */
int64_t mrg_sample_neighborhood_workspace_bytes(int64_t N, int64_t T);
int mrg_sample_edge_neighborhood(const int32_t *rowptr, const int32_t *adj_edge, const int32_t *adj_other, const int32_t *degrees,
                                 int64_t N, int64_t T, int64_t sample_size, const double *u_vertex, const int64_t *tries,
                                 int64_t n_tries, const double *u_edge, int32_t *edges, int64_t *status, void *ws,
                                 int64_t ws_bytes, void *stream);
int64_t mrg_relabel_workspace_bytes(int64_t num_nodes);
int mrg_relabel_nodes(const int64_t *src, const int64_t *dst, int64_t n, int64_t num_nodes, int64_t *uniq,
                      int64_t *new_src, int64_t *new_dst, int32_t *count, void *ws, int64_t ws_bytes, void *stream);
/* Dense targets of a (subject, relation) batch: process() + TrainDataset / TestDataset.get_label (+ label smoothing),
 * reference utils/process_data.py:4-31, utils/data_set.py:15-33.  keys [U] ascending = subject * (2R) + relation of the
 * known pairs, rowptr [U + 1] / objs = their object lists; out [B][num_ent] = v_zero everywhere, v_one at the objects of
 * query[b] (a query without a list gives an all-v_zero row). */
int mrg_multi_hot_labels(const int64_t *keys, const int32_t *rowptr, const int32_t *objs, const int64_t *query,
                         int64_t B, int64_t U, int64_t num_ent, float v_zero, float v_one, float *out, void *stream);

/* ---- node-classification blocks with per-layer fan-outs (sampler.NeighborSampler, csrc/blocks.hip) ------------------
 * One layer of one minibatch from a RESIDENT in-edge index of the graph: rowptr [N + 1] over destinations, in_eid / in_src /
 * in_type [E_graph] = edge id, global source and type of the in-edges in stable destination order (edge ids ascending inside a
 * destination; in_type may be NULL with etype NULL).  dst_nodes [n_dst] int64: the layer's destinations (unique; an id outside
 * [0, N) has no edges and is never used as an index).  k: the fan-out, 0 = every in-edge, else 1..64 (another k: MRG_E_SHAPE).
 * No launch or memset of these entry points grows with N or E_graph: the work is O(n_dst max(k, 1) + E).
 *   mrg_block_sizes: first [n_dst + 1] = exclusive sums of cnt[i] = min(deg(dst_nodes[i]), k) (deg when k == 0);
 *     first[n_dst] = E, which the caller reads.  ws: mrg_block_sizes_workspace_bytes(n_dst).
 *   mrg_block_emit: the block's E edges, grouped by destination in destination order, edge ids ascending inside one: eid / etype /
 *     ldst [E] int64 (etype may be NULL), gsrc [E] int32 = the global sources.  A destination with deg <= k (or k == 0) keeps its
 *     whole in-list; one with deg > k keeps the k positions that Floyd's algorithm picks from its row of u [n_dst][k] (float64 in
 *     [0, 1)): for i = 0 .. k - 1, j = deg - k + i, t = min(floor(u_i (j + 1)), j), pick j if t is already picked, else t.
 *     Also enters the layer into the tables: local[dst_nodes[i]] = i, firstpos[s] = the lowest block edge with source s.
 *   mrg_block_relabel: src_nodes [n_dst + E] int64 = dst_nodes, then the n_new sources that are no destination in the order of
 *     their first edge (entries past n_dst + n_new are not written); lsrc [E] int64 = every edge's index into it; n_new [1]
 *     (device).  Restores both tables at the entries mrg_block_emit touched.  ws: mrg_block_relabel_workspace_bytes(E).
 * local / firstpos [N] int32 are the caller's: -1 / INT32_MAX everywhere before mrg_block_emit and again after mrg_block_relabel;
 * the three calls of a layer go to ONE stream, in this order, and one pair of tables serves one stream at a time.
 * n_dst == 0 or E == 0: MRG_OK, nothing launched (and the tables untouched).  Integer atomics only; deterministic.
 * MRG_E_NULLPTR, MRG_E_SHAPE (a negative size, k outside 0..64, n_dst + E beyond 2^31 - 2), MRG_E_WORKSPACE. */
int64_t mrg_block_sizes_workspace_bytes(int64_t n_dst);
int mrg_block_sizes(const int32_t *rowptr, const int64_t *dst_nodes, int64_t n_dst, int64_t N, int k, int32_t *first, void *ws,
                    int64_t ws_bytes, void *stream);
int mrg_block_emit(const int32_t *rowptr, const int32_t *in_eid, const int32_t *in_src, const int32_t *in_type,
                   const int64_t *dst_nodes, const int32_t *first, int64_t n_dst, int64_t N, int k, const double *u, int64_t E,
                   int64_t *eid, int64_t *etype, int64_t *ldst, int32_t *gsrc, int32_t *local, int32_t *firstpos, void *stream);
int64_t mrg_block_relabel_workspace_bytes(int64_t E);
int mrg_block_relabel(const int32_t *gsrc, const int64_t *dst_nodes, int64_t n_dst, int64_t N, int64_t E, int32_t *local,
                      int32_t *firstpos, int64_t *src_nodes, int64_t *lsrc, int32_t *n_new, void *ws, int64_t ws_bytes, void *stream);

/* The same blocks with one fan-out PER EDGE TYPE (csrc/blocks_rel.hip; sampler.NeighborSampler with a per-relation layer).  A run
 * (v, r) is the in-edges of destination v with type r in ascending edge id.  The resident index: rel_eid [E_graph] int32 = the edge
 * ids in stable (destination, type, edge id) order; run_ptr [N + 1] = the number of runs before every destination; run_start
 * [n_runs + 1] = every run's first position in rel_eid, then E_graph; run_type [n_runs]; src_of / type_of [E_graph] int32 = the
 * graph's sources and types by edge id (type_of may be NULL with etype NULL).
 * The specification comes twice and the two must agree: fan_host [R] in HOST memory (checked before any launch) and spec [2 R] on
 * the device = the same R entries, then every type's first column in a row of u.  An entry is -1 (every in-edge of the type), 0
 * (none) or 1..64 (another value: MRG_E_SHAPE); K = the sum of the entries >= 1 (another K: MRG_E_SHAPE); u [n_dst][K] float64 in
 * [0, 1) (may be NULL when K == 0).  Of a run of length d with entry f a destination keeps nothing (f == 0), all of it (f == -1 or
 * d <= f) or the f positions of the run that Floyd's algorithm (mrg_block_emit) picks from u[i][col_r .. col_r + f).
 *   mrg_block_rel_sizes: first [n_dst + 1] = exclusive sums of the kept edges per destination; first[n_dst] = E.
 *     ws: mrg_block_rel_sizes_workspace_bytes(n_dst) (the scan's temporary storage and the n_dst + 1 counts).
 *   mrg_block_rel_emit: the block's E edges with mrg_block_emit's outputs and conventions -- grouped by destination, edge ids
 *     ascending inside one ACROSS the types -- and the layer entered into local / firstpos; mrg_block_relabel follows, unchanged.
 *     ws: mrg_block_rel_emit_workspace_bytes(E) (two key buffers and the temporary storage of a key sort over E items).
 * No launch, memset or work item of these entry points grows with N or E_graph.  n_dst == 0 or E == 0: MRG_OK, nothing launched.
 * Integer atomics only; deterministic.  MRG_E_NULLPTR, MRG_E_SHAPE (a negative size, R < 1, a bad entry or K), MRG_E_WORKSPACE. */
int64_t mrg_block_rel_sizes_workspace_bytes(int64_t n_dst);
int mrg_block_rel_sizes(const int32_t *run_ptr, const int32_t *run_start, const int32_t *run_type, const int64_t *dst_nodes,
                        int64_t n_dst, int64_t N, const int32_t *fan_host, const int32_t *spec, int R, int32_t *first, void *ws,
                        int64_t ws_bytes, void *stream);
int64_t mrg_block_rel_emit_workspace_bytes(int64_t E);
int mrg_block_rel_emit(const int32_t *run_ptr, const int32_t *run_start, const int32_t *run_type, const int32_t *rel_eid,
                       const int32_t *src_of, const int32_t *type_of, int64_t E_graph, const int64_t *dst_nodes,
                       const int32_t *first, int64_t n_dst, int64_t N, const int32_t *fan_host, const int32_t *spec, int R,
                       const double *u, int64_t K, int64_t E, int64_t *eid, int64_t *etype, int64_t *ldst, int32_t *gsrc,
                       int32_t *local, int32_t *firstpos, void *ws, int64_t ws_bytes, void *stream);

/* ---- f3: filtered ranking and the [B, N] score functions ---------------------------------------------
 * predict(), reference train/mr_lp_train.py:290-299: entries with a non-zero label are pushed to -1e7, the target keeps
 * its score; ranks[b] = 1 + #(greater) + #(equal at a lower index)  (the position in a stable descending sort). */
int mrg_rank_filtered(const float *pred, const float *labels, const int64_t *obj, int64_t B, int64_t N,
                      int64_t *ranks, void *stream);
/* calc_mrr, reference utils/utils_rgcn.py:212-380 (perturb_and_get_raw_rank / perturb_*_and_get_filtered_rank): ranks of Q DistMult
 * queries against all N entities with no [Q, N] tensor in memory.  Query i fixes entity a_idx[i] and relation r_idx[i]; candidate e
 * scores x_e = sum_c ent[a, c] * rel[r, c] * ent[e, c] (the reference ranks sigmoid(x): monotone, and where float32 sigmoid saturates
 * and the reference's sort order among ties is unspecified, this value lies inside its tie interval);
 *   ranks[i] = 1 + #(x_e > x_t) + #(x_e == x_t, e < t)   over candidates e != t = t_idx[i] that are not filtered
 * (the rule of mrg_rank_filtered).  Filter: the list of key qkey[i] (-1 or an unknown key: none) in the index keys [U] ascending /
 * rowptr [U + 1] / members (entity ids, ascending inside a list) / gone_at; member j is filtered iff gone_at[j] > when[i].  The reference's
 * protocol removes a test triple from its filter set for good when it is queried (gone_at = index of the first equal test triple,
 * when = i for the subject pass, T for the object pass); when = -1 with gone_at >= 0 is the standard protocol.  The index arguments
 * may all be NULL with U == 0 (raw ranks).  One decision per (query, candidate), taken on the accumulator that is compared; the
 * target's score is formed by the sweep's own tile routine, so a duplicate of the target's row ties exactly.  Counts are integer
 * atomics: deterministic.  Split-bf16 core for D > 48 with D % 4 == 0 (error class of mrg_linear_fwd), else the exact-f32 core.
 * Indices are trusted (0 <= a, t < N; 0 <= r < rows of rel; members < N).  Workspace: O(N D + min(Q, 8192) D + Q) bytes.
 * Argument errors are returned before any HIP call; Q == 0 returns MRG_OK with nothing launched. */
int64_t mrg_distmult_rank_workspace_bytes(int64_t Q, int64_t N, int D);
int mrg_distmult_rank(const float *ent, const float *rel, const int32_t *a_idx, const int32_t *r_idx, const int32_t *t_idx,
                      const int64_t *qkey, const int32_t *when, const int64_t *keys, const int32_t *rowptr, const int32_t *members,
                      const int32_t *gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t *ranks, void *ws, int64_t ws_bytes,
                      void *stream);
/* The fixed-genotype driver's 1-N training loss (reference train/mr_lp_train.py Network._loss: BCELoss over sf_DisMult_op's [B, N]
 * predictions and the label-smoothed multi-hot labels of utils/data_set.py:21-33) with no [B, N] tensor in memory.  Additive: ABI 23.
 *   x[b, e] = sum_c q[b, c] * ent[e, c]   (q [B, D] = ent[subj] * rel_emb[rel], materialised by the caller),  p = sigmoid(x) in float32
 *   y[b, e] = v_one if e is in the list of key qkey[b] (= subj * 2R + rel) in the index keys [U] ascending / rowptr [U + 1] / objs
 *             (entity ids, ascending inside a list: sampler.LabelIndex), else v_zero; an unknown key has an empty list
 * mrg_distmult_bce_fwd:    loss[0] (float32, device) = mean over b, e of (y - 1) * max(log1p(-p), -100) - y * max(log p, -100): torch's
 *   binary_cross_entropy term for term (p == 1 gives 100 (1 - y), p == 0 gives 100 y), summed in float64 -- lane, wave, workgroup, then
 *   one float64 partial per workgroup added in a fixed order: no float atomics, bitwise repeatable.
 * mrg_distmult_bce_dlogit: dl [B][c1 - c0] = gscale[0] * (p - y) * (p (1 - p) / max(p (1 - p), 1e-12)) for the entities [c0, c1): torch's
 *   binary_cross_entropy_backward times sigmoid_backward, exactly 0 where p saturates.  gscale: one float on the device, the upstream
 *   gradient divided by B * N (no host synchronisation).
 * Both recompute the product as the row GEMM of mrg_distmult_rank: split-bf16 core for D > 48 with D % 4 == 0 (error class of
 * mrg_linear_fwd), else the exact-f32 core.  Indices are trusted (objs < N).  Workspace: mrg_distmult_bce_workspace_bytes(B, N, D) for the
 * forward and (B, c1 - c0, D) for the logit gradient, O(min(columns, 28 672) D + B + B columns / 28 672) bytes.  Argument errors are
 * returned before any HIP call; B == 0 returns MRG_OK with nothing launched; N is bounded as for mrg_distmult_rank. */
int64_t mrg_distmult_bce_workspace_bytes(int64_t B, int64_t N, int D);
int mrg_distmult_bce_fwd(const float *q, const float *ent, const int64_t *qkey, const int64_t *keys, const int32_t *rowptr,
                         const int32_t *objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D, float *loss,
                         void *ws, int64_t ws_bytes, void *stream);
int mrg_distmult_bce_dlogit(const float *q, const float *ent, const int64_t *qkey, const int64_t *keys, const int32_t *rowptr,
                            const int32_t *objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D, int64_t c0,
                            int64_t c1, const float *gscale, float *dl, void *ws, int64_t ws_bytes, void *stream);
/* mrg_distmult_rank for query rows the caller already holds (q [Q][D]: DistMult's ent[a] * rel[r], ConvE's hidden vector after BN2 + ReLU):
 * candidate e scores x_e = sum_c q[i, c] * ent[e, c]; everything else -- target rows gathered, rule, filter, cores, workspace
 * (mrg_distmult_rank_workspace_bytes), errors -- is mrg_distmult_rank's.  Rows that are not 16-byte aligned run the exact-f32 core.
 * Additive: ABI 23. */
int mrg_rows_rank(const float *q, const float *ent, const int32_t *t_idx, const int64_t *qkey, const int32_t *when, const int64_t *keys,
                  const int32_t *rowptr, const int32_t *members, const int32_t *gone_at, int64_t U, int64_t Q, int64_t N, int D,
                  int64_t *ranks, void *ws, int64_t ws_bytes, void *stream);
/* The 1-N loss, its logit gradient and the filtered ranks of sf_TransE_op without a [B, N] tensor (csrc/transe_1n.hip).  Additive: ABI 23.
 *   dist[b, e] = sum_c |obj[b, c] - ent[e, c]|  (obj [B][D] = sub + rel in float32, formed by the caller),  x = gamma - dist,
 *   p = sigmoid(x) in float32.  Every distance is one float32 accumulator over c ascending: bit-identical with mrg_transe_score_fwd's.
 * mrg_transe_bce_fwd / mrg_transe_bce_dlogit: mrg_distmult_bce_fwd / _dlogit on this x -- same labels (index keys / rowptr / objs, key
 *   qkey[b]), same terms, same saturation, float64 partials per workgroup added in a fixed order (bitwise repeatable), gscale on the
 *   device.  Workspace: mrg_transe_bce_workspace_bytes(B, N, D) for the forward and (B, c1 - c0, D) for the logit gradient: two integers
 *   per query and one float64 per tile of 64 x 64 elements.
 * mrg_transe_dist_bwd: the gradients that one slice dl [B][nc] (leading dimension ld >= nc) of the loss gradient with respect to x
 *   contributes, for the nc entity rows at ent_c: d loss / d dist = -dl,
 *     gobj[b, c]   (+)= sum_e (-dl[b, e]) * sgn(obj[b, c] - ent_c[e, c])      (accumulate != 0: added to gobj)
 *     gent_c[e, c]   = -sum_b (-dl[b, e]) * sgn(obj[b, c] - ent_c[e, c])      sgn(0) = 0
 *   either output may be NULL.  Sums in a fixed order.
 * mrg_transe_rank: ranks[i] = 1 + #(dist_e < dist_t) + #(dist_e == dist_t, e < t) over candidates e != t = t_idx[i] that are not filtered:
 *   mrg_distmult_rank's rule on the score gamma - dist and its filter (index, gone_at > when), compared on dist itself; the target's
 *   distance is formed by the same float32 chain, so a duplicate of the target's row ties exactly.  Integer atomics only.
 *   Workspace: mrg_transe_rank_workspace_bytes(Q, N, D), O(Q) bytes.
 * 1 <= D <= 1024, N bounded as for mrg_distmult_rank; indices are trusted.  Argument errors are returned before any HIP call; B == 0 /
 * Q == 0 returns MRG_OK with nothing launched. */
int64_t mrg_transe_bce_workspace_bytes(int64_t B, int64_t ncols, int D);
int mrg_transe_bce_fwd(const float *obj, const float *ent, const int64_t *qkey, const int64_t *keys, const int32_t *rowptr,
                       const int32_t *objs, int64_t U, float gamma, float v_zero, float v_one, int64_t B, int64_t N, int D, float *loss,
                       void *ws, int64_t ws_bytes, void *stream);
int mrg_transe_bce_dlogit(const float *obj, const float *ent, const int64_t *qkey, const int64_t *keys, const int32_t *rowptr,
                          const int32_t *objs, int64_t U, float gamma, float v_zero, float v_one, int64_t B, int64_t N, int D,
                          int64_t c0, int64_t c1, const float *gscale, float *dl, void *ws, int64_t ws_bytes, void *stream);
int mrg_transe_dist_bwd(const float *ent_c, const float *obj, const float *dl, int64_t ld, float *gent_c, float *gobj, int accumulate,
                        int64_t B, int64_t nc, int D, void *stream);
int64_t mrg_transe_rank_workspace_bytes(int64_t Q, int64_t N, int D);
int mrg_transe_rank(const float *obj, const float *ent, const int32_t *t_idx, const int64_t *qkey, const int32_t *when,
                    const int64_t *keys, const int32_t *rowptr, const int32_t *members, const int32_t *gone_at, int64_t U, int64_t Q,
                    int64_t N, int D, int64_t *ranks, void *ws, int64_t ws_bytes, void *stream);
/* Top-k link prediction without a [Q, N] tensor (csrc/topk.hip, csrc/transe_1n.hip, csrc/topk_parts.hpp).  Additive: ABI 23.
 *   mrg_rows_topk:   the k unfiltered entities with the largest x_e = sum_c q[i, c] * ent[e, c], largest first (mrg_rows_rank's score).
 *   mrg_transe_topk: the k unfiltered entities with the smallest dist_e = sum_c |obj[i, c] - ent[e, c]|, smallest first
 *                    (mrg_transe_rank's distance; the distance itself is compared).
 * Equal values: the lower entity id first, the rule of mrg_rank_filtered.  Filter: the index and rule of the rank entry points (a member
 * of the list of qkey[i] is excluded iff gone_at > when[i]; an unknown key, qkey[i] = -1 or U = 0 excludes nothing); there is no target, so
 * nothing is exempt.  ids [Q][k] int32, vals [Q][k] float32: the float32 accumulator the sweep compared, bit-identical with what
 * mrg_rows_rank / mrg_transe_rank compare for the same (query, entity) -- same cores, same tile routines -- so the rank of ids[i][j]
 * under the same filter is j + 1.  Where fewer than k candidates remain the tail is id -1 with value -inf (rows) / +inf (transe).
 * 1 <= k <= 64, else MRG_E_SHAPE; shapes, N and the other errors as for the rank entry points; Q == 0 returns MRG_OK with nothing
 * launched.  No atomics: bitwise repeatable.  Workspace: mrg_*_topk_workspace_bytes(Q, N, D, k) = the split table of one block of at
 * most 28 672 entities (rows, split core) + 16 bytes per query + the (row, tile) lists of one launch, at most 16 MiB: it does not
 * grow with N beyond 28 672. */
int64_t mrg_rows_topk_workspace_bytes(int64_t Q, int64_t N, int D, int k);
int mrg_rows_topk(const float *q, const float *ent, const int64_t *qkey, const int32_t *when, const int64_t *keys, const int32_t *rowptr,
                  const int32_t *members, const int32_t *gone_at, int64_t U, int64_t Q, int64_t N, int D, int k, int32_t *ids,
                  float *vals, void *ws, int64_t ws_bytes, void *stream);
int64_t mrg_transe_topk_workspace_bytes(int64_t Q, int64_t N, int D, int k);
int mrg_transe_topk(const float *obj, const float *ent, const int64_t *qkey, const int32_t *when, const int64_t *keys,
                    const int32_t *rowptr, const int32_t *members, const int32_t *gone_at, int64_t U, int64_t Q, int64_t N, int D, int k,
                    int32_t *ids, float *vals, void *ws, int64_t ws_bytes, void *stream);
/* The "dot" sweeps under a per-entity score bias, x[b, e] = sum_c q[b, c] * ent[e, c] + bias[e] -- the logit of the reference's baseline
 * model CompGCN_ConvE (models/compgcn.py:188-269) -- without a [B, N] tensor (csrc/bce.hip, rank.hip, topk.hip).  Additive: ABI 23.
 * Each entry point is its unbiased twin (mrg_distmult_bce_fwd, mrg_distmult_bce_dlogit, mrg_rows_rank, mrg_rows_topk) with bias [N]
 * float32 after ent: same arguments, same labels / filter, same cores, same errors, and the SAME workspace query
 * (mrg_distmult_bce_workspace_bytes, mrg_distmult_rank_workspace_bytes, mrg_rows_topk_workspace_bytes).  bias is required (NULL:
 * MRG_E_NULLPTR).  The bias joins the float32 accumulator by one float32 add before the sigmoid and loss term, the logit gradient,
 * the rank comparison and the top-k selection see it; kernel instances of their own, so a call without a bias runs the code it ran.
 * The rank's target score is the diagonal accumulator plus bias[t_idx[i]], the float32 add the sweep forms for the target's column: a
 * duplicate entity row with an equal bias ties exactly.  mrg_rows_bias_topk's vals are the biased logits mrg_rows_bias_rank compares.
 * mrg_cols_sum: out[c] = sum_r x[r][c] for x [rows][cols] with leading dimension ld >= cols (rows == 0: zeros) -- the bias gradient of a
 *   slice of mrg_rows_bias_bce_dlogit.  float64 accumulation in a fixed order (a wave adds every eighth row ascending, eight waves are
 *   added in wave order), stored as float32; no atomics: bitwise repeatable. */
int mrg_rows_bias_bce_fwd(const float *q, const float *ent, const float *bias, const int64_t *qkey, const int64_t *keys,
                          const int32_t *rowptr, const int32_t *objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D,
                          float *loss, void *ws, int64_t ws_bytes, void *stream);
int mrg_rows_bias_bce_dlogit(const float *q, const float *ent, const float *bias, const int64_t *qkey, const int64_t *keys,
                             const int32_t *rowptr, const int32_t *objs, int64_t U, float v_zero, float v_one, int64_t B, int64_t N, int D,
                             int64_t c0, int64_t c1, const float *gscale, float *dl, void *ws, int64_t ws_bytes, void *stream);
int mrg_rows_bias_rank(const float *q, const float *ent, const float *bias, const int32_t *t_idx, const int64_t *qkey,
                       const int32_t *when, const int64_t *keys, const int32_t *rowptr, const int32_t *members, const int32_t *gone_at,
                       int64_t U, int64_t Q, int64_t N, int D, int64_t *ranks, void *ws, int64_t ws_bytes, void *stream);
int mrg_rows_bias_topk(const float *q, const float *ent, const float *bias, const int64_t *qkey, const int32_t *when,
                       const int64_t *keys, const int32_t *rowptr, const int32_t *members, const int32_t *gone_at, int64_t U, int64_t Q,
                       int64_t N, int D, int k, int32_t *ids, float *vals, void *ws, int64_t ws_bytes, void *stream);
int mrg_cols_sum(const float *x, int64_t rows, int64_t cols, int64_t ld, float *out, void *stream);
/* The score-function search leg without a [B, N] tensor (csrc/sf_mix_1n.hip): the 1-N loss, its gradients and the filtered ranks under
 * the mixed score of MixedOp_SF over SF_OPS = [sf_TransE, sf_DisMult] (reference models/cell_lp.py:36-50, 71-86, 191-200; the
 * supernet's score_f, models/model_search_lp.py:160-161).  Additive: ABI 23.
 *   dist[b, e] = sum_c |obj[b, c] - ent[e, c]|  (obj [B][D] = sub + rel),  dot[b, e] = sum_c qd[b, c] * ent[e, c]  (qd [B][D] = sub * rel),
 *   both operands float32 and formed by the caller;  p0 = sigmoid(gamma - dist), p1 = sigmoid(dot), p = w[0] * p0 + w[1] * p1 in float32
 *   with every product and the sum rounded on its own.  w: [2] float32 ON THE DEVICE, TransE's weight first (no host synchronisation).
 *   dist is one float32 accumulator over c ascending (bit-identical with mrg_transe_score_fwd's), dot one float32 fused multiply-add
 *   chain over c ascending.
 * mrg_sfmix_bce_fwd:  loss[0] = mean over b, e of (y - 1) * max(log1p(-p), -100) - y * max(log p, -100), labels as for
 *   mrg_distmult_bce_fwd (index keys / rowptr / objs, key qkey[b], v_zero / v_one), summed in float64 -- lane, wave, workgroup, then one
 *   partial per workgroup added in a fixed order: no float atomics, bitwise repeatable.
 * mrg_sfmix_bce_grad: for the entities [c0, c1), with G = gscale[0] * (p - y) / max((1 - p) p, 1e-12) (torch's
 *   binary_cross_entropy_backward; gscale: one float on the device, the upstream gradient divided by B * N):
 *     dl0 [B][c1 - c0] = (G w[0]) ((1 - p0) p0)   the gradient with respect to x0 = gamma - dist   (feeds mrg_transe_dist_bwd)
 *     dl1 [B][c1 - c0] = (G w[1]) ((1 - p1) p1)   the gradient with respect to x1 = dot            (feeds the row GEMM's gradients)
 *   each exactly 0 where its component saturates, and dw[k] = sum over b and the entities [c0, c1) of G p_k: two float64 partials per
 *   workgroup added in a fixed order, WRITTEN to dw [2] (float32) when c0 == 0 and ADDED to it otherwise -- a caller sweeps its column
 *   chunks in ascending order.  G p_k is not clamped where p itself saturates (neither is the dense formulation's).
 * mrg_sfmix_rank: ranks[i] = 1 + #(p_e > p_t) + #(p_e == p_t, e < t) over candidates e != t = t_idx[i] that are not filtered:
 *   mrg_transe_rank's rule and filter (index, gone_at > when) on the float32 p itself; the target's p is formed by the same two chains and
 *   the same expression, so a duplicate of the target's row ties exactly.  Integer atomics only.
 * Workspace: mrg_sfmix_bce_workspace_bytes(B, N, D) for the forward and (B, c1 - c0, D) for the gradient: two integers per query and two
 * float64 per tile of 64 x 64 elements; mrg_sfmix_rank_workspace_bytes(Q, N, D), O(Q) bytes.  1 <= D <= 1024, N bounded as for
 * mrg_distmult_rank; indices are trusted.  Argument errors are returned before any HIP call; B == 0 / Q == 0 returns MRG_OK with nothing
 * launched. */
int64_t mrg_sfmix_bce_workspace_bytes(int64_t B, int64_t ncols, int D);
int mrg_sfmix_bce_fwd(const float *obj, const float *qd, const float *ent, const float *w, const int64_t *qkey, const int64_t *keys,
                      const int32_t *rowptr, const int32_t *objs, int64_t U, float gamma, float v_zero, float v_one, int64_t B, int64_t N,
                      int D, float *loss, void *ws, int64_t ws_bytes, void *stream);
int mrg_sfmix_bce_grad(const float *obj, const float *qd, const float *ent, const float *w, const int64_t *qkey, const int64_t *keys,
                       const int32_t *rowptr, const int32_t *objs, int64_t U, float gamma, float v_zero, float v_one, int64_t B, int64_t N,
                       int D, int64_t c0, int64_t c1, const float *gscale, float *dl0, float *dl1, float *dw, void *ws, int64_t ws_bytes,
                       void *stream);
int64_t mrg_sfmix_rank_workspace_bytes(int64_t Q, int64_t N, int D);
int mrg_sfmix_rank(const float *obj, const float *qd, const float *ent, const float *w, float gamma, const int32_t *t_idx,
                   const int64_t *qkey, const int32_t *when, const int64_t *keys, const int32_t *rowptr, const int32_t *members,
                   const int32_t *gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t *ranks, void *ws, int64_t ws_bytes,
                   void *stream);
/* The same leg over THREE scorers, [sf_TransE, sf_DisMult, sf_ConvE] (csrc/sf_mix_1n.hip; reference models/operations_lp.py:26-30).
 * Additive: ABI 23.  The two-way entry points argument for argument, with
 *   qh [B][D]: ConvE's hidden rows after BN2 + ReLU (float32, formed by the caller) after qd,  dot2[b, e] = sum_c qh[b, c] * ent[e, c]
 *   (one float32 fused multiply-add chain over c ascending),  p2 = sigmoid(dot2),
 *   w: [3] float32 ON THE DEVICE, and p = (w[0] * p0 + w[1] * p1) + w[2] * p2 in float32 with every product and every sum rounded on
 *   its own (the order in which sum(w * op(...)) evaluates).  With w[2] == 0 the loss, dl0, dl1 and dw[0..1] equal the two-way entry
 *   points' bit for bit.
 * mrg_sfmix3_bce_grad: dl2 [B][c1 - c0] = (G w[2]) ((1 - p2) p2), the gradient with respect to dot2, after dl1; dw [3], three float64
 *   partials per workgroup.  mrg_sfmix3_rank: the target's p is formed by the same three chains and the same expression.
 * Workspace: as above with three float64 per tile.  The same shape checks, error codes and B == 0 / Q == 0 / U == 0 handling. */
int64_t mrg_sfmix3_bce_workspace_bytes(int64_t B, int64_t ncols, int D);
int mrg_sfmix3_bce_fwd(const float *obj, const float *qd, const float *qh, const float *ent, const float *w, const int64_t *qkey,
                       const int64_t *keys, const int32_t *rowptr, const int32_t *objs, int64_t U, float gamma, float v_zero, float v_one,
                       int64_t B, int64_t N, int D, float *loss, void *ws, int64_t ws_bytes, void *stream);
int mrg_sfmix3_bce_grad(const float *obj, const float *qd, const float *qh, const float *ent, const float *w, const int64_t *qkey,
                        const int64_t *keys, const int32_t *rowptr, const int32_t *objs, int64_t U, float gamma, float v_zero, float v_one,
                        int64_t B, int64_t N, int D, int64_t c0, int64_t c1, const float *gscale, float *dl0, float *dl1, float *dl2,
                        float *dw, void *ws, int64_t ws_bytes, void *stream);
int64_t mrg_sfmix3_rank_workspace_bytes(int64_t Q, int64_t N, int D);
int mrg_sfmix3_rank(const float *obj, const float *qd, const float *qh, const float *ent, const float *w, float gamma, const int32_t *t_idx,
                    const int64_t *qkey, const int32_t *when, const int64_t *keys, const int32_t *rowptr, const int32_t *members,
                    const int32_t *gone_at, int64_t U, int64_t Q, int64_t N, int D, int64_t *ranks, void *ws, int64_t ws_bytes,
                    void *stream);
/* sf_TransE_op.forward, reference models/operations_lp.py:101-112:
 *   score[b, n] = sigmoid(gamma - sum_c |sub[b, c] + rel[b, c] - ent[n, c]|)
 * backward: gobj [B][D] (the gradient of both sub and rel) and gent [N][D]; either may be NULL.
 * (sf_DisMult_op, :115-127, is mrg_compose_fwd(MULT) + mrg_linear_fwd(act = MRG_ACT_SIGMOID).) */
int mrg_transe_score_fwd(const float *ent, const float *sub, const float *rel, float gamma, float *score,
                         int64_t B, int64_t N, int D, void *stream);
int mrg_transe_score_bwd(const float *ent, const float *sub, const float *rel, const float *gscore, const float *score,
                         float *gent, float *gobj, int64_t B, int64_t N, int D, void *stream);
/* ---- standalone circular correlation (ABI 17) ---------------------------------------------------------
 * ccorr(a, b) of reference utils/utils.py:285-301 and models/operations_lp.py:58-68 (pre_corr_op), which the reference
 * computes as irfft(conj(rfft(a)) * rfft(b)).  Rows of width 1 <= D <= MRG_CCORR_MAX_D, float32, row-major [N][D].
 * mrg_ccorr_rows: out[i] = corr(X[i], Y[i])  (MRG_CCORR: out[k] = sum_j X[j] Y[(j + k) % D])  or conv(X[i], Y[i])
 *   (MRG_CCONV: out[m] = sum_j X[j] Y[(m - j) % D]).  dL/da = corr(g, b), dL/db = conv(a, g).  N = 0 launches nothing.
 *   Sums over j ascending per output: bit-reproducible.
 * A row r shared by every row of the other operand makes ccorr a row GEMM (mrg_linear_fwd with W = the D x D circulant):
 * mrg_ccorr_matrix writes W[k][j] = r[(j + k) % D] (MRG_CCORR_H: ccorr(a, r) = a W^T) or W[k][m] = r[(m - k) % D]
 *   (MRG_CCORR_T: ccorr(r, b) = b W^T);
 * mrg_ccorr_matrix_grad folds the weight gradient gW [D][D] of that product onto gr [D]: gr[m] = sum_k gW[k][(m - k) % D] (H)
 *   or sum_k gW[k][(k + m) % D] (T), in a fixed order (no atomics).  W and gW are [D][D], not aliased with r / gr. */
#define MRG_CCORR_MAX_D 512
#define MRG_CCORR        0
#define MRG_CCONV        1
#define MRG_CCORR_H      0
#define MRG_CCORR_T      1
int mrg_ccorr_rows(int mode, const float *X, const float *Y, float *out, int64_t N, int D, void *stream);
int mrg_ccorr_matrix(int mode, const float *r, float *W, int D, void *stream);
int mrg_ccorr_matrix_grad(int mode, const float *gW, float *gr, int D, void *stream);

/* ---- ConvE feature path (ABI 18) ------------------------------------------------------------------------------------------
 * The scorer of reference models/operations_lp.py:150-205 (sf_ConvE_op) and models/compgcn.py:188-269 (CompGCN_ConvE), from the
 * (subject, relation) rows to the hidden vector in front of BN2:
 *   img = layout(sub [B][D], rel [B][D]) [B][1][Hi][Wi], Hi Wi = 2 D;  pixel t of a row (t = y Wi + x):
 *         MRG_CONVE_STACKED      (sf_ConvE_op.concat):   (t < D ? sub : rel)[t % D]
 *         MRG_CONVE_INTERLEAVED  (CompGCN_ConvE.concat): (t % 2 == 0 ? sub : rel)[t / 2]
 *   x0 = BN0(img) (BatchNorm2d(1));  z = conv(x0, Wc [F][1][ks][ks]) + bc (valid, stride 1; bc may be NULL)  [B][F][Ho][Wo]
 *   a  = keep1 * relu(BN1(z))  (BatchNorm2d(F); keep1 [B][F][Ho][Wo] = the dropout mask scaled by 1 / (1 - p), or NULL)
 *   h  = keep2 * (a.view(B, K) Wfc^T + bfc),  K = F Ho Wo  (keep2 [B][D] or NULL; bfc may be NULL)
 * training != 0: BN0 / BN1 use the batch statistics and update running_mean / running_var in place as torch does (momentum, unbiased
 *   variance; num_batches_tracked is the caller's); training == 0: the running statistics.  stats0 [2] = {mean, invstd} and
 *   stats1 [2 F] = {mean [F], invstd [F]} are written by the forward and read by the backward.
 * Shapes: 1 <= D <= MRG_CONVE_MAX_D, 1 <= ks <= MRG_CONVE_MAX_KS, ks <= Hi, Wi; else MRG_E_SHAPE.  f32 FMA arithmetic; statistics and
 *   gradient sums in float64 in a fixed order (no atomics): bit-reproducible.
 * Call order, forward: mrg_conve_bn0_fwd -> mrg_conve_conv_fwd (z) -> mrg_conve_bn1_fwd (a) -> mrg_conve_fc_fwd (h; workspace
 *   mrg_conve_fc_workspace_bytes).  Backward from gh = dL/dh: mrg_conve_fc_bwd (ga = dL/da [B][K], gWfc [D][K], gbfc; the same
 *   workspace) -> mrg_conve_bn1_bwd (ga -> dL/dz in place; gw1, gb1 [F]) -> mrg_conve_conv_bwd (workspace
 *   mrg_conve_bwd_workspace_bytes) -> mrg_conve_finish_bwd (same workspace: gsub, grel [B][D], gw0, gb0 [1], gWc [F][ks][ks], gbc [F]
 *   or NULL). */
#define MRG_CONVE_STACKED      0
#define MRG_CONVE_INTERLEAVED  1
#define MRG_CONVE_MAX_D     1024
#define MRG_CONVE_MAX_KS      15
int64_t mrg_conve_fc_workspace_bytes(int64_t B, int64_t K, int D);
int64_t mrg_conve_bwd_workspace_bytes(int64_t B, int D, int F, int ks);
int mrg_conve_bn0_fwd(const float *sub, const float *rel, int64_t B, int D, float *running_mean, float *running_var, int training,
                      float eps, float momentum, float *stats0, void *stream);
int mrg_conve_conv_fwd(int layout, const float *sub, const float *rel, int64_t B, int D, int Hi, int Wi, const float *stats0,
                       const float *bn0_w, const float *bn0_b, const float *Wc, const float *bc, int F, int ks, float *z, void *stream);
int mrg_conve_bn1_fwd(const float *z, int64_t B, int F, int P, const float *bn1_w, const float *bn1_b, float *running_mean,
                      float *running_var, const float *keep1, int training, float eps, float momentum, float *stats1, float *a,
                      void *stream);
int mrg_conve_fc_fwd(const float *a, const float *Wfc, const float *bfc, const float *keep2, float *h, void *ws, int64_t B, int64_t K,
                     int D, void *stream);
int mrg_conve_fc_bwd(const float *gh, const float *keep2, const float *a, const float *Wfc, float *ga, float *gWfc, float *gbfc,
                     void *ws, int64_t B, int64_t K, int D, void *stream);
int mrg_conve_bn1_bwd(float *g, const float *z, const float *a, const float *keep1, const float *stats1, const float *bn1_w,
                      int training, int64_t B, int F, int P, float *gw1, float *gb1, void *stream);
int mrg_conve_conv_bwd(int layout, const float *sub, const float *rel, int64_t B, int D, int Hi, int Wi, const float *stats0,
                       const float *bn0_w, const float *bn0_b, const float *Wc, int F, int ks, const float *gz, void *ws, void *stream);
int mrg_conve_finish_bwd(int layout, const float *sub, const float *rel, int64_t B, int D, int F, int ks, const float *stats0,
                         const float *bn0_w, int training, const void *ws, float *gsub, float *grel, float *gw0, float *gb0,
                         float *gWc, float *gbc, void *stream);

/* gT[n][b] = g[b][n] * act'(y[b][n]): the output gradient of a wide, short Linear (the [B, N] scorers: N = all entities) with the
 * activation's derivative folded in, transposed to [N][B] rows -- the layout both of its gradient products stream
 * (functional._Linear.backward; replaces torch's mul / rsub / mul / strided copy).  act: MRG_ACT_NONE (y may be NULL) / _RELU /
 * _SIGMOID, y = the forward's output.  B <= 64 * 65535. */
int mrg_act_grad_transpose(const float *g, const float *y, float *gT, int64_t B, int64_t N, int act, void *stream);

/* ---- the candidate Linears of one node-classification MixedOp ------------------------------------
 * MixedOp.__init__ / op_forward   reference models/cell.py:17-31: every candidate k of a MixedOp carries its own
 * nn.Linear(D, D, bias=True) between the operator and the BatchNorm.  One launch serves n <= 4 candidates ("members") of the same
 * rows and the same square D:   Y[k] = X[k] W[k]^T + bias[k]   (mrg_cand_linear_fwd)   gX[k] = gY[k] W[k]   (mrg_cand_linear_bwd_input,
 * the same product with the weight read through transposed strides, no bias).  X / W / bias / Y: HOST arrays of n device pointers
 * (bias, or any of its entries, may be NULL; two members may read the same X; the outputs are distinct), X[k], Y[k]: [rows][D],
 * W[k]: [D][D], all 16-byte aligned.  Exact-f32 matrix core (v_mfma_f32_32x32x2_f32), the weight staged in LDS: no global
 * workspace -- mrg_cand_linear_workspace_bytes(n, D) is 0 for every shape of this core, and ws may then be NULL
 * (MRG_E_WORKSPACE when it returns > 0 and ws is NULL).  Shapes: D % 4 == 0 and 16 <= D <= 128, any rows >= 0; another D, or a
 * pointer that is not 16-byte aligned: MRG_E_SHAPE (the caller runs mrg_linear_fwd / mrg_linear_bwd_input per member).
 * colsum (reference models/cell.py:19, the BatchNorm1d that reads Y[k]): NULL, or [n][blocks][2 (sum, sum of squares)][D] float64,
 * the column sums of the float32 values stored in Y[k], one partial per workgroup formed from the registers that hold the output
 * and added in a fixed order (no atomics) -- the layout of mrg_gated_branch.given with given_n = blocks, given_stride = 2 D.
 * blocks = mrg_cand_linear_colsum_blocks(rows, D), 0 = the shape has no grouped form; colsum_blocks: what the caller sized
 * colsum for (MRG_E_SHAPE when the launch would write another number).  Y is the same bits with and without colsum. */
int64_t mrg_cand_linear_colsum_blocks(int64_t rows, int D);
int64_t mrg_cand_linear_workspace_bytes(int n, int D);
int mrg_cand_linear_fwd(int n, const float *const *X, const float *const *W, const float *const *bias, float *const *Y, void *ws,
                        int64_t rows, int D, void *stream, double *colsum, int64_t colsum_blocks);
int mrg_cand_linear_bwd_input(int n, const float *const *gY, const float *const *W, float *const *gX, void *ws, int64_t rows, int D,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MRGNAS_H */
