"""The step after the path: DistMult triple scoring, the [B, N] score functions (csrc/scoring.hip) and the 1-N losses that need no
[B, N] tensor: the "dot" scorers' (DistMult, ConvE: csrc/bce.hip) and TransE's (csrc/transe_1n.hip).

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h): every Function enqueues HIP kernels of
libmrgnas_hip.so on torch's current stream through ctypes; every call site states the algorithmic bytes / flops of the launch."""
import ctypes

import torch

from .._lib import MrgnasError, call, check, f32c, ptr, require_hip, stream_of
from ._base import _ws, _ws_bytes
from .gcs import span_gcs
from .compose_gather import compose
from .row_linear import linear


class ScorePlan:
    """Index structures of a scoring batch of (s, r, o) triples: int32 indices for the forward and
    three span plans (by subject, by object, by relation) whose metadata carries the element id in
    the scale slot, so the backward can take the upstream gradient as an external scale."""

    def __init__(self, triplets, n_ent, n_rel):
        from ..graph import span_plan
        t = triplets.long()
        s, r, o = t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous()
        self.T, self.n_ent, self.n_rel = int(t.shape[0]), int(n_ent), int(n_rel)
        self.s32, self.r32, self.o32 = (x.to(torch.int32).contiguous() for x in (s, r, o))

        def packed(plan, xi, yi):
            from ..graph import span_meta
            return span_meta(plan, xi, yi, None, w_is_index=True)
        self.by_s, self.by_o, self.by_r = span_plan(s, n_ent), span_plan(o, n_ent), span_plan(r, n_rel)
        self.m_s = packed(self.by_s, o, r)        # g_ent[s] += g_t * ent[o] * rel[r]
        self.m_o = packed(self.by_o, s, r)        # g_ent[o] += g_t * ent[s] * rel[r]
        self.m_r = packed(self.by_r, s, o)        # g_rel[r] += g_t * ent[s] * ent[o]     (Y = ent as well)


class _DistMult(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ent, rel, sp):
        ent, rel = f32c(ent), f32c(rel)
        require_hip(ent, rel)
        D = ent.shape[1]
        score = torch.empty(sp.T, dtype=torch.float32, device=ent.device)
        call("mrg_distmult_score", (ptr(ent), ptr(rel), ptr(sp.s32), ptr(sp.r32), ptr(sp.o32), ptr(score), sp.T, D, stream_of(ent)),
             nbytes=sp.T * (12 * D + 16))
        ctx.sp = sp
        ctx.save_for_backward(ent, rel)
        return score

    @staticmethod
    def backward(ctx, g):
        ent, rel = ctx.saved_tensors
        sp = ctx.sp
        g = f32c(g)
        g_ent = span_gcs("mul", ent, rel, sp.m_s, sp.by_s, ext_scal=g)
        g_ent += span_gcs("mul", ent, rel, sp.m_o, sp.by_o, ext_scal=g)
        g_rel = span_gcs("mul", ent, ent, sp.m_r, sp.by_r, ext_scal=g)
        return g_ent, g_rel, None


def distmult_score(ent, rel, sp):
    """sum_c ent[s] * rel[r] * ent[o] per triple (reference models/model_search_lp.py:169-176)."""
    return _DistMult.apply(ent, rel, sp)


def distmult_scores_all(all_ent, sub_emb, rel_emb):
    """sf_DisMult_op (reference models/operations_lp.py:115-127): sigmoid((sub * rel) all_ent^T) as the compose kernel +
    the MFMA row GEMM with a sigmoid epilogue (all_ent [N, D] is the GEMM's weight operand: no transpose, no [B, N]
    pre-activation tensor)."""
    return linear(compose("mult", sub_emb, rel_emb), all_ent, None, "sigmoid")


BCE_COL_BLOCK = 7 * 32              # the sweep's column block (csrc/sweep_host.hpp: RANK_NT tiles of 32)
BCE_DL_BYTES = 64 << 20             # default bound of the backward's [B, col_chunk] logit-gradient slice


def bce_default_col_chunk(B):
    """The largest multiple of the sweep's column block whose [B, col_chunk] float32 slice stays within BCE_DL_BYTES."""
    return max(BCE_COL_BLOCK, BCE_DL_BYTES // (4 * max(int(B), 1)) // BCE_COL_BLOCK * BCE_COL_BLOCK)


# The C entry points of the 1-N losses by score kind: "dot" (logit = q . entity, csrc/bce.hip) and "l1" (logit = gamma - ||q - entity||_1,
# csrc/transe_1n.hip).  The "l1" calls take gamma in front of v_zero; everything else is the same argument list.
_BCE_ENTRY = {"dot": ("mrg_distmult_bce_workspace_bytes", "mrg_distmult_bce_fwd", "mrg_distmult_bce_dlogit"),
              "l1": ("mrg_transe_bce_workspace_bytes", "mrg_transe_bce_fwd", "mrg_transe_bce_dlogit")}
# The "dot" calls with a per-entity score bias (logit = q . entity + bias[entity]: CompGCN_ConvE): the bias pointer follows ent; same
# workspace.  Kernel instances of their own: a call without a bias runs what it always ran.
_BCE_BIAS_ENTRY = ("mrg_distmult_bce_workspace_bytes", "mrg_rows_bias_bce_fwd", "mrg_rows_bias_bce_dlogit")


def _bce_entry(kind, bias):
    return _BCE_ENTRY[kind] if bias is None else _BCE_BIAS_ENTRY         # (score_bias_arg has refused a bias with kind "l1")


def score_bias_arg(what, bias, kind, N):
    """The checks of an optional per-entity score bias, before any device check: None stays None; else kind must be "dot" and the
    bias [N].  Returns it float32 and contiguous."""
    if bias is None:
        return None
    if kind != "dot":
        raise ValueError(f"{what}: a score bias is defined for \"dot\" scorers only (logit = q . entity + bias[entity]); kind \"{kind}\" has none")
    if bias.dim() != 1 or int(bias.numel()) != int(N):
        raise ValueError(f"{what}: bias [num_ent] = [{int(N)}] expected, got {list(bias.shape)}")
    return f32c(bias)


def _checked_ws(name, B, cols, D, like):
    nbytes = _ws_bytes(name, B, cols, D)
    if nbytes < 0:
        check(int(nbytes), name)
    return _ws(nbytes, like), int(nbytes)


def _bce_mean(kind, gamma, q, ent, li, qkey, v_zero, v_one, bias=None):
    ws_name, fwd, _ = _bce_entry(kind, bias)
    (B, D), N = q.shape, ent.shape[0]
    loss = torch.empty((), dtype=torch.float32, device=q.device)
    ws, nbytes = _checked_ws(ws_name, B, N, D, q)
    values = (float(gamma), v_zero, v_one) if kind == "l1" else (v_zero, v_one)
    head = (ptr(q), ptr(ent)) if bias is None else (ptr(q), ptr(ent), ptr(bias))
    call(fwd, (*head, ptr(qkey), ptr(li.keys), ptr(li.rowptr), ptr(li.objs), int(li.keys.numel()), *values, B, N, D,
               ptr(loss), ptr(ws), nbytes, stream_of(q)),
         nbytes=4 * (B + N) * D, flops=2 * B * N * D)
    return loss


def _bce_dlogit(kind, gamma, q, ent, li, qkey, v_zero, v_one, c0, c1, gscale, out, bias=None):
    ws_name, _, dlogit = _bce_entry(kind, bias)
    (B, D), N, nc = q.shape, ent.shape[0], c1 - c0
    if out is None:
        out = torch.empty(B * nc, dtype=torch.float32, device=q.device)
    ws, nbytes = _checked_ws(ws_name, B, nc, D, q)
    values = (float(gamma), v_zero, v_one) if kind == "l1" else (v_zero, v_one)
    head = (ptr(q), ptr(ent)) if bias is None else (ptr(q), ptr(ent), ptr(bias))
    call(dlogit, (*head, ptr(qkey), ptr(li.keys), ptr(li.rowptr), ptr(li.objs), int(li.keys.numel()), *values, B, N, D,
                  c0, c1, ptr(gscale), ptr(out), ptr(ws), nbytes, stream_of(q)),
         nbytes=4 * (B + nc) * D + 4 * B * nc, flops=2 * B * nc * D)
    return out[:B * nc].view(B, nc)


def distmult_bce_mean(q, ent, label_index, qkey, v_zero, v_one, bias=None):
    """mrg_distmult_bce_fwd, no autograd: mean over [B, N] of BCE(sigmoid(q ent^T), labels) as a float32 device scalar.  bias [N]:
    the logits are q ent^T + bias (mrg_rows_bias_bce_fwd)."""
    bias = score_bias_arg("distmult_bce_mean", bias, "dot", ent.shape[0])
    require_hip(bias)
    return _bce_mean("dot", None, q, ent, label_index, qkey, v_zero, v_one, bias)


def transe_bce_mean(obj, ent, gamma, label_index, qkey, v_zero, v_one):
    """mrg_transe_bce_fwd, no autograd: mean over [B, N] of BCE(sigmoid(gamma - ||obj - ent||_1), labels) as a float32 device scalar."""
    return _bce_mean("l1", gamma, obj, ent, label_index, qkey, v_zero, v_one)


def distmult_bce_dlogit(q, ent, label_index, qkey, v_zero, v_one, c0, c1, gscale, out=None, bias=None):
    """mrg_distmult_bce_dlogit, no autograd: the loss gradient with respect to the logits of the entities [c0, c1) as [B, c1 - c0],
    written into the first B * (c1 - c0) floats of `out` when given.  gscale: float32 [1] on the device (upstream gradient / (B N)).
    bias [N]: the logits are q ent^T + bias (mrg_rows_bias_bce_dlogit)."""
    bias = score_bias_arg("distmult_bce_dlogit", bias, "dot", ent.shape[0])
    require_hip(bias)
    return _bce_dlogit("dot", None, q, ent, label_index, qkey, v_zero, v_one, c0, c1, gscale, out, bias)


def cols_sum(x, out=None):
    """mrg_cols_sum, no autograd: the column sums of x [rows, cols] float32 as [cols] float32 (into `out` when given), accumulated in
    float64 in a fixed order -- no float atomics, the same bits on every call.  The bias gradient of a logit-gradient slice."""
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
    call("mrg_cols_sum", (ptr(x), rows, cols, cols, ptr(out), stream_of(x)), nbytes=4 * (rows + 1) * cols)
    return out


def transe_bce_dlogit(obj, ent, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, out=None):
    """mrg_transe_bce_dlogit, no autograd: the loss gradient with respect to x = gamma - dist of the entities [c0, c1) as [B, c1 - c0],
    written into the first B * (c1 - c0) floats of `out` when given.  gscale: float32 [1] on the device (upstream gradient / (B N))."""
    return _bce_dlogit("l1", gamma, obj, ent, label_index, qkey, v_zero, v_one, c0, c1, gscale, out)


def _dot_chunk_bwd(q, ent, dl, c0, nc, g_q, g_ent, pre, st, ent_dst=None):
    """One column chunk of the "dot" backward: the two gradient GEMMs of `linear` on dl [B, nc]: g_q += dl ent[c0:c1]
    (mrg_linear_bwd_input, accumulating) and g_ent[c0:c1] = dl^T q (mrg_linear_fwd on the transposed operands).  pre: (q^T, the row
    GEMM's workspace) when g_ent is wanted.  ent_dst: a [>= nc, D] scratch that receives dl^T q in place of g_ent[c0:c1] (a second "dot"
    leg on the same entities, which its caller adds)."""
    (B, D), esz = q.shape, ent.element_size()
    need_q, need_ent = g_q is not None, g_ent is not None
    work = dict(nbytes=4 * B * (D + nc) + 4 * D * nc, flops=2 * B * D * nc)
    ent_c = ctypes.c_void_p(ent.data_ptr() + c0 * D * esz)
    # a wide chunk: both gradients run on the transposed slice dl^T [nc, B], as `linear`'s backward does for Nout = N >> rows
    wide_q = need_q and nc > 1024 and B <= 1024 and (B <= 128 or (B % 4 == 0 and D % 4 == 0))
    dlT = dl[:B * nc].view(B, nc).t().contiguous() if (need_ent or wide_q) else None
    if wide_q:
        # g_q (+)= dl ent[c0:c1] is a reduction over the chunk's entities into a [B, D] block, the shape of a weight gradient
        # (rows := nc, gY := dl^T, X := ent[c0:c1]): the split-over-rows kernel spreads it over the chip, where the row GEMM
        # would give the whole reduction to ceil(B / 128) workgroups
        out = g_q if c0 == 0 else torch.empty_like(g_q)
        ws = _ws(_ws_bytes("mrg_linear_bwd_weight_workspace_bytes", nc, D, B), q)
        call("mrg_linear_bwd_weight", (ptr(dlT), ent_c, None, ptr(out), None, ptr(ws), nc, D, 0, B, st), **work)
        if c0 > 0:
            g_q += out
    elif need_q:                  # g_q (+)= dl ent[c0:c1]
        wt = _ws(_ws_bytes("mrg_linear_bwd_input_workspace_bytes", D, nc), q)
        call("mrg_linear_bwd_input", (ptr(dl), ent_c, ptr(g_q), ptr(wt), B, D, nc, D, 1 if c0 > 0 else 0, st), **work)
    if need_ent:
        # g_ent[c0:c1] = dl^T q: a tall-skinny row GEMM over the transposed operands (the split-over-rows weight-gradient
        # kernel keeps all of gW's row tiles in registers: it does not cover thousands of output rows, nor a chunk whose
        # width is no multiple of 4)
        qT, gws = pre
        dst = ctypes.c_void_p(g_ent.data_ptr() + c0 * D * esz) if ent_dst is None else ptr(ent_dst)
        call("mrg_linear_fwd", (ptr(dlT), ptr(qT), None, dst, ptr(gws), nc, B, D, 0, st), **work)


def _l1_chunk_bwd(obj, ent, dl, c0, nc, g_obj, g_ent, pre, st):
    """One column chunk of the "l1" backward: mrg_transe_dist_bwd on dl [B, nc], the gradient with respect to gamma - dist:
    g_ent[c0:c1] written, g_obj accumulated in chunk order.  No transpose."""
    (B, D), esz = obj.shape, ent.element_size()
    need_obj, need_ent = g_obj is not None, g_ent is not None
    call("mrg_transe_dist_bwd", (ctypes.c_void_p(ent.data_ptr() + c0 * D * esz), ptr(obj), ptr(dl), nc,
                                 ctypes.c_void_p(g_ent.data_ptr() + c0 * D * esz) if need_ent else None, ptr(g_obj),
                                 1 if c0 > 0 else 0, B, nc, D, st),
         nbytes=4 * (B * nc + (B + nc) * D), flops=(int(need_obj) + int(need_ent)) * 2 * B * nc * D)


class _BCE1N(torch.autograd.Function):
    """loss(q, ent) of the 1-N losses, kind "dot" or "l1".  Forward: one sweep that stores nothing per element.  Backward: per column
    chunk the logit gradient slice dl [B, chunk] (mrg_distmult_bce_dlogit / mrg_transe_bce_dlogit, the tile recomputed) and the
    kind's work on it (_dot_chunk_bwd / _l1_chunk_bwd)."""

    @staticmethod
    def forward(ctx, kind, gamma, q, ent, label_index, qkey, v_zero, v_one, col_chunk, bias=None):
        q, ent = f32c(q), f32c(ent)
        li = label_index
        bias = score_bias_arg("the 1-N loss", bias, kind, ent.shape[0])
        require_hip(q, ent, qkey, li.keys, li.rowptr, li.objs, bias)
        ctx.kind, ctx.gamma = kind, None if gamma is None else float(gamma)
        ctx.li, ctx.v, ctx.col_chunk = li, (v_zero, v_one), col_chunk
        ctx.save_for_backward(q, ent, qkey, bias)
        return _bce_mean(kind, gamma, q, ent, li, qkey, v_zero, v_one, bias)

    @staticmethod
    def backward(ctx, g):
        q, ent, qkey, bias = ctx.saved_tensors
        kind, li, (v_zero, v_one), step = ctx.kind, ctx.li, ctx.v, ctx.col_chunk
        (B, D), N, st = q.shape, ent.shape[0], stream_of(q)
        step = min(step, N)
        need_q, need_ent = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        g_bias = torch.empty_like(bias) if bias is not None and ctx.needs_input_grad[9] else None
        gscale = (g.detach().float().reshape(1) / float(B * N)).contiguous()          # stays on the device: no host synchronisation
        dl = torch.empty(B * step, dtype=torch.float32, device=q.device)               # ONE slice, reused by every chunk
        g_q = torch.empty_like(q) if need_q else None
        g_ent = torch.empty_like(ent) if need_ent else None
        pre = None
        if kind == "dot" and need_ent:
            pre = q.t().contiguous(), _ws(_ws_bytes("mrg_gemm_workspace_bytes", B, D), q)
        chunk_bwd = _dot_chunk_bwd if kind == "dot" else _l1_chunk_bwd
        for c0 in range(0, N, step):
            c1 = min(N, c0 + step)
            dl_c = _bce_dlogit(kind, ctx.gamma, q, ent, li, qkey, v_zero, v_one, c0, c1, gscale, dl, bias)
            if g_bias is not None:                                                     # g_bias[c0:c1] = the slice's column sums
                cols_sum(dl_c, g_bias[c0:c1])
            chunk_bwd(q, ent, dl, c0, c1 - c0, g_q, g_ent, pre, st)
        return None, None, g_q, g_ent, None, None, None, None, None, g_bias


def _require_cuda(what, tensors):
    for t in tensors:
        if not t.is_cuda:
            raise MrgnasError(f"{what} runs on a HIP device (no CPU fallback); got a tensor on " + str(t.device))


def _bce_all_args(what, tensors, B, N, label_index, subj, rel, label_smooth, col_chunk):
    """The checks and the derived arguments the 1-N losses share: (qkey, v_zero, v_one, col_chunk)."""
    _require_cuda(what, tensors)
    if B == 0 or N == 0 or N != label_index.num_ent or subj.numel() != B or rel.numel() != B:
        raise ValueError(f"{what}: all_ent [num_ent, D], query rows [B, D], subj / rel [B] with B > 0 expected")
    if col_chunk is None:
        col_chunk = bce_default_col_chunk(B)
    col_chunk = int(col_chunk)
    if col_chunk < 1:
        raise ValueError(f"{what}: col_chunk must be positive")
    v_zero, v_one = label_index.label_values(label_smooth)
    qkey = (subj.long() * (2 * label_index.num_rel) + rel.long()).contiguous()
    return qkey, v_zero, v_one, col_chunk


def rows_bce_all(kind, gamma, all_ent, q, label_index, subj, rel, label_smooth=0.0, col_chunk=None, _what="rows_bce_all", bias=None):
    """The 1-N losses from the point where the query rows exist (the scorers' ``query``): the mean over [B, N] of BCELoss(sigmoid(x),
    label_index.labels(subj, rel, label_smooth)) for rows q [B, D] the caller formed, with x = q all_ent^T for kind "dot" (DistMult's
    sub * rel, ConvE's hidden vector after BN2 + ReLU; gamma unused) and x = gamma - ||q - all_ent||_1 for kind "l1" (TransE's
    sub + rel).  bias [num_ent] (kind "dot" only, else ValueError): a per-entity score bias, x = q all_ent^T + bias, with its gradient
    (CompGCN_ConvE's).  No [B, N] tensor, no host synchronisation."""
    if q.dim() != 2 or all_ent.dim() != 2 or q.shape[1] != all_ent.shape[1]:
        raise ValueError(f"{_what}: all_ent [num_ent, D] and query rows [B, D] expected")
    B, N = int(q.shape[0]), int(all_ent.shape[0])
    score_bias_arg(_what, bias, kind, N)                       # (before any device check)
    tensors = (all_ent, q, subj, rel) if bias is None else (all_ent, q, subj, rel, bias)
    qkey, v_zero, v_one, col_chunk = _bce_all_args(_what, tensors, B, N, label_index, subj, rel, label_smooth, col_chunk)
    return _BCE1N.apply(kind, gamma, q, all_ent, label_index, qkey, v_zero, v_one, col_chunk, bias)


def dot_bce_all(all_ent, q, label_index, subj, rel, label_smooth=0.0, col_chunk=None, _what="dot_bce_all", bias=None):
    """distmult_bce_all from the point where the query rows exist: rows_bce_all for the "dot" scorers.  Same kernels, same memory."""
    return rows_bce_all("dot", None, all_ent, q, label_index, subj, rel, label_smooth, col_chunk, _what=_what, bias=bias)


def distmult_bce_all(all_ent, sub_emb, rel_emb, label_index, subj, rel, label_smooth=0.0, col_chunk=None):
    """The fixed-genotype driver's training loss (reference train/mr_lp_train.py Network._loss with sf_DisMult_op): the mean over [B, N]
    of BCELoss(sigmoid((sub_emb * rel_emb) all_ent^T), label_index.labels(subj, rel, label_smooth)) as a float32 scalar, with no [B, N]
    tensor -- neither the labels, nor the predictions, nor the loss terms.  The backward holds one [B, col_chunk] slice of the logit
    gradient and its transpose (default: bce_default_col_chunk(B)).  label_index: sampler.LabelIndex on the same device.  No host synchronisation."""
    _require_cuda("distmult_bce_all", (all_ent, sub_emb, rel_emb, subj, rel))
    if int(sub_emb.shape[0]) == 0:
        raise ValueError("distmult_bce_all: all_ent [num_ent, D], sub_emb / rel_emb [B, D], subj / rel [B] with B > 0 expected")
    return dot_bce_all(all_ent, compose("mult", sub_emb, rel_emb), label_index, subj, rel, label_smooth, col_chunk, _what="distmult_bce_all")


def transe_bce_all(all_ent, sub_emb, rel_emb, gamma, label_index, subj, rel, label_smooth=0.0, col_chunk=None):
    """The fixed-genotype driver's training loss with sf_TransE_op: the mean over [B, N] of BCELoss(sigmoid(gamma - ||sub_emb + rel_emb -
    all_ent||_1), label_index.labels(subj, rel, label_smooth)) as a float32 scalar with no [B, N] tensor (csrc/transe_1n.hip).  The
    backward holds one [B, col_chunk] slice (default: bce_default_col_chunk(B)) and no transpose; the gradient of obj = sub_emb + rel_emb
    goes to both.  No host synchronisation."""
    if sub_emb.dim() != 2 or sub_emb.shape != rel_emb.shape or all_ent.dim() != 2 or sub_emb.shape[1] != all_ent.shape[1]:
        raise ValueError("transe_bce_all: all_ent [num_ent, D] and sub_emb / rel_emb [B, D] expected")
    _require_cuda("transe_bce_all", (all_ent, sub_emb, rel_emb, subj, rel))
    if int(sub_emb.shape[0]) == 0:
        raise ValueError("transe_bce_all: all_ent [num_ent, D], query rows [B, D], subj / rel [B] with B > 0 expected")
    return rows_bce_all("l1", gamma, all_ent, compose("add", sub_emb, rel_emb), label_index, subj, rel, label_smooth, col_chunk,
                        _what="transe_bce_all")


class _TransE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, all_ent, sub, rel, gamma):
        all_ent, sub, rel = f32c(all_ent), f32c(sub), f32c(rel)
        require_hip(all_ent, sub, rel)
        B, D = sub.shape
        N = all_ent.shape[0]
        score = torch.empty(B, N, dtype=torch.float32, device=sub.device)
        call("mrg_transe_score_fwd", (ptr(all_ent), ptr(sub), ptr(rel), float(gamma), ptr(score), B, N, D, stream_of(sub)),
             nbytes=4 * (B * N + (N + 2 * B) * D))
        ctx.save_for_backward(all_ent, sub, rel, score)
        return score

    @staticmethod
    def backward(ctx, g):
        all_ent, sub, rel, score = ctx.saved_tensors
        g = f32c(g)
        B, D = sub.shape
        N = all_ent.shape[0]
        gent = torch.empty_like(all_ent) if ctx.needs_input_grad[0] else None
        gobj = torch.empty_like(sub) if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) else None
        call("mrg_transe_score_bwd", (ptr(all_ent), ptr(sub), ptr(rel), ptr(g), ptr(score), ptr(gent), ptr(gobj), B, N, D, stream_of(sub)))
        return gent, gobj, gobj, None


def transe_scores_all(all_ent, sub_emb, rel_emb, gamma):
    """sf_TransE_op (reference models/operations_lp.py:101-112): sigmoid(gamma - ||sub + rel - ent||_1) for all entities."""
    return _TransE.apply(all_ent, sub_emb, rel_emb, gamma)
