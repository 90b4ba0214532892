"""The score-function search leg: the 1-N loss under the MIXED score of MixedOp_SF without a [B, N] tensor (csrc/sf_mix_1n.hip; reference
models/cell_lp.py:36-50, models/model_search_lp.py:160-161), over SF_OPS = ['sf_TransE', 'sf_DisMult']

    p[b, e] = w0 * sigmoid(gamma - ||sub_b + rel_b - ent_e||_1) + w1 * sigmoid((sub_b * rel_b) . ent_e)

or over ['sf_TransE', 'sf_DisMult', 'sf_ConvE'], with the third term + w2 * sigmoid(hidden_b . ent_e), hidden = sf_ConvE_op.query(sub_emb,
rel_emb), the [B, D] row after BN2 + ReLU: the ConvE parameters get their gradient through it.

BCE(sum w_k p_k, y) is no function of the BCE(p_k, y), so this is one sweep that forms all scores of every (query, entity) pair from the
same staged rows -- not a composition of the fixed-genotype losses of functional.scoring.  One implementation serves both: the "dot"
operands (qd = sub * rel, then hidden) are a tuple, NS = 1 + len(dots) selects the mrg_sfmix_* or the mrg_sfmix3_* entry points.

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h): every Function enqueues HIP kernels of
libmrgnas_hip.so on torch's current stream through ctypes; every call site states the algorithmic bytes / flops of the launch."""
import ctypes

import torch

from .._lib import call, f32c, ptr, require_hip, stream_of
from ._base import _ws, _ws_bytes
from .compose_gather import compose
from .scoring import _bce_all_args, _checked_ws, _dot_chunk_bwd, _require_cuda, bce_default_col_chunk

_PREFIX = {2: "mrg_sfmix", 3: "mrg_sfmix3"}          # by the number of scorers NS = 1 + the number of dot operands


def _labels(li, qkey):
    return ptr(qkey), ptr(li.keys), ptr(li.rowptr), ptr(li.objs), int(li.keys.numel())


def _mix_mean(obj, dots, ent, weights, gamma, label_index, qkey, v_zero, v_one):
    """<prefix>_bce_fwd: the mean over [B, N] of BCE(mixed p, labels) as a float32 device scalar."""
    obj, ent, weights, dots = f32c(obj), f32c(ent), f32c(weights), tuple(f32c(q) for q in dots)
    require_hip(obj, *dots, ent, weights, qkey)
    (B, D), N, ns = obj.shape, ent.shape[0], 1 + len(dots)
    loss = torch.empty((), dtype=torch.float32, device=obj.device)
    ws, nbytes = _checked_ws(_PREFIX[ns] + "_bce_workspace_bytes", B, N, D, obj)
    call(_PREFIX[ns] + "_bce_fwd", (ptr(obj), *(ptr(q) for q in dots), ptr(ent), ptr(weights), *_labels(label_index, qkey), float(gamma), v_zero,
                                    v_one, B, N, D, ptr(loss), ptr(ws), nbytes, stream_of(obj)),
         nbytes=4 * (ns * B + N) * D, flops=(2 * ns + 1) * B * N * D)
    return loss


def _mix_grad(obj, dots, ent, weights, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, dl, dw):
    """<prefix>_bce_grad: (dl_0 .. dl_{NS-1}, dw) for the entities [c0, c1); dl: NS buffers or Nones, dw [NS] or None."""
    (B, D), N, nc, ns = obj.shape, ent.shape[0], c1 - c0, 1 + len(dots)
    dl = [torch.empty(B * nc, dtype=torch.float32, device=obj.device) if d is None else d for d in dl]
    dw = torch.zeros(ns, dtype=torch.float32, device=obj.device) if dw is None else dw
    ws, nbytes = _checked_ws(_PREFIX[ns] + "_bce_workspace_bytes", B, nc, D, obj)
    call(_PREFIX[ns] + "_bce_grad", (ptr(obj), *(ptr(q) for q in dots), ptr(ent), ptr(weights), *_labels(label_index, qkey), float(gamma), v_zero,
                                     v_one, B, N, D, c0, c1, ptr(gscale), *(ptr(d) for d in dl), ptr(dw), ptr(ws), nbytes, stream_of(obj)),
         nbytes=4 * (ns * B + nc) * D + 4 * ns * B * nc, flops=(2 * ns + 1) * B * nc * D)
    return (*(d[:B * nc].view(B, nc) for d in dl), dw)


def sf_mix_bce_mean(obj, qd, ent, weights, gamma, label_index, qkey, v_zero, v_one):
    """mrg_sfmix_bce_fwd, no autograd: the mean over [B, N] of BCE(w0 sigmoid(gamma - ||obj - ent||_1) + w1 sigmoid(qd ent^T), labels) as
    a float32 device scalar.  obj = sub + rel and qd = sub * rel [B, D]; weights [2] float32 on the device (TransE's first)."""
    return _mix_mean(obj, (qd,), ent, weights, gamma, label_index, qkey, v_zero, v_one)


def sf_mix_bce_grad(obj, qd, ent, weights, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, dl0=None, dl1=None, dw=None):
    """mrg_sfmix_bce_grad, no autograd: (dl0, dl1, dw) for the entities [c0, c1): the loss gradient with respect to gamma - dist and to
    the dot product as [B, c1 - c0] each (written into the first B * (c1 - c0) floats of dl0 / dl1 when given), and the gradient with
    respect to the two weights, written to dw [2] when c0 == 0 and added to it otherwise.  gscale: float32 [1] on the device."""
    return _mix_grad(obj, (qd,), ent, weights, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, (dl0, dl1), dw)


def sf_mix3_bce_mean(obj, qd, qh, ent, weights, gamma, label_index, qkey, v_zero, v_one):
    """mrg_sfmix3_bce_fwd, no autograd: the mean over [B, N] of BCE((w0 sigmoid(gamma - ||obj - ent||_1) + w1 sigmoid(qd ent^T)) +
    w2 sigmoid(qh ent^T), labels) as a float32 device scalar.  obj = sub + rel, qd = sub * rel and qh = ConvE's hidden rows [B, D];
    weights [3] float32 on the device (TransE's, DistMult's, ConvE's)."""
    return _mix_mean(obj, (qd, qh), ent, weights, gamma, label_index, qkey, v_zero, v_one)


def sf_mix3_bce_grad(obj, qd, qh, ent, weights, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, dl0=None, dl1=None, dl2=None,
                     dw=None):
    """mrg_sfmix3_bce_grad, no autograd: (dl0, dl1, dl2, dw) for the entities [c0, c1): the loss gradient with respect to gamma - dist,
    to the DistMult dot product and to the ConvE dot product as [B, c1 - c0] each (written into the first B * (c1 - c0) floats of dl0 /
    dl1 / dl2 when given), and the gradient with respect to the three weights, written to dw [3] when c0 == 0 and added to it
    otherwise.  gscale: float32 [1] on the device."""
    return _mix_grad(obj, (qd, qh), ent, weights, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, (dl0, dl1, dl2), dw)


class _MixBCE1N(torch.autograd.Function):
    """loss(ent, weights, obj, *dots).  Forward: one sweep that stores nothing per element.  Backward, per column chunk: ONE
    <prefix>_bce_grad into NS reused slices dl_k [B, chunk] with the chunk's share of dw (the tile recomputed); the "dot" work on dl_1
    with qd (scoring._dot_chunk_bwd: g_qd accumulated, g_ent[c0:c1] written); the same work on every further dot operand, its entity
    half into a [chunk, D] scratch that is added to g_ent[c0:c1]; last the "l1" work on dl_0 (mrg_transe_dist_bwd: g_obj accumulated
    in chunk order), its entity half through the same scratch.  g_ent[c0:c1] = (DistMult's [+ ConvE's]) + TransE's, in that order on
    one stream: bit-repeatable."""

    @staticmethod
    def forward(ctx, gamma, label_index, qkey, v_zero, v_one, col_chunk, ent, weights, obj, *dots):
        obj, ent, weights, dots = f32c(obj), f32c(ent), f32c(weights), tuple(f32c(q) for q in dots)
        li = label_index
        require_hip(obj, *dots, ent, weights, qkey, li.keys, li.rowptr, li.objs)
        ctx.gamma, ctx.li, ctx.v, ctx.col_chunk = float(gamma), li, (v_zero, v_one), col_chunk
        ctx.save_for_backward(ent, weights, qkey, obj, *dots)
        return _mix_mean(obj, dots, ent, weights, gamma, li, qkey, v_zero, v_one)

    @staticmethod
    def backward(ctx, g):
        ent, weights, qkey, obj, *dots = ctx.saved_tensors
        li, (v_zero, v_one), ns = ctx.li, ctx.v, 1 + len(dots)
        (B, D), N, st, esz = obj.shape, ent.shape[0], stream_of(obj), ent.element_size()
        step = min(ctx.col_chunk, N)
        gscale = (g.detach().float().reshape(1) / float(B * N)).contiguous()          # stays on the device: no host synchronisation
        dl = [torch.empty(B * step, dtype=torch.float32, device=obj.device) for _ in range(ns)]       # NS slices, reused by every chunk
        dw = torch.empty(ns, dtype=torch.float32, device=obj.device)
        g_obj, g_ent, g_dots = torch.empty_like(obj), torch.empty_like(ent), [torch.empty_like(q) for q in dots]
        g_tmp = torch.empty(step, D, dtype=torch.float32, device=obj.device)          # a further dot leg's, then the L1 share of g_ent[c0:c1]
        gws = _ws(_ws_bytes("mrg_gemm_workspace_bytes", B, D), obj)
        pre = [(q.t().contiguous(), gws) for q in dots]
        for c0 in range(0, N, step):
            c1 = min(N, c0 + step)
            nc = c1 - c0
            _mix_grad(obj, dots, ent, weights, ctx.gamma, li, qkey, v_zero, v_one, c0, c1, gscale, dl, dw)
            _dot_chunk_bwd(dots[0], ent, dl[1], c0, nc, g_dots[0], g_ent, pre[0], st)
            for k in range(1, ns - 1):
                _dot_chunk_bwd(dots[k], ent, dl[k + 1], c0, nc, g_dots[k], g_ent, pre[k], st, ent_dst=g_tmp)
                g_ent[c0:c1] += g_tmp[:nc]
            call("mrg_transe_dist_bwd", (ctypes.c_void_p(ent.data_ptr() + c0 * D * esz), ptr(obj), ptr(dl[0]), nc, ptr(g_tmp), ptr(g_obj),
                                         1 if c0 > 0 else 0, B, nc, D, st),
                 nbytes=4 * (B * nc + (B + nc) * D), flops=4 * B * nc * D)
            g_ent[c0:c1] += g_tmp[:nc]
        need = ctx.needs_input_grad
        grads = (g_ent, dw, g_obj, *g_dots)
        return (None,) * 6 + tuple(x if need[6 + i] else None for i, x in enumerate(grads))


def sf_mix_bce_all(all_ent, sub_emb, rel_emb, weights, gamma, label_index, subj, rel, label_smooth=0.0, col_chunk=None):
    """The supernet's training loss when the score function is searched (reference models/model_search_lp.py:160-161 with BCELoss over
    the label-smoothed multi-hot labels): the mean over [B, N] of BCELoss(w0 sf_TransE(...) + w1 sf_DisMult(...),
    label_index.labels(subj, rel, label_smooth)) as a float32 scalar with no [B, N] tensor, differentiable in all_ent, sub_emb, rel_emb
    and weights [2] (softmax of the score-function alpha; TransE's weight first).  The backward holds two [B, col_chunk] slices
    (default: half of bce_default_col_chunk(B), so that both stay within its bound), the "dot" slice's transpose and a [col_chunk, D]
    scratch.  label_index: sampler.LabelIndex on the same device.  No host synchronisation."""
    what = "sf_mix_bce_all"
    if (sub_emb.dim() != 2 or sub_emb.shape != rel_emb.shape or all_ent.dim() != 2 or sub_emb.shape[1] != all_ent.shape[1]
            or weights.numel() != 2):
        raise ValueError(f"{what}: all_ent [num_ent, D], sub_emb / rel_emb [B, D] and weights [2] expected")
    _require_cuda(what, (all_ent, sub_emb, rel_emb, weights, subj, rel))
    return _mix_all(what, all_ent, sub_emb, rel_emb, (), weights, gamma, label_index, subj, rel, label_smooth, col_chunk)


def sf_mix3_bce_all(all_ent, sub_emb, rel_emb, hidden, weights, gamma, label_index, subj, rel, label_smooth=0.0, col_chunk=None):
    """sf_mix_bce_all for MixedOp_SF over ['sf_TransE', 'sf_DisMult', 'sf_ConvE']: the mean over [B, N] of BCELoss((w0 sf_TransE(...) +
    w1 sf_DisMult(...)) + w2 sigmoid(hidden all_ent^T), label_index.labels(subj, rel, label_smooth)) as a float32 scalar with no [B, N]
    tensor, differentiable in all_ent, sub_emb, rel_emb, hidden and weights [3].  hidden [B, D]: sf_ConvE_op.query(sub_emb, rel_emb), the
    row after BN2 + ReLU, formed ONCE per step by the caller (it draws ConvE's dropout masks and updates its BatchNorm statistics); the
    ConvE parameters receive their gradient through it.  The backward holds three [B, col_chunk] slices (default: a third of
    bce_default_col_chunk(B), so that the three stay within its bound), one "dot" slice's transpose at a time and a [col_chunk, D]
    scratch.  label_index: sampler.LabelIndex on the same device.  No host synchronisation."""
    what = "sf_mix3_bce_all"
    if (sub_emb.dim() != 2 or sub_emb.shape != rel_emb.shape or hidden.shape != sub_emb.shape or all_ent.dim() != 2
            or sub_emb.shape[1] != all_ent.shape[1] or weights.numel() != 3):
        raise ValueError(f"{what}: all_ent [num_ent, D], sub_emb / rel_emb / hidden [B, D] and weights [3] expected")
    _require_cuda(what, (all_ent, sub_emb, rel_emb, hidden, weights, subj, rel))
    return _mix_all(what, all_ent, sub_emb, rel_emb, (hidden,), weights, gamma, label_index, subj, rel, label_smooth, col_chunk)


def _mix_all(what, all_ent, sub_emb, rel_emb, more_dots, weights, gamma, label_index, subj, rel, label_smooth, col_chunk):
    """The checked front ends' common tail; more_dots: the dot operands after sub * rel."""
    ns = 2 + len(more_dots)
    B, N = int(sub_emb.shape[0]), int(all_ent.shape[0])
    if col_chunk is None:
        col_chunk = max(1, bce_default_col_chunk(B) // ns)
    qkey, v_zero, v_one, col_chunk = _bce_all_args(what, (), B, N, label_index, subj, rel, label_smooth, col_chunk)
    return _MixBCE1N.apply(gamma, label_index, qkey, v_zero, v_one, col_chunk, all_ent, weights.reshape(ns),
                           compose("add", sub_emb, rel_emb), compose("mult", sub_emb, rel_emb), *more_dots)
