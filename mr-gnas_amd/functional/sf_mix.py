"""The score-function search leg: the 1-N loss under the MIXED score of MixedOp_SF over SF_OPS = ['sf_TransE', 'sf_DisMult'] without a
[B, N] tensor (csrc/sf_mix_1n.hip; reference models/cell_lp.py:36-50, models/model_search_lp.py:160-161).

    p[b, e] = w0 * sigmoid(gamma - ||sub_b + rel_b - ent_e||_1) + w1 * sigmoid((sub_b * rel_b) . ent_e)

BCE(w0 p0 + w1 p1, y) is no function of BCE(p0, y) and BCE(p1, y), so this is one sweep that forms both scores of every (query, entity)
pair from the same staged rows -- not a composition of the fixed-genotype losses of functional.scoring.

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h): every Function enqueues HIP kernels of
libmrgnas_hip.so on torch's current stream through ctypes; every call site states the algorithmic bytes / flops of the launch."""
import ctypes

import torch

from .._lib import call, f32c, ptr, require_hip, stream_of
from ._base import _ws, _ws_bytes
from .compose_gather import compose
from .scoring import _bce_all_args, _checked_ws, _dot_chunk_bwd, _require_cuda, bce_default_col_chunk

_WS = "mrg_sfmix_bce_workspace_bytes"


def _labels(li, qkey):
    return ptr(qkey), ptr(li.keys), ptr(li.rowptr), ptr(li.objs), int(li.keys.numel())


def sf_mix_bce_mean(obj, qd, ent, weights, gamma, label_index, qkey, v_zero, v_one):
    """mrg_sfmix_bce_fwd, no autograd: the mean over [B, N] of BCE(w0 sigmoid(gamma - ||obj - ent||_1) + w1 sigmoid(qd ent^T), labels) as
    a float32 device scalar.  obj = sub + rel and qd = sub * rel [B, D]; weights [2] float32 on the device (TransE's first)."""
    obj, qd, ent, weights = f32c(obj), f32c(qd), f32c(ent), f32c(weights)
    require_hip(obj, qd, ent, weights, qkey)
    (B, D), N = obj.shape, ent.shape[0]
    loss = torch.empty((), dtype=torch.float32, device=obj.device)
    ws, nbytes = _checked_ws(_WS, B, N, D, obj)
    call("mrg_sfmix_bce_fwd", (ptr(obj), ptr(qd), ptr(ent), ptr(weights), *_labels(label_index, qkey), float(gamma), v_zero, v_one, B, N, D,
                               ptr(loss), ptr(ws), nbytes, stream_of(obj)),
         nbytes=4 * (2 * B + N) * D, flops=5 * B * N * D)
    return loss


def sf_mix_bce_grad(obj, qd, ent, weights, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, dl0=None, dl1=None, dw=None):
    """mrg_sfmix_bce_grad, no autograd: (dl0, dl1, dw) for the entities [c0, c1): the loss gradient with respect to gamma - dist and to
    the dot product as [B, c1 - c0] each (written into the first B * (c1 - c0) floats of dl0 / dl1 when given), and the gradient with
    respect to the two weights, written to dw [2] when c0 == 0 and added to it otherwise.  gscale: float32 [1] on the device."""
    (B, D), N, nc = obj.shape, ent.shape[0], c1 - c0
    dl0 = torch.empty(B * nc, dtype=torch.float32, device=obj.device) if dl0 is None else dl0
    dl1 = torch.empty(B * nc, dtype=torch.float32, device=obj.device) if dl1 is None else dl1
    dw = torch.zeros(2, dtype=torch.float32, device=obj.device) if dw is None else dw
    ws, nbytes = _checked_ws(_WS, B, nc, D, obj)
    call("mrg_sfmix_bce_grad", (ptr(obj), ptr(qd), ptr(ent), ptr(weights), *_labels(label_index, qkey), float(gamma), v_zero, v_one, B, N, D,
                                c0, c1, ptr(gscale), ptr(dl0), ptr(dl1), ptr(dw), ptr(ws), nbytes, stream_of(obj)),
         nbytes=4 * (2 * B + nc) * D + 8 * B * nc, flops=5 * B * nc * D)
    return dl0[:B * nc].view(B, nc), dl1[:B * nc].view(B, nc), dw


class _MixBCE1N(torch.autograd.Function):
    """loss(obj, qd, ent, weights).  Forward: one sweep that stores nothing per element.  Backward, per column chunk: the two gradient
    slices dl0 / dl1 [B, chunk] and the chunk's share of dw (mrg_sfmix_bce_grad, the tile recomputed), the "dot" work on dl1
    (scoring._dot_chunk_bwd: the qd gradient and g_ent[c0:c1]) and the "l1" work on dl0 (mrg_transe_dist_bwd: g_obj accumulated in
    chunk order, its entity half into a [chunk, D] scratch that is added to g_ent[c0:c1])."""

    @staticmethod
    def forward(ctx, gamma, obj, qd, ent, weights, label_index, qkey, v_zero, v_one, col_chunk):
        obj, qd, ent, weights = f32c(obj), f32c(qd), f32c(ent), f32c(weights)
        li = label_index
        require_hip(obj, qd, ent, weights, qkey, li.keys, li.rowptr, li.objs)
        ctx.gamma, ctx.li, ctx.v, ctx.col_chunk = float(gamma), li, (v_zero, v_one), col_chunk
        ctx.save_for_backward(obj, qd, ent, weights, qkey)
        return sf_mix_bce_mean(obj, qd, ent, weights, gamma, li, qkey, v_zero, v_one)

    @staticmethod
    def backward(ctx, g):
        obj, qd, ent, weights, qkey = ctx.saved_tensors
        li, (v_zero, v_one) = ctx.li, ctx.v
        (B, D), N, st, esz = obj.shape, ent.shape[0], stream_of(obj), ent.element_size()
        step = min(ctx.col_chunk, N)
        gscale = (g.detach().float().reshape(1) / float(B * N)).contiguous()          # stays on the device: no host synchronisation
        dl0 = torch.empty(B * step, dtype=torch.float32, device=obj.device)            # TWO slices, reused by every chunk
        dl1 = torch.empty(B * step, dtype=torch.float32, device=obj.device)
        dw = torch.empty(2, dtype=torch.float32, device=obj.device)
        g_obj, g_qd, g_ent = torch.empty_like(obj), torch.empty_like(qd), torch.empty_like(ent)
        g_l1 = torch.empty(step, D, dtype=torch.float32, device=obj.device)            # the L1 half of g_ent[c0:c1]
        pre = qd.t().contiguous(), _ws(_ws_bytes("mrg_gemm_workspace_bytes", B, D), qd)
        for c0 in range(0, N, step):
            c1 = min(N, c0 + step)
            nc = c1 - c0
            sf_mix_bce_grad(obj, qd, ent, weights, ctx.gamma, li, qkey, v_zero, v_one, c0, c1, gscale, dl0, dl1, dw)
            _dot_chunk_bwd(qd, ent, dl1, c0, nc, g_qd, g_ent, pre, st)
            call("mrg_transe_dist_bwd", (ctypes.c_void_p(ent.data_ptr() + c0 * D * esz), ptr(obj), ptr(dl0), nc, ptr(g_l1), ptr(g_obj),
                                         1 if c0 > 0 else 0, B, nc, D, st),
                 nbytes=4 * (B * nc + (B + nc) * D), flops=4 * B * nc * D)
            g_ent[c0:c1] += g_l1[:nc]
        need = ctx.needs_input_grad
        return (None, g_obj if need[1] else None, g_qd if need[2] else None, g_ent if need[3] else None, dw if need[4] else None,
                None, None, None, None, None)


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
    B, N = int(sub_emb.shape[0]), int(all_ent.shape[0])
    if col_chunk is None:
        col_chunk = max(1, bce_default_col_chunk(B) // 2)
    qkey, v_zero, v_one, col_chunk = _bce_all_args(what, (), B, N, label_index, subj, rel, label_smooth, col_chunk)
    return _MixBCE1N.apply(gamma, compose("add", sub_emb, rel_emb), compose("mult", sub_emb, rel_emb), all_ent, weights.reshape(2),
                           label_index, qkey, v_zero, v_one, col_chunk)


# ---- three scorers: ['sf_TransE', 'sf_DisMult', 'sf_ConvE'] (csrc/sf_mix3_1n.hip) -----------------------------------------------------------
#     p[b, e] = (w0 * sigmoid(gamma - ||sub_b + rel_b - ent_e||_1) + w1 * sigmoid((sub_b * rel_b) . ent_e)) + w2 * sigmoid(hidden_b . ent_e)
# hidden = sf_ConvE_op.query(sub_emb, rel_emb), the [B, D] row after BN2 + ReLU: the ConvE parameters get their gradient through it.
_WS3 = "mrg_sfmix3_bce_workspace_bytes"


def sf_mix3_bce_mean(obj, qd, qh, ent, weights, gamma, label_index, qkey, v_zero, v_one):
    """mrg_sfmix3_bce_fwd, no autograd: the mean over [B, N] of BCE((w0 sigmoid(gamma - ||obj - ent||_1) + w1 sigmoid(qd ent^T)) +
    w2 sigmoid(qh ent^T), labels) as a float32 device scalar.  obj = sub + rel, qd = sub * rel and qh = ConvE's hidden rows [B, D];
    weights [3] float32 on the device (TransE's, DistMult's, ConvE's)."""
    obj, qd, qh, ent, weights = f32c(obj), f32c(qd), f32c(qh), f32c(ent), f32c(weights)
    require_hip(obj, qd, qh, ent, weights, qkey)
    (B, D), N = obj.shape, ent.shape[0]
    loss = torch.empty((), dtype=torch.float32, device=obj.device)
    ws, nbytes = _checked_ws(_WS3, B, N, D, obj)
    call("mrg_sfmix3_bce_fwd", (ptr(obj), ptr(qd), ptr(qh), ptr(ent), ptr(weights), *_labels(label_index, qkey), float(gamma), v_zero, v_one,
                                B, N, D, ptr(loss), ptr(ws), nbytes, stream_of(obj)),
         nbytes=4 * (3 * B + N) * D, flops=7 * B * N * D)
    return loss


def sf_mix3_bce_grad(obj, qd, qh, ent, weights, gamma, label_index, qkey, v_zero, v_one, c0, c1, gscale, dl0=None, dl1=None, dl2=None,
                     dw=None):
    """mrg_sfmix3_bce_grad, no autograd: (dl0, dl1, dl2, dw) for the entities [c0, c1): the loss gradient with respect to gamma - dist,
    to the DistMult dot product and to the ConvE dot product as [B, c1 - c0] each (written into the first B * (c1 - c0) floats of dl0 /
    dl1 / dl2 when given), and the gradient with respect to the three weights, written to dw [3] when c0 == 0 and added to it
    otherwise.  gscale: float32 [1] on the device."""
    (B, D), N, nc = obj.shape, ent.shape[0], c1 - c0
    dl0, dl1, dl2 = (torch.empty(B * nc, dtype=torch.float32, device=obj.device) if d is None else d for d in (dl0, dl1, dl2))
    dw = torch.zeros(3, dtype=torch.float32, device=obj.device) if dw is None else dw
    ws, nbytes = _checked_ws(_WS3, B, nc, D, obj)
    call("mrg_sfmix3_bce_grad", (ptr(obj), ptr(qd), ptr(qh), ptr(ent), ptr(weights), *_labels(label_index, qkey), float(gamma), v_zero, v_one,
                                 B, N, D, c0, c1, ptr(gscale), ptr(dl0), ptr(dl1), ptr(dl2), ptr(dw), ptr(ws), nbytes, stream_of(obj)),
         nbytes=4 * (3 * B + nc) * D + 12 * B * nc, flops=7 * B * nc * D)
    return dl0[:B * nc].view(B, nc), dl1[:B * nc].view(B, nc), dl2[:B * nc].view(B, nc), dw


class _Mix3BCE1N(torch.autograd.Function):
    """loss(obj, qd, qh, ent, weights).  Forward: one sweep that stores nothing per element.  Backward, per column chunk: ONE
    mrg_sfmix3_bce_grad into three reused slices dl0 / dl1 / dl2 [B, chunk] with the chunk's share of dw; the "dot" work on dl1 with qd
    (scoring._dot_chunk_bwd: g_qd accumulated, g_ent[c0:c1] written); the same work on dl2 with qh, its entity half into a [chunk, D]
    scratch that is added to g_ent[c0:c1]; the "l1" work on dl0 (mrg_transe_dist_bwd), its entity half through the same scratch.
    g_ent[c0:c1] = (DistMult's + ConvE's) + TransE's, in that order on one stream: bit-repeatable."""

    @staticmethod
    def forward(ctx, gamma, obj, qd, qh, ent, weights, label_index, qkey, v_zero, v_one, col_chunk):
        obj, qd, qh, ent, weights = f32c(obj), f32c(qd), f32c(qh), f32c(ent), f32c(weights)
        li = label_index
        require_hip(obj, qd, qh, ent, weights, qkey, li.keys, li.rowptr, li.objs)
        ctx.gamma, ctx.li, ctx.v, ctx.col_chunk = float(gamma), li, (v_zero, v_one), col_chunk
        ctx.save_for_backward(obj, qd, qh, ent, weights, qkey)
        return sf_mix3_bce_mean(obj, qd, qh, ent, weights, gamma, li, qkey, v_zero, v_one)

    @staticmethod
    def backward(ctx, g):
        obj, qd, qh, ent, weights, qkey = ctx.saved_tensors
        li, (v_zero, v_one) = ctx.li, ctx.v
        (B, D), N, st, esz = obj.shape, ent.shape[0], stream_of(obj), ent.element_size()
        step = min(ctx.col_chunk, N)
        gscale = (g.detach().float().reshape(1) / float(B * N)).contiguous()          # stays on the device: no host synchronisation
        dl0, dl1, dl2 = (torch.empty(B * step, dtype=torch.float32, device=obj.device) for _ in range(3))    # reused by every chunk
        dw = torch.empty(3, dtype=torch.float32, device=obj.device)
        g_obj, g_qd, g_qh, g_ent = torch.empty_like(obj), torch.empty_like(qd), torch.empty_like(qh), torch.empty_like(ent)
        g_tmp = torch.empty(step, D, dtype=torch.float32, device=obj.device)          # ConvE's, then the L1 share of g_ent[c0:c1]
        gws = _ws(_ws_bytes("mrg_gemm_workspace_bytes", B, D), qd)
        pre_d, pre_h = (qd.t().contiguous(), gws), (qh.t().contiguous(), gws)
        for c0 in range(0, N, step):
            c1 = min(N, c0 + step)
            nc = c1 - c0
            sf_mix3_bce_grad(obj, qd, qh, ent, weights, ctx.gamma, li, qkey, v_zero, v_one, c0, c1, gscale, dl0, dl1, dl2, dw)
            _dot_chunk_bwd(qd, ent, dl1, c0, nc, g_qd, g_ent, pre_d, st)
            _dot_chunk_bwd(qh, ent, dl2, c0, nc, g_qh, g_ent, pre_h, st, ent_dst=g_tmp)
            g_ent[c0:c1] += g_tmp[:nc]
            call("mrg_transe_dist_bwd", (ctypes.c_void_p(ent.data_ptr() + c0 * D * esz), ptr(obj), ptr(dl0), nc, ptr(g_tmp), ptr(g_obj),
                                         1 if c0 > 0 else 0, B, nc, D, st),
                 nbytes=4 * (B * nc + (B + nc) * D), flops=4 * B * nc * D)
            g_ent[c0:c1] += g_tmp[:nc]
        need = ctx.needs_input_grad
        return (None, g_obj if need[1] else None, g_qd if need[2] else None, g_qh if need[3] else None, g_ent if need[4] else None,
                dw if need[5] else None, None, None, None, None, None)


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
    B, N = int(sub_emb.shape[0]), int(all_ent.shape[0])
    if col_chunk is None:
        col_chunk = max(1, bce_default_col_chunk(B) // 3)
    qkey, v_zero, v_one, col_chunk = _bce_all_args(what, (), B, N, label_index, subj, rel, label_smooth, col_chunk)
    return _Mix3BCE1N.apply(gamma, compose("add", sub_emb, rel_emb), compose("mult", sub_emb, rel_emb), hidden, all_ent,
                            weights.reshape(3), label_index, qkey, v_zero, v_one, col_chunk)
