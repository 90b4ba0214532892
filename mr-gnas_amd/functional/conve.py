"""ConvE feature path: (subject, relation) rows -> the hidden vector in front of BN2 (csrc/conve.hip; reference
models/operations_lp.py:150-205 sf_ConvE_op, models/compgcn.py:188-269 CompGCN_ConvE).

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h): every Function enqueues HIP kernels of
libmrgnas_hip.so on torch's current stream through ctypes; every call site states the algorithmic bytes / flops of the launch.

    img = layout(sub, rel) [B, 1, Hi, Wi]     x0 = BN0(img)     z = conv(x0, Wc) + bc     a = keep1 * relu(BN1(z))
    h   = keep2 * (a.view(B, -1) @ Wfc^T + bfc)

STACKED is sf_ConvE_op's image (sub then rel, 2 k_h x k_w), INTERLEAVED CompGCN_ConvE's (sub and rel alternating, 2 k_w x k_h).
BN2, the ReLU and the score product stay on the MixedOp epilogue and the row GEMM (the callers in operations_lp / compgcn).
"""
import torch

from .. import _lib
from .. import lazy as LZ
from .._lib import call, f32c, ptr, require_hip, stream_of
from ._base import _ws, _ws_bytes, bump_counters

STACKED, INTERLEAVED = 0, 1        # MRG_CONVE_STACKED / MRG_CONVE_INTERLEAVED
MAX_D, MAX_KS = 1024, 15           # MRG_CONVE_MAX_D / MRG_CONVE_MAX_KS


class _Cfg:
    """What the Function needs besides its differentiable inputs: the layout and shapes, the BatchNorm modules (running statistics
    updated in place) and their mode."""

    def __init__(self, layout, Hi, Wi, ks, bn0, bn1, training):
        self.layout, self.Hi, self.Wi, self.ks, self.bn0, self.bn1, self.training = layout, Hi, Wi, ks, bn0, bn1, training


class _ConvEFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, sub, rel, w0, b0, Wc, bc, w1, b1, Wfc, bfc, keep1, keep2):
        sub, rel = f32c(sub), f32c(rel)
        Wc, Wfc = f32c(Wc), f32c(Wfc)
        require_hip(sub, rel, w0, b0, Wc, bc, w1, b1, Wfc, bfc, keep1, keep2)
        B, D = sub.shape
        F, ks = Wc.shape[0], cfg.ks
        Ho, Wo = cfg.Hi - ks + 1, cfg.Wi - ks + 1
        P = Ho * Wo
        K = F * P
        dev, st = sub.device, stream_of(sub)
        tr = int(cfg.training)
        bn0, bn1 = cfg.bn0, cfg.bn1
        stats0 = torch.empty(2, dtype=torch.float32, device=dev)
        stats1 = torch.empty(2 * F, dtype=torch.float32, device=dev)
        call("mrg_conve_bn0_fwd", (ptr(sub), ptr(rel), B, D, ptr(bn0.running_mean), ptr(bn0.running_var), tr, bn0.eps,
                                   float(bn0.momentum), ptr(stats0), st), nbytes=8 * B * D * (2 if tr else 0))
        z = torch.empty(B, K, dtype=torch.float32, device=dev)
        call("mrg_conve_conv_fwd", (cfg.layout, ptr(sub), ptr(rel), B, D, cfg.Hi, cfg.Wi, ptr(stats0), ptr(w0), ptr(b0), ptr(Wc), ptr(bc),
                                    F, ks, ptr(z), st), nbytes=4 * (2 * B * D + F * ks * ks + B * K), flops=2 * B * K * ks * ks)
        a = torch.empty(B, K, dtype=torch.float32, device=dev)
        call("mrg_conve_bn1_fwd", (ptr(z), B, F, P, ptr(w1), ptr(b1), ptr(bn1.running_mean), ptr(bn1.running_var), ptr(keep1), tr,
                                   bn1.eps, float(bn1.momentum), ptr(stats1), ptr(a), st),
             nbytes=4 * B * K * ((3 if tr else 1) + 1 + (keep1 is not None)))
        if tr:
            bump_counters([bn0, bn1])
        h = torch.empty(B, D, dtype=torch.float32, device=dev)
        ws = _ws(_ws_bytes("mrg_conve_fc_workspace_bytes", B, K, D), sub)
        call("mrg_conve_fc_fwd", (ptr(a), ptr(Wfc), ptr(bfc), ptr(keep2), ptr(h), ptr(ws), B, K, D, st),
             nbytes=4 * (B * K + D * K + B * D), flops=2 * B * K * D)
        ctx.cfg, ctx.has_bc, ctx.has_bfc = cfg, bc is not None, bfc is not None
        ctx.save_for_backward(sub, rel, w0, b0, Wc, w1, Wfc, keep1, keep2, stats0, stats1, z, a)
        return h

    @staticmethod
    def backward(ctx, gh):
        sub, rel, w0, b0, Wc, w1, Wfc, keep1, keep2, stats0, stats1, z, a = ctx.saved_tensors
        cfg = ctx.cfg
        gh = f32c(gh)
        require_hip(gh)
        B, D = sub.shape
        F, ks = Wc.shape[0], cfg.ks
        P = (cfg.Hi - ks + 1) * (cfg.Wi - ks + 1)
        K = F * P
        dev, st = sub.device, stream_of(sub)
        tr = int(cfg.training)
        g = torch.empty(B, K, dtype=torch.float32, device=dev)
        gWfc = torch.empty_like(Wfc)
        gbfc = torch.empty(D, dtype=torch.float32, device=dev) if ctx.has_bfc else None
        ws = _ws(_ws_bytes("mrg_conve_fc_workspace_bytes", B, K, D), sub)
        call("mrg_conve_fc_bwd", (ptr(gh), ptr(keep2), ptr(a), ptr(Wfc), ptr(g), ptr(gWfc), ptr(gbfc), ptr(ws), B, K, D, st),
             nbytes=4 * (2 * B * K + 2 * D * K + 3 * B * D), flops=4 * B * K * D)
        gw1 = torch.empty(F, dtype=torch.float32, device=dev)
        gb1 = torch.empty(F, dtype=torch.float32, device=dev)
        call("mrg_conve_bn1_bwd", (ptr(g), ptr(z), ptr(a), ptr(keep1), ptr(stats1), ptr(w1), tr, B, F, P, ptr(gw1), ptr(gb1), st),
             nbytes=4 * B * K * (7 + 2 * (keep1 is not None)))
        wsb = _ws(_ws_bytes("mrg_conve_bwd_workspace_bytes", B, D, F, ks), sub)
        call("mrg_conve_conv_bwd", (cfg.layout, ptr(sub), ptr(rel), B, D, cfg.Hi, cfg.Wi, ptr(stats0), ptr(w0), ptr(b0), ptr(Wc), F, ks,
                                    ptr(g), ptr(wsb), st), nbytes=4 * (2 * B * K + 4 * B * D), flops=4 * B * K * ks * ks)
        gsub, grel = torch.empty_like(sub), torch.empty_like(rel)
        gw0 = torch.empty(1, dtype=torch.float32, device=dev)
        gb0 = torch.empty(1, dtype=torch.float32, device=dev)
        gWc = torch.empty_like(Wc)
        gbc = torch.empty(F, dtype=torch.float32, device=dev) if ctx.has_bc else None
        call("mrg_conve_finish_bwd", (cfg.layout, ptr(sub), ptr(rel), B, D, F, ks, ptr(stats0), ptr(w0), tr, ptr(wsb), ptr(gsub), ptr(grel),
                                      ptr(gw0), ptr(gb0), ptr(gWc), ptr(gbc), st), nbytes=4 * 8 * B * D)
        return None, gsub, grel, gw0, gb0, gWc, gbc, gw1, gb1, gWfc, gbfc, None, None


def drop_masks(feature_drop, hidden_drop, B, F, Ho, Wo, D, device):
    """The two dropout masks torch's formulation draws, in its order (the feature mask [B, F, Ho, Wo] first, then the hidden
    mask [B, D]), as the modules' own nn.Dropout applied to ones; None when not training or p == 0."""
    def mask(drop, shape):
        if not drop.training or drop.p == 0:
            return None
        return drop(torch.ones(shape, dtype=torch.float32, device=device))
    keep1 = mask(feature_drop, (B, F, Ho, Wo))
    keep2 = mask(hidden_drop, (B, D))
    return keep1, keep2


def conve_features(sub, rel, layout, img_hw, bn0, conv, bn1, keep1, fc, keep2):
    """keep2 * fc(keep1 * relu(bn1(conv(bn0(layout(sub, rel)))))) of [B, D] float32 HIP rows: the [B, D] hidden vector in front of
    BN2.  img_hw = (Hi, Wi) of the image (Hi * Wi == 2 D); keep1 [B, F, Ho, Wo] / keep2 [B, D]: dropout masks (already scaled) or None.
    The BatchNorms must track running statistics with a float momentum (the callers check; torch's formulation otherwise)."""
    sub, rel = LZ.real(sub), LZ.real(rel)
    B, D = sub.shape
    Hi, Wi = img_hw
    F, ks = conv.weight.shape[0], conv.weight.shape[-1]
    if rel.shape != sub.shape:
        raise _lib.MrgnasError(f"conve: subject rows {tuple(sub.shape)} and relation rows {tuple(rel.shape)} differ")
    if Hi * Wi != 2 * D or not 1 <= D <= MAX_D or not 1 <= ks <= min(MAX_KS, Hi, Wi) or tuple(conv.weight.shape[1:]) != (1, ks, ks):
        raise _lib.MrgnasError(f"conve: image {Hi} x {Wi}, width {D}, kernel {tuple(conv.weight.shape)} not covered")
    K = F * (Hi - ks + 1) * (Wi - ks + 1)
    if fc.weight.shape[1] != K:
        raise _lib.MrgnasError(f"conve: fc takes {fc.weight.shape[1]} inputs, the conv gives {K}")
    if keep1 is not None:
        keep1 = f32c(keep1).reshape(B, K)
    if keep2 is not None:
        keep2 = f32c(keep2)
    cfg = _Cfg(layout, Hi, Wi, ks, bn0, bn1, bn0.training)
    return _ConvEFeatures.apply(cfg, sub, rel, bn0.weight, bn0.bias, conv.weight, conv.bias, bn1.weight, bn1.bias, fc.weight, fc.bias,
                                keep1, keep2)


def _hooked(m):
    return bool(m._forward_hooks or m._forward_pre_hooks or getattr(m, "_forward_hooks_with_kwargs", None)
                or getattr(m, "_forward_pre_hooks_with_kwargs", None))


def hip_path_ok(modules, bns, tensors):
    """Does a ConvE scorer run on the library?  Float32 HIP operands, autocast off, no forward (pre-)hooks on the scorer's submodules
    (the module_linear rule: the library bypasses their __call__), and BatchNorms that track running statistics with a float momentum
    and are all in the same mode.  Otherwise the caller runs torch's formulation."""
    if torch.is_autocast_enabled():
        return False
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return False
    if any(_hooked(m) for m in modules):
        return False
    return all(b.track_running_stats and b.affine and isinstance(b.momentum, float) and b.training == bns[0].training for b in bns)


def conve_query(sub, rel, layout, img_hw, bn0, conv, bn1, feature_drop, fc, hidden_drop, bn2, one):
    """relu(bn2(conve_features(...))) [B, D]: the row every entity is scored against -- the ConvE scorer up to its [B, N] product, BN2 +
    ReLU on the one-branch MixedOp epilogue.  Draws the dropout masks and updates the BatchNorm statistics as conve_scores does."""
    from .mixed import mixed_epilogue
    sub, rel = LZ.real(sub), LZ.real(rel)
    B, D = sub.shape
    if bn2.training and B == 1:                       # what F.batch_norm raises for BatchNorm1d on one row
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([B, D])}")
    Hi, Wi = img_hw
    F, ks = conv.weight.shape[0], conv.weight.shape[-1]
    keep1, keep2 = drop_masks(feature_drop, hidden_drop, B, F, Hi - ks + 1, Wi - ks + 1, D, sub.device)
    h = conve_features(sub, rel, layout, img_hw, bn0, conv, bn1, keep1, fc, keep2)
    return mixed_epilogue([h], [bn2], one if one.device == h.device else one.to(h.device))


def conve_scores(sub, rel, layout, img_hw, bn0, conv, bn1, feature_drop, fc, hidden_drop, bn2, one, ent, bias):
    """sigmoid(conve_query(...) @ ent^T + bias): the whole ConvE scorer, the [B, N] product on the row GEMM (what distmult_scores_all
    runs)."""
    from .row_linear import linear
    x = conve_query(sub, rel, layout, img_hw, bn0, conv, bn1, feature_drop, fc, hidden_drop, bn2, one)
    return linear(x, LZ.real(ent), bias, "sigmoid")
