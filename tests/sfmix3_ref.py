"""Restatements for the three-way score-function search leg (csrc/sf_mix_1n.hip, functional.sf_mix3_bce_all, cell_lp.MixedOp_SF.loss_1n
over ['sf_TransE', 'sf_DisMult', 'sf_ConvE'], evaluation.mix_ranks / predict_mix with a hidden operand), shared by test_sf_mix3_cpu.py and
test_sf_mix3_gpu.py.  Plain torch on whatever device the operands live on; no kernel of the library is called here."""
import torch

import sfmix_ref as MX

THREE = ['sf_TransE', 'sf_DisMult', 'sf_ConvE']


def scores64(ent, sub, relb, hidden, gamma):
    """(x0, x1, x2) [B, N] in float64: sfmix_ref.scores64's two and x2 = hidden . ent, hidden at its float32 values."""
    x0, x1 = MX.scores64(ent, sub, relb, gamma)
    return x0, x1, hidden.float().double() @ ent.double().T


def prob64(ent, sub, relb, hidden, w, gamma):
    """The mixed probability [B, N] in float64."""
    x0, x1, x2 = scores64(ent, sub, relb, hidden, gamma)
    return float(w[0]) * torch.sigmoid(x0) + float(w[1]) * torch.sigmoid(x1) + float(w[2]) * torch.sigmoid(x2)


def mix3_loss64(ent, sub, relb, hidden, w, y, gamma, upstream=3.0):
    """(loss, g_ent, g_sub, g_rel, g_hidden, g_w) of upstream * mean BCE(w0 sigmoid(x0) + w1 sigmoid(x1) + w2 sigmoid(x2), y) in float64.
    The gradients of obj and qd are taken at their float32 values and carried to sub and rel by the chain rule, as
    sfmix_ref.mix_loss64 does."""
    e = ent.detach().double().requires_grad_(True)
    o = (sub.detach().float() + relb.detach().float()).double().requires_grad_(True)
    q = (sub.detach().float() * relb.detach().float()).double().requires_grad_(True)
    h = hidden.detach().float().double().requires_grad_(True)
    w64 = w.detach().double().reshape(3).clone().requires_grad_(True)
    x0 = gamma - torch.cat([(o[i:i + MX.ROWS].unsqueeze(1) - e.unsqueeze(0)).abs().sum(-1) for i in range(0, o.shape[0], MX.ROWS)])
    p = w64[0] * torch.sigmoid(x0) + w64[1] * torch.sigmoid(q @ e.T) + w64[2] * torch.sigmoid(h @ e.T)
    y = y.double()
    loss = -(y * torch.log(p) + (1.0 - y) * torch.log1p(-p)).mean()
    (upstream * loss).backward()
    return (loss.detach(), e.grad, o.grad + q.grad * relb.detach().double(), o.grad + q.grad * sub.detach().double(), h.grad, w64.grad)


def conve_args(D, k_h, k_w, ker, filt, drop=0.0):
    return {'embed_dim': int(D), 'k_h': int(k_h), 'k_w': int(k_w), 'ker_sz': int(ker), 'num_filt': int(filt), 'conve_hid_drop': drop,
            'feat_drop': drop}


def cpu_sf_registry():
    """sfmix_ref.cpu_sf_registry plus the package's own sf_ConvE_op, whose torch formulation runs on CPU tensors."""
    from mr_gnas_amd import operations_lp as O
    return {**MX.cpu_sf_registry(), "sf_ConvE": O.sf_ConvE_op}
