"""Restatements for the score-function search leg (csrc/sf_mix_1n.hip, functional.sf_mix_bce_all, cell_lp.MixedOp_SF.loss_1n,
supernet.ScoreSearchNetwork, evaluation.mix_ranks / predict_mix), shared by test_sf_mix_cpu.py and test_sf_mix_gpu.py.  Plain torch on
whatever device the operands live on; no kernel of the library is called here."""
import torch
import torch.nn as nn

ROWS = 64           # row blocks bound the [rows, N, D] intermediate of the L1 distance


def scores64(ent, sub, relb, gamma):
    """(x0, x1) [B, N] in float64: x0 = gamma - ||obj - ent||_1 and x1 = qd . ent, starting from obj = float32(sub + rel) and
    qd = float32(sub * rel) as the kernels see them (l1_ref.transe_loss64 explains why for obj)."""
    e = ent.double()
    o, q = (sub.float() + relb.float()).double(), (sub.float() * relb.float()).double()
    x0 = gamma - torch.cat([(o[i:i + ROWS].unsqueeze(1) - e.unsqueeze(0)).abs().sum(-1) for i in range(0, o.shape[0], ROWS)])
    return x0, q @ e.T


def prob64(ent, sub, relb, w, gamma):
    """The mixed probability [B, N] in float64."""
    x0, x1 = scores64(ent, sub, relb, gamma)
    return float(w[0]) * torch.sigmoid(x0) + float(w[1]) * torch.sigmoid(x1)


def mix_loss64(ent, sub, relb, w, y, gamma, upstream=3.0):
    """(loss, g_ent, g_sub, g_rel, g_w) of upstream * mean BCE(w0 sigmoid(x0) + w1 sigmoid(x1), y) in float64.  The gradients of obj and
    qd are taken at their float32 values and carried to sub and rel by the chain rule g_sub = g_obj + g_qd * rel, g_rel = g_obj +
    g_qd * sub.  torch's abs backward has sgn(0) = 0."""
    e = ent.detach().double().requires_grad_(True)
    o = (sub.detach().float() + relb.detach().float()).double().requires_grad_(True)
    q = (sub.detach().float() * relb.detach().float()).double().requires_grad_(True)
    w64 = w.detach().double().reshape(2).clone().requires_grad_(True)
    x0 = gamma - torch.cat([(o[i:i + ROWS].unsqueeze(1) - e.unsqueeze(0)).abs().sum(-1) for i in range(0, o.shape[0], ROWS)])
    p = w64[0] * torch.sigmoid(x0) + w64[1] * torch.sigmoid(q @ e.T)
    y = y.double()
    loss = -(y * torch.log(p) + (1.0 - y) * torch.log1p(-p)).mean()
    (upstream * loss).backward()
    return loss.detach(), e.grad, o.grad + q.grad * relb.detach().double(), o.grad + q.grad * sub.detach().double(), w64.grad


def mix_rank_band(p64, target, allowed, eps):
    """(lo, hi) [Q]: lo = 1 + #(p_e > p_t + eps), hi = 1 + #(p_e >= p_t - eps, e != t), both over the allowed candidates."""
    t = target.long().unsqueeze(1)
    pt = p64.gather(1, t)
    others = allowed & (torch.arange(p64.shape[1], device=p64.device).unsqueeze(0) != t)
    return 1 + ((p64 > pt + eps) & others).sum(dim=1), 1 + ((p64 >= pt - eps) & others).sum(dim=1)


class _TransE(nn.Module):
    """sf_TransE_op as the reference writes it (models/operations_lp.py:101-112), on any device."""

    def __init__(self, args):
        super().__init__()
        self.gamma = args.get('gamma', 40)

    def forward(self, all_ent, sub_emb, rel_emb):
        return torch.sigmoid(self.gamma - torch.norm((sub_emb + rel_emb).unsqueeze(1) - all_ent, p=1, dim=2))


class _DistMult(nn.Module):
    """sf_DisMult_op as the reference writes it (models/operations_lp.py:115-127), on any device."""

    def __init__(self, args):
        super().__init__()

    def forward(self, all_ent, sub_emb, rel_emb):
        return torch.sigmoid(torch.mm(sub_emb * rel_emb, all_ent.transpose(1, 0)))


def cpu_sf_registry():
    """A scorer registry for CPU runs of Cell_SF / ScoreSearchNetwork (the product's scorers have no CPU form)."""
    return {"sf_TransE": _TransE, "sf_DisMult": _DistMult}
