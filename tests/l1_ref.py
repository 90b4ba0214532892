"""Restatements for the scorer-general 1-N paths (csrc/transe_1n.hip, mrg_rows_rank, functional.transe_bce_all / dot_bce_all,
evaluation.query_ranks / predict_1n), shared by test_fused_scorers_cpu.py and test_fused_scorers_gpu.py.  Plain torch on whatever
device the operands live on; no kernel of the library is called here."""
import torch
import torch.nn.functional as F


def chain_dist32(obj, ent):
    """dist[b, e] = sum_c |obj[b, c] - ent[e, c]| as the kernels form it: ONE float32 accumulator per pair, c ascending from 0."""
    obj, ent = obj.float(), ent.float()
    acc = torch.zeros(obj.shape[0], ent.shape[0], dtype=torch.float32, device=obj.device)
    for c in range(obj.shape[1]):
        acc += (obj[:, c].unsqueeze(1) - ent[:, c].unsqueeze(0)).abs()
    return acc


def dist64(obj, ent, rows=64):
    """The same distances in float64 (row blocks bound the [rows, N, D] intermediate)."""
    obj, ent = obj.double(), ent.double()
    return torch.cat([(obj[i:i + rows].unsqueeze(1) - ent.unsqueeze(0)).abs().sum(-1) for i in range(0, obj.shape[0], rows)])


def chain_bound(D, dist):
    """|float32 chain - exact| <= (D + 1) 2^-24 dist: D - 1 additions and D subtractions, each within half an ulp of a value <= dist."""
    return (D + 1) * 2.0 ** -24 * dist


def transe_loss64(ent, sub, relb, y, gamma, upstream=3.0):
    """(loss, g_ent, g_sub, g_rel) of upstream * mean BCE(sigmoid(gamma - dist), y) in float64, starting from obj = float32(sub + rel)
    as the kernels see it (the rounding of obj across an entity's coordinate would otherwise flip a sign now and then, and one flipped
    sign is a few percent of a gradient entry).  torch's abs backward has sgn(0) = 0."""
    e = ent.detach().double().requires_grad_(True)
    o = (sub.detach().float() + relb.detach().float()).double().requires_grad_(True)
    x = gamma - torch.cat([(o[i:i + 64].unsqueeze(1) - e.unsqueeze(0)).abs().sum(-1) for i in range(0, o.shape[0], 64)])
    loss = -(y * F.logsigmoid(x) + (1.0 - y) * F.logsigmoid(-x)).mean()
    (upstream * loss).backward()
    return loss.detach(), e.grad, o.grad, o.grad


def l1_rank_band(d64, target, allowed, D):
    """(lo, hi) [Q]: every admissible rank of a float32 chain lies in [1 + #(dist < t - d), 1 + #(dist <= t + d)] over the allowed
    candidates other than the target, d = 2 (D + 1) 2^-24 max_e dist: the sequential-sum bound taken twice, once for the target and
    once for the candidate."""
    t = target.long().unsqueeze(1)
    d = 2 * chain_bound(D, d64.max(dim=1, keepdim=True).values)
    dt = d64.gather(1, t)
    others = allowed & (torch.arange(d64.shape[1], device=d64.device).unsqueeze(0) != t)
    return 1 + ((d64 < dt - d) & others).sum(dim=1), 1 + ((d64 <= dt + d) & others).sum(dim=1)


def rows_rank_band(q, ent, target, allowed):
    """mrr_ref.rank_band restated for given query rows q [Q, D]: x = q ent^T in float64, delta = 3 D 2^-24 max_e sum_c |q_c ent[e, c]|."""
    q, e = q.double(), ent.double()
    x = q @ e.T
    d = (3 * ent.shape[1] * 2.0 ** -24 * (q.abs() @ e.abs().T).max(dim=1).values).unsqueeze(1)
    t = target.long().unsqueeze(1)
    xt = x.gather(1, t)
    others = allowed & (torch.arange(x.shape[1], device=x.device).unsqueeze(0) != t)
    return 1 + ((x > xt + d) & others).sum(dim=1), 1 + ((x >= xt - d) & others).sum(dim=1)
