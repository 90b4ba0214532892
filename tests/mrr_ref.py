"""Restatements of the DistMult ranking of mr_gnas_amd.evaluation (calc_mrr / mrg_distmult_rank) on the CPU, shared by
test_mrr_cpu.py and test_mrr_gpu.py.  Everything here works on an index given as plain tensors (keys [U] ascending, rowptr [U + 1],
members, gone_at): the layout of include/mrgnas.h."""
import torch

INT32_MAX = 2 ** 31 - 1


def allowed_mask(N, qkey, when, target, keys, rowptr, members, gone_at):
    """bool [Q, N]: candidate e of query i is NOT filtered.  Filtered iff e is a member of the list of qkey[i] with
    gone_at > when[i], and e is not the target.  qkey None = raw."""
    Q = target.numel()
    ok = torch.ones(Q, N, dtype=torch.bool)
    if qkey is None or keys is None or keys.numel() == 0:
        return ok
    pos = torch.searchsorted(keys, qkey.clamp(min=0))
    for i in range(Q):
        u = int(pos[i])
        if int(qkey[i]) < 0 or u >= keys.numel() or int(keys[u]) != int(qkey[i]):
            continue
        lo, hi = int(rowptr[u]), int(rowptr[u + 1])
        m = members[lo:hi][gone_at[lo:hi] > int(when[i])].long()
        ok[i, m] = False
        ok[i, int(target[i])] = True
    return ok


def exact_ranks(x, target, allowed):
    """rank = 1 + #(greater) + #(equal at a lower entity id) over allowed candidates other than the target; x [Q, N] exact scores."""
    Q, N = x.shape
    ids = torch.arange(N).unsqueeze(0)
    t = target.long().unsqueeze(1)
    xt = x.gather(1, t)
    beats = (x > xt) | ((x == xt) & (ids < t))
    return 1 + (beats & allowed & (ids != t)).sum(dim=1)


def scores64(emb, w, a, r):
    e = emb.double()
    return (e[a.long()] * w.double()[r.long()]) @ e.T


def delta_q(emb, w, a, r):
    """3 * D * 2^-24 * max_e sum_c |q_c emb[e, c]|: the float32 chain bound of two sums of D products times the 1.5 x the header pins
    the split core to."""
    e = emb.double()
    q = e[a.long()] * w.double()[r.long()]
    return 3 * emb.shape[1] * 2.0 ** -24 * (q.abs() @ e.abs().T).max(dim=1).values


def rank_band(emb, w, a, r, target, allowed):
    """(lo, hi) [Q]: every admissible rank of a float32 kernel lies in [1 + #(x > t + delta), #(x >= t - delta)] over the allowed
    candidates (the target is allowed and counts itself in the upper end)."""
    x = scores64(emb, w, a, r)
    d = delta_q(emb, w, a, r).unsqueeze(1)
    xt = x.gather(1, target.long().unsqueeze(1))
    ids = torch.arange(x.shape[1]).unsqueeze(0)
    others = allowed & (ids != target.long().unsqueeze(1))
    lo = 1 + ((x > xt + d) & others).sum(dim=1)
    hi = 1 + ((x >= xt - d) & others).sum(dim=1)
    return lo, hi
