"""Restatements for top-k link prediction (csrc/topk.hip, csrc/transe_1n.hip L1_TOPK, evaluation.query_topk / predict_topk), shared by
test_topk_cpu.py and test_topk_gpu.py.  Plain torch in float64 on the CPU; no kernel of the library is called here."""
import torch

import l1_ref as L1


def allowed_mask(N, qkey, when, keys, rowptr, members, gone_at):
    """bool [Q, N]: candidate e of query i is NOT filtered.  mrr_ref.allowed_mask without a target: a member of the list of qkey[i] is
    filtered iff gone_at > when[i]; a key of -1 or an unknown key filters nothing; nothing is exempt."""
    Q = qkey.numel()
    ok = torch.ones(Q, N, dtype=torch.bool)
    if keys is None or keys.numel() == 0:
        return ok
    pos = torch.searchsorted(keys, qkey.clamp(min=0))
    for i in range(Q):
        u = int(pos[i])
        if int(qkey[i]) < 0 or u >= keys.numel() or int(keys[u]) != int(qkey[i]):
            continue
        lo, hi = int(rowptr[u]), int(rowptr[u + 1])
        ok[i, members[lo:hi][gone_at[lo:hi] > int(when[i])].long()] = False
    return ok


def scores64(kind, q, ent):
    """[Q, N] float64: the logits q ent^T ("dot") or the distances ||q - ent[e]||_1 ("l1")."""
    return q.double() @ ent.double().T if kind == "dot" else L1.dist64(q, ent)


def topk64(kind, x, allowed, k):
    """(ids [Q, k] int64, values [Q, k] float64) of exact scores x [Q, N]: the allowed entities sorted by (-score, id) for "dot" and by
    (distance, id) for "l1", cut to k; the tail beyond the allowed entities is id -1 with value -inf / +inf."""
    Q, N = x.shape
    key = (-x if kind == "dot" else x).clone()
    assert bool(torch.isfinite(key).all())
    key[~allowed] = float("inf")
    order = torch.argsort(key, dim=1, stable=True)             # stable: equal keys keep ascending ids
    pad = float("-inf") if kind == "dot" else float("inf")
    ids = torch.full((Q, k), -1, dtype=torch.int64)
    vals = torch.full((Q, k), pad, dtype=torch.float64)
    m = min(k, N)
    valid = torch.arange(m).unsqueeze(0) < allowed.sum(dim=1, keepdim=True)
    ids[:, :m] = torch.where(valid, order[:, :m], ids[:, :m])
    vals[:, :m] = torch.where(valid, x.gather(1, order[:, :m]), vals[:, :m])
    return ids, vals


def delta64(kind, q, ent):
    """[Q, 1]: the distance within which a float32 score of the kernels lies of the float64 one and within which two scores may swap --
    the delta of l1_ref.rows_rank_band ("dot") / l1_ref.l1_rank_band ("l1")."""
    D = ent.shape[1]
    if kind == "dot":
        return (3 * D * 2.0 ** -24 * (q.double().abs() @ ent.double().abs().T).max(dim=1).values).unsqueeze(1)
    return 2 * L1.chain_bound(D, L1.dist64(q, ent).max(dim=1, keepdim=True).values)


def position_band(kind, q, ent, ids, allowed):
    """(lo, hi) [Q, k]: the admissible positions (1-based) of entity ids[:, j] in a float32 list -- l1_ref.rows_rank_band /
    l1_ref.l1_rank_band with that entity as the target.  Columns with id -1 are computed for entity 0 and are to be masked."""
    lo, hi = [], []
    x = None if kind == "dot" else L1.dist64(q, ent)
    for j in range(ids.shape[1]):
        t = ids[:, j].clamp(min=0)
        a, b = L1.rows_rank_band(q, ent, t, allowed) if kind == "dot" else L1.l1_rank_band(x, t, allowed, ent.shape[1])
        lo.append(a)
        hi.append(b)
    return torch.stack(lo, 1), torch.stack(hi, 1)
