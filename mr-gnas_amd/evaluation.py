"""Filtered ranking of the fixed-genotype driver on the device (reference train/mr_lp_train.py:269-358).

``filtered_ranks`` is the body of the reference's ``predict`` loop (:290-299) as one HIP kernel
(``mrg_rank_filtered``): instead of a masked copy of the [B, N] score matrix and two full argsorts per batch, one
pass counts, per row, the entries that beat the target.  Ties follow a stable descending sort (the reference's
``torch.argsort`` leaves the order of equal scores unspecified).  ``predict`` / ``combine_results`` mirror the
reference's functions of the same role so a driver can swap them in.

The search driver's evaluation (reference utils/utils_rgcn.py:212-380, search/mr_lp_search.py:258-278) is the second half of the
module: ``calc_mrr`` / ``calc_raw_mrr`` / ``calc_filtered_mrr`` / ``infer_graph`` over ``KnownTriples`` and ``distmult_ranks``
(``mrg_distmult_rank``: the DistMult product as a row GEMM whose epilogue counts; no [Q, N] tensor).

``predict_fused`` (DistMult) and ``predict_1n`` (every scorer with ``query`` / ``score_kind``: DistMult, ConvE, TransE) are ``predict``
without a [B, N] tensor, over ``query_ranks`` (``mrg_rows_rank`` / ``mrg_transe_rank``).  ``distmult_ranks`` and ``query_ranks`` share
their filter side and their call (``_filter_side``, ``_rank_call``); the three ``predict`` passes share their per-batch statistics
vector and their one device -> host copy (``_stats_begin``, ``_batch_stats``, ``_stats_end``).

``query_topk`` / ``predict_topk`` answer (s, r, ?): the k best unfiltered entities per query from the same sweeps
(``mrg_rows_topk`` / ``mrg_transe_topk``), again without a [B, N] tensor.

``mix_ranks`` / ``predict_mix`` are ``query_ranks`` / ``predict_1n`` under the mixed score of the score-function search cell
(``mrg_sfmix_rank`` / ``mrg_sfmix_bce_fwd``, csrc/sf_mix_1n.hip), on embeddings the caller holds.
"""
import torch
import torch.nn.functional as F

from ._lib import MrgnasError, call, check, load, ptr, require_hip, stream_of, f32c


def filtered_ranks(pred, labels, obj):
    """ranks [B] int64 (1-based): position of obj[b] among the entities whose label is zero (plus itself)."""
    pred, labels, obj = f32c(pred), f32c(labels), obj.long().contiguous()
    require_hip(pred, labels, obj)
    B, N = pred.shape
    if labels.shape != pred.shape or obj.numel() != B:
        raise ValueError("filtered_ranks: pred / labels [B, N] and obj [B] expected")
    ranks = torch.empty(B, dtype=torch.int64, device=pred.device)
    call("mrg_rank_filtered", (ptr(pred), ptr(labels), ptr(obj), B, N, ptr(ranks), stream_of(pred)), nbytes=8 * B * N)
    return ranks


_HITS = (1, 3, 10)


def _stats_begin(device):
    """(ks, acc): the hit thresholds and the zeroed float64 device vector [count, mr, mrr, loss, hits@k ...] an evaluation pass adds to."""
    return torch.tensor(_HITS, dtype=torch.float64, device=device), torch.zeros(4 + len(_HITS), dtype=torch.float64, device=device)


def _batch_stats(ranks, loss, ks):
    """One batch's [count, mr, mrr, loss, hits@k ...] from its float64 ranks and its mean loss, on the device."""
    return torch.cat((torch.stack((ranks.new_tensor(float(ranks.numel())), ranks.sum(), ranks.reciprocal().sum(), loss.double())),
                      (ranks.unsqueeze(0) <= ks.unsqueeze(1)).sum(dim=1).double()))


def _stats_end(acc):
    """(results, summed loss) of a pass: the pass's only device -> host copy."""
    tot = acc.tolist()
    results = {'count': int(tot[0]), 'mr': tot[1], 'mrr': tot[2]}
    results.update({f'hits@{k}': int(tot[4 + i]) for i, k in enumerate(_HITS)})
    return results, tot[3]


def predict(val_test_loader, g, model, device):
    """The evaluation pass of the fixed-genotype driver (reference train/mr_lp_train.py:269-314) with its bookkeeping on the device:
    the per-batch rank statistics (number of predictions, sum of ranks, sum of reciprocal ranks, hits at 1 / 3 / 10) and the summed
    BCE loss are accumulated in ONE float64 device vector and read back by ONE copy when the loader is exhausted -- the reference
    synchronises three times per batch (`.item()`).  Returns (results, summed loss), results keyed 'count', 'mr', 'mrr', 'hits@k'
    like the reference's, counts as int."""
    ks, acc = _stats_begin(device)
    with torch.no_grad():
        model.eval()
        for triplets, labels in val_test_loader:
            triplets, labels = triplets.to(device), labels.to(device)
            pred = model(g, triplets[:, 0], triplets[:, 1])
            ranks = filtered_ranks(pred, labels, triplets[:, 2]).double()
            acc += _batch_stats(ranks, F.binary_cross_entropy(pred, labels), ks)
    return _stats_end(acc)


class _LabelSide:
    """A sampler.LabelIndex as the filter side of distmult_ranks (the layout of _KnownSide with num_rels = 2R): every labelled object
    is a member that never leaves (gone_at = 0 against when = -1, the "standard" protocol)."""

    __slots__ = ("keys", "rowptr", "members", "gone_at", "num_rels")

    def __init__(self, label_index):
        li = label_index
        self.keys, self.rowptr, self.members, self.num_rels = li.keys, li.rowptr, li.objs, 2 * li.num_rel
        self.gone_at = torch.zeros_like(li.objs)


def predict_fused(val_test_loader, g, model, label_index, device):
    """predict() for a DistMult network without a [B, N] tensor: same (results, summed loss), same single device -> host copy.
    Per batch of (s, r, o) triples one model.embed(g); the ranks come from distmult_ranks (mrg_distmult_rank) with label_index -- a
    sampler.LabelIndex over the known triples, the source of predict's dense labels -- as the filter: every labelled object but the
    target is filtered, mrg_rank_filtered's rule; the batch's mean BCE comes from mrg_distmult_bce_fwd on the unsmoothed labels.
    The loader yields triplets; a second element (dense labels), if present, is ignored.
    Ranks are taken on the logits, as calc_mrr takes them, where predict ranks float32 sigmoid(x): sigmoid is monotone, ties follow
    the same rule (equal score at a lower entity id), and where float32 sigmoid ties two different logits the value returned here
    lies inside predict's tie interval."""
    from .operations_lp import sf_DisMult_op
    if torch.device(device).type != "cuda" or not next(model.parameters()).is_cuda:
        raise MrgnasError("predict_fused runs on a HIP device (no CPU fallback); got " + str(device))
    if not isinstance(model.score_func, sf_DisMult_op):
        raise MrgnasError(f"predict_fused covers the DistMult scorer only; this network scores with {type(model.score_func).__name__}")
    return predict_1n(val_test_loader, g, model, label_index, device)


def predict_1n(val_test_loader, g, model, label_index, device):
    """predict_fused for every scorer that follows the scorer protocol (operations_lp: ``query`` and ``score_kind``): DistMult, ConvE
    ("dot"), TransE ("l1") and a "dot" scorer with a ``score_bias`` (compgcn.CompGCN_ConvE, its own scorer: the bias goes to the ranks
    and to the loss).  Per batch one model.embed(g) and one score_func.query(ent[s], rel_emb[r]); the ranks come from
    query_ranks with label_index as the filter and when = -1, the batch's mean BCE from mrg_distmult_bce_fwd / mrg_transe_bce_fwd on the
    unsmoothed labels.  "dot" ranks are taken on the logits, "l1" ranks on the distances: where predict's float32 sigmoid ties
    different logits -- with gamma = 40 and realistic L1 distances it saturates to exactly 0 and ties whole rows -- the value
    returned here lies inside predict's tie interval."""
    from . import functional as K
    if torch.device(device).type != "cuda" or not next(model.parameters()).is_cuda:
        raise MrgnasError("predict_1n runs on a HIP device (no CPU fallback); got " + str(device))
    sf = model.score_func
    kind = getattr(sf, "score_kind", None)
    if not hasattr(sf, "query") or kind not in ("dot", "l1"):
        raise MrgnasError(f"predict_1n needs a scorer with query() and a score_kind of 'dot' or 'l1'; this network scores with {type(sf).__name__}")
    side = _LabelSide(label_index)
    v_zero, v_one = label_index.label_values(0.0)
    bias = getattr(sf, "score_bias", None)                  # a "dot" scorer's optional per-entity bias (CompGCN_ConvE)
    ks, acc = _stats_begin(device)
    with torch.no_grad():
        model.eval()
        for batch in val_test_loader:
            triplets = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(device)
            s, r, o = (triplets[:, i].int().contiguous() for i in range(3))
            ent, rel_emb = model.embed(g)
            ent = f32c(ent)
            q = f32c(sf.query(K.gather_rows(ent, s), K.gather_rows(f32c(rel_emb), r)))
            when = torch.full((s.numel(),), -1, dtype=torch.int32, device=device)
            qkey = (s.long() * side.num_rels + r.long()).contiguous()
            ranks = query_ranks(q, ent, o, side, when, qkey, kind, bias=bias).double()
            if kind == "l1":
                loss = K.transe_bce_mean(q, ent, sf.gamma, label_index, qkey, v_zero, v_one)
            else:
                loss = K.distmult_bce_mean(q, ent, label_index, qkey, v_zero, v_one, bias=bias)
            acc += _batch_stats(ranks, loss, ks)
    return _stats_end(acc)


def combine_results(left, right):
    """get_combined_results of the reference's infer() (train/mr_lp_train.py:327-345)."""
    if left['count'] != right['count']:
        raise AssertionError("head and tail evaluations must cover the same number of triples")
    count, results = float(left['count']), {}
    for side, r in (('left', left), ('right', right)):
        results[f'{side}_mr'] = round(r['mr'] / count, 5)
        results[f'{side}_mrr'] = round(r['mrr'] / count, 5)
    results['mr'] = round((left['mr'] + right['mr']) / (2 * count), 5)
    results['mrr'] = round((left['mrr'] + right['mrr']) / (2 * count), 5)
    for k in [1, 3, 10]:
        results[f'left_hits@{k}'] = round(left[f'hits@{k}'] / count, 5)
        results[f'right_hits@{k}'] = round(right[f'hits@{k}'] / count, 5)
        results[f'hits@{k}'] = round((results[f'left_hits@{k}'] + results[f'right_hits@{k}']) / 2, 5)
    return results


# ---- calc_mrr: the search driver's evaluation (reference utils/utils_rgcn.py:212-380, search/mr_lp_search.py:258-278) ----------------
# Raw and filtered MRR / Hits@k of entity and relation embeddings under DistMult, on the device and without a [Q, N] tensor: one
# entry point, ``mrg_distmult_rank``, runs the product (emb[a] * w[r]) emb^T as a row GEMM whose epilogue counts, per query, the
# unfiltered candidates that beat the target.
#
# Semantics (checked against the reference's own functions, tests/golden/make_golden_mrr.py):
#   * the reference ranks sigmoid(x); sigmoid is monotone, so the kernel ranks x.  Ties follow mrg_rank_filtered's rule,
#     rank = 1 + #(greater) + #(equal at a lower entity id); the reference's torch.sort leaves equal scores in unspecified order, and
#     where float32 sigmoid saturates and the reference ties, this value lies inside the reference's tie interval.
#   * raw: nothing is filtered.  Pass S perturbs the subject (fixed entity o, target s), pass O the object (fixed s, target o).
#   * filtered, protocol="reference": the reference's filter set starts as the distinct triples of train, valid and test, and
#     filter_s / filter_o REMOVE the query's own triple from it for good.  Pass S runs first on the same set object, so its query i is
#     filtered by the set minus test triples 0..i, and every query of pass O by the set minus all test triples.  Here every known
#     triple carries gone_at = index of the first test triple equal to it (else INT32_MAX), every query a `when` (i in pass S, T in
#     pass O), and a candidate is filtered iff its triple is known, gone_at > when, and it is not the target.
#   * protocol="standard" filters every known triple but the query's own: the same kernel with when = -1.  It differs from the
#     reference's numbers and is therefore not the default.
#   * the reference's calc_raw_mrr returns only mrr, so its calc_mrr(eval_p="raw") fails at the unpacking; here both protocols return
#     (mrr, hit_k).
_INT32_MAX = 2 ** 31 - 1


class _KnownSide:
    """The filter index of one pass: list u holds the entities that complete key keys[u] = fixed_entity * num_rels + relation to a
    known triple, members[rowptr[u]:rowptr[u + 1]] ascending, with their gone_at."""

    __slots__ = ("keys", "rowptr", "members", "gone_at", "num_rels")

    def __init__(self, key, member, gone_at, num_ent, num_rels):
        order = torch.argsort(key * num_ent + member)              # (key, member) ascending; the triples are distinct
        key, self.num_rels = key[order], num_rels
        self.members, self.gone_at = member[order].int().contiguous(), gone_at[order].int().contiguous()
        self.keys, counts = torch.unique_consecutive(key, return_counts=True)
        self.rowptr = torch.cat((counts.new_zeros(1), counts.cumsum(0))).int().contiguous()


class KnownTriples:
    """The distinct triples of train, valid and test as the two filter indexes of calc_mrr, built with torch sorts on whatever device
    the triples live on (CPU tensors work too).  `subject`: key o * R + r, members s (pass S); `object`: key s * R + r, members o
    (pass O).  gone_at: index of the first test triple equal to the member's triple, else INT32_MAX."""

    def __init__(self, train, valid, test, num_ent, num_rels):
        parts = [torch.as_tensor(t).long().reshape(-1, 3) for t in (train, valid, test)]
        parts = [p.to(parts[2].device) for p in parts]
        tri = torch.cat(parts)
        self.num_ent, self.num_rels, self.num_test = int(num_ent), int(num_rels), int(parts[2].shape[0])
        if tri.numel() and (int(tri.min()) < 0 or int(tri[:, (0, 2)].max()) >= num_ent or int(tri[:, 1].max()) >= num_rels):
            raise ValueError("KnownTriples: an entity or relation id is out of range")
        if num_ent * num_rels * num_ent >= 2 ** 63 or tri.shape[0] >= _INT32_MAX or num_ent >= _INT32_MAX:
            raise ValueError("KnownTriples: the triple codes do not fit")
        code = (tri[:, 0] * num_rels + tri[:, 1]) * num_ent + tri[:, 2]
        pos = torch.full((tri.shape[0],), _INT32_MAX, dtype=torch.int64, device=tri.device)
        pos[tri.shape[0] - self.num_test:] = torch.arange(self.num_test, device=tri.device)
        uniq, inv = torch.unique(code, return_inverse=True)
        gone = torch.full((uniq.numel(),), _INT32_MAX, dtype=torch.int64, device=tri.device).scatter_reduce(0, inv, pos, "amin")
        s, r, o = uniq // (num_rels * num_ent), (uniq // num_ent) % num_rels, uniq % num_ent
        self.subject = _KnownSide(o * num_rels + r, s, gone, num_ent, num_rels)
        self.object = _KnownSide(s * num_rels + r, o, gone, num_ent, num_rels)


def _filter_side(msg, known_side, when, qkey, Q):
    """The filter side of a rank call: (qkey, when, keys, rowptr, members, gone_at, U) on the HIP device, or all None and U = 0 for raw
    ranks (no known_side, or an empty one).  qkey: the queries' keys [Q], or a function of known_side that forms them."""
    k = known_side
    if k is None or k.keys.numel() == 0:
        return None, None, None, None, None, None, 0
    if when is None or when.numel() != Q or qkey is None or not (callable(qkey) or qkey.numel() == Q):
        raise ValueError(msg)
    qkey, when = (qkey(k) if callable(qkey) else qkey).long().contiguous(), when.int().contiguous()
    require_hip(k.keys, k.rowptr, k.members, k.gone_at, qkey, when)
    return qkey, when, k.keys, k.rowptr, k.members, k.gone_at, k.keys.numel()


def _score_bias(what, bias, kind, N):
    """An optional per-entity score bias of a "dot" sweep, checked before any device check (functional.score_bias_arg): float32 [N]."""
    from .functional.scoring import score_bias_arg
    bias = score_bias_arg(what, bias, kind, N)
    if bias is not None and not bias.is_cuda:
        raise MrgnasError(f"{what} runs on a HIP device (no CPU fallback)")
    return None if bias is None else bias.detach()


def _rank_call(name, ws_name, ws_err, head, side, Q, N, D, like):
    """ranks [Q] of entry point `name`(*head, *side, Q, N, D, ranks, workspace, stream): the workspace queried (ws_name; an error code is
    raised under ws_err) and allocated beside `like`."""
    ranks = torch.empty(Q, dtype=torch.int64, device=like.device)
    nbytes = getattr(load(), ws_name)(Q, N, D)
    if nbytes < 0:
        check(int(nbytes), ws_err)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=like.device)
    call(name, (*(ptr(t) for t in head), *(ptr(t) for t in side[:6]), side[6], Q, N, D, ptr(ranks), ptr(ws), int(nbytes), stream_of(like)),
         nbytes=4 * (Q + N) * D, flops=2 * Q * N * D)
    return ranks


def distmult_ranks(embedding, w, a, r, target, known_side=None, when=None):
    """ranks [Q] int64 (1-based) of `target` among all entities for the DistMult queries (fixed entity a, relation r), through
    mrg_distmult_rank.  known_side: a KnownTriples side (`.subject` when the subject is perturbed, `.object` when the object is) with
    `when` [Q] int32, or None for raw ranks.  Ids are trusted to be in range (KnownTriples and calc_mrr check theirs)."""
    embedding, w = f32c(embedding), f32c(w)
    a, r, target = (t.int().contiguous() for t in (a, r, target))
    require_hip(embedding, w, a, r, target)
    Q, (N, D) = a.numel(), embedding.shape
    if r.numel() != Q or target.numel() != Q or w.shape[1] != D:
        raise ValueError("distmult_ranks: a / r / target [Q] and w [R, D] expected")
    side = _filter_side("distmult_ranks: a filtered call needs when [Q]", known_side, when, lambda k: a.long() * k.num_rels + r.long(), Q)
    return _rank_call("mrg_distmult_rank", "mrg_distmult_rank_workspace_bytes", "mrg_distmult_rank_workspace_bytes",
                      (embedding, w, a, r, target), side, Q, N, D, embedding)


def query_ranks(q, ent, target, known_side=None, when=None, qkey=None, kind="dot", bias=None):
    """ranks [Q] int64 (1-based) of `target` among all entities for query rows q [Q, D] the caller holds (a scorer's ``query``).
    kind "dot": the score is q . ent[e] (mrg_rows_rank: distmult_ranks from the point where the rows exist); kind "l1": the score is
    -||q - ent[e]||_1, compared on the distance itself (mrg_transe_rank).  known_side / when as in distmult_ranks, with qkey [Q] int64
    the queries' keys into known_side (fixed entity * num_rels + relation); None for raw ranks.  bias [N] (kind "dot" only, else
    ValueError): the score is q . ent[e] + bias[e] (mrg_rows_bias_rank)."""
    if kind not in ("dot", "l1"):
        raise ValueError("query_ranks: kind is 'dot' or 'l1'")
    bias = _score_bias("query_ranks", bias, kind, ent.shape[0])
    if not (q.is_cuda and ent.is_cuda and target.is_cuda):
        raise MrgnasError("query_ranks runs on a HIP device (no CPU fallback)")
    q, ent, target = f32c(q), f32c(ent), target.int().contiguous()
    require_hip(q, ent, target)
    (Q, D), N = q.shape, ent.shape[0]
    if ent.shape[1] != D or target.numel() != Q:
        raise ValueError("query_ranks: q [Q, D], ent [N, D] and target [Q] expected")
    side = _filter_side("query_ranks: a filtered call needs when [Q] and qkey [Q]", known_side, when, qkey, Q)
    name, ws_name = ("mrg_rows_rank", "mrg_distmult_rank_workspace_bytes") if kind == "dot" else ("mrg_transe_rank", "mrg_transe_rank_workspace_bytes")
    if bias is not None:
        require_hip(bias)
        return _rank_call("mrg_rows_bias_rank", ws_name, "mrg_rows_bias_rank", (q, ent, bias, target), side, Q, N, D, q)
    return _rank_call(name, ws_name, name, (q, ent, target), side, Q, N, D, q)


def mix_ranks(sub_emb, rel_emb, ent, weights, gamma, target, known_side=None, when=None, qkey=None, hidden=None):
    """ranks [Q] int64 (1-based) of `target` among all entities under the mixed score of the score-function search cell,
    p_e = w0 sigmoid(gamma - ||sub + rel - ent[e]||_1) + w1 sigmoid((sub * rel) . ent[e]), compared on the float32 p itself
    (mrg_sfmix_rank; equal p: the lower entity id first).  sub_emb / rel_emb [Q, D]; weights [2] float32 on the device, TransE's first.
    With weights [3] and hidden [Q, D] (sf_ConvE_op.query's rows) the score has the third term + w2 sigmoid(hidden . ent[e])
    (mrg_sfmix3_rank).  known_side / when / qkey as in query_ranks; None for raw ranks."""
    from . import functional as K
    if not (sub_emb.is_cuda and rel_emb.is_cuda and ent.is_cuda and weights.is_cuda and target.is_cuda):
        raise MrgnasError("mix_ranks runs on a HIP device (no CPU fallback)")
    nw = 2 if hidden is None else 3
    if (sub_emb.dim() != 2 or sub_emb.shape != rel_emb.shape or ent.dim() != 2 or ent.shape[1] != sub_emb.shape[1] or weights.numel() != nw
            or (hidden is not None and hidden.shape != sub_emb.shape)):
        raise ValueError("mix_ranks: sub_emb / rel_emb [Q, D], ent [N, D] and weights [2], or hidden [Q, D] and weights [3], expected")
    if hidden is not None and not hidden.is_cuda:
        raise MrgnasError("mix_ranks runs on a HIP device (no CPU fallback)")
    sub_emb, rel_emb, ent, weights, target = f32c(sub_emb), f32c(rel_emb), f32c(ent), f32c(weights.reshape(nw)), target.int().contiguous()
    require_hip(sub_emb, rel_emb, ent, weights, target)
    (Q, D), N = sub_emb.shape, ent.shape[0]
    if target.numel() != Q:
        raise ValueError("mix_ranks: target [Q] expected")
    side = _filter_side("mix_ranks: a filtered call needs when [Q] and qkey [Q]", known_side, when, qkey, Q)
    with torch.no_grad():
        obj, qd = K.compose("add", sub_emb, rel_emb), K.compose("mult", sub_emb, rel_emb)
    ranks = torch.empty(Q, dtype=torch.int64, device=ent.device)
    name = "mrg_sfmix_rank" if hidden is None else "mrg_sfmix3_rank"
    nbytes = getattr(load(), name + "_workspace_bytes")(Q, N, D)
    if nbytes < 0:
        check(int(nbytes), name)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=ent.device)
    tail = (ptr(ent), ptr(weights), float(gamma), ptr(target), *(ptr(t) for t in side[:6]), side[6], Q, N, D, ptr(ranks), ptr(ws), int(nbytes),
            stream_of(ent))
    if hidden is None:
        call(name, (ptr(obj), ptr(qd), *tail), nbytes=4 * (2 * Q + N) * D, flops=5 * Q * N * D)
    else:
        qh = f32c(hidden.detach())
        require_hip(qh)
        call(name, (ptr(obj), ptr(qd), ptr(qh), *tail), nbytes=4 * (3 * Q + N) * D, flops=7 * Q * N * D)
    return ranks


def predict_mix(loader, ent, rel_emb, weights, gamma, label_index, device, conve=None):
    """predict_1n's loop and result dictionary under the mixed score, on embeddings the caller already holds (a supernet's forward):
    per batch of (s, r, o) triples the ranks come from mix_ranks with label_index as the filter and when = -1, the batch's mean BCE
    from mrg_sfmix_bce_fwd on the unsmoothed labels.  conve: the sf_ConvE_op of a three-way MixedOp_SF (weights [3]); it is put in
    eval mode for the pass (and back afterwards) and forms the batch's hidden rows.  Returns (results, summed loss) after ONE
    device -> host copy."""
    from . import functional as K
    if torch.device(device).type != "cuda" or not (ent.is_cuda and rel_emb.is_cuda and weights.is_cuda):
        raise MrgnasError("predict_mix runs on a HIP device (no CPU fallback); got " + str(device))
    side = _LabelSide(label_index)
    v_zero, v_one = label_index.label_values(0.0)
    ks, acc = _stats_begin(device)
    was_training = conve is not None and conve.training
    if conve is not None:
        conve.eval()
    try:
        with torch.no_grad():
            ent, rel_emb, weights = f32c(ent), f32c(rel_emb), f32c(weights.reshape(2 if conve is None else 3))
            for batch in loader:
                triplets = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(device)
                s, r, o = (triplets[:, i].int().contiguous() for i in range(3))
                sub_e, rel_e = K.gather_rows(ent, s), K.gather_rows(rel_emb, r)
                when = torch.full((s.numel(),), -1, dtype=torch.int32, device=device)
                qkey = (s.long() * side.num_rels + r.long()).contiguous()
                obj, qd = K.compose("add", sub_e, rel_e), K.compose("mult", sub_e, rel_e)
                if conve is None:
                    ranks = mix_ranks(sub_e, rel_e, ent, weights, gamma, o, side, when, qkey).double()
                    loss = K.sf_mix_bce_mean(obj, qd, ent, weights, gamma, label_index, qkey, v_zero, v_one)
                else:
                    hidden = conve.query(sub_e, rel_e)
                    ranks = mix_ranks(sub_e, rel_e, ent, weights, gamma, o, side, when, qkey, hidden=hidden).double()
                    loss = K.sf_mix3_bce_mean(obj, qd, hidden, ent, weights, gamma, label_index, qkey, v_zero, v_one)
                acc += _batch_stats(ranks, loss, ks)
    finally:
        if was_training:
            conve.train()
    return _stats_end(acc)


_TOPK_MAX = 64


def query_topk(q, ent, k, known_side=None, when=None, qkey=None, kind="dot", bias=None):
    """(ids [Q, k] int64, values [Q, k] float32): per query row of q [Q, D] the k best unfiltered entities, best first, without a
    [Q, N] tensor -- the twin of query_ranks.  kind "dot": the largest logits q . ent[e] (mrg_rows_topk); kind "l1": the smallest
    distances ||q - ent[e]||_1 (mrg_transe_topk).  Equal values: the lower entity id first.  known_side / when / qkey as in
    query_ranks; there is no target, so every member with gone_at > when is excluded.  values are the float32 accumulators the rank
    sweeps compare, so query_ranks(q, ent, ids[:, j], ...) == j + 1.  Where fewer than k candidates remain the tail is id -1 with
    value -inf ("dot") / +inf ("l1").  bias [N] (kind "dot" only, else ValueError): the logits, and the values returned, are
    q . ent[e] + bias[e] (mrg_rows_bias_topk), the numbers query_ranks(..., bias=bias) compares."""
    if kind not in ("dot", "l1"):
        raise ValueError("query_topk: kind is 'dot' or 'l1'")
    bias = _score_bias("query_topk", bias, kind, ent.shape[0])
    k = int(k)
    if not 1 <= k <= _TOPK_MAX:
        raise ValueError(f"query_topk: 1 <= k <= {_TOPK_MAX} (got {k}); for a longer list run the dense forward, model(g, subj, rel), "
                         "and torch.topk")
    if not (q.is_cuda and ent.is_cuda):
        raise MrgnasError("query_topk runs on a HIP device (no CPU fallback)")
    q, ent = f32c(q), f32c(ent)
    require_hip(q, ent)
    if q.dim() != 2 or ent.dim() != 2 or ent.shape[1] != q.shape[1]:
        raise ValueError("query_topk: q [Q, D] and ent [N, D] expected")
    (Q, D), N = q.shape, ent.shape[0]
    side = _filter_side("query_topk: a filtered call needs when [Q] and qkey [Q]", known_side, when, qkey, Q)
    name = "mrg_rows_topk" if kind == "dot" else "mrg_transe_topk"
    ws_name = name + "_workspace_bytes"
    head = (ptr(q), ptr(ent))
    if bias is not None:
        require_hip(bias)
        name, head = "mrg_rows_bias_topk", (ptr(q), ptr(ent), ptr(bias))               # (same workspace)
    ids = torch.empty(Q, k, dtype=torch.int32, device=q.device)
    vals = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    nbytes = getattr(load(), ws_name)(Q, N, D, k)
    if nbytes < 0:
        check(int(nbytes), name)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=q.device)
    call(name, (*head, *(ptr(t) for t in side[:6]), side[6], Q, N, D, k, ptr(ids), ptr(vals), ptr(ws), int(nbytes), stream_of(q)),
         nbytes=4 * (Q + N) * D, flops=2 * Q * N * D)
    return ids.long(), vals


def predict_topk(model, g, subj, rel, k, label_index=None):
    """(objects [B, k] int64, probabilities [B, k] float32): the k most probable objects of every query (subj[b], rel[b], ?) of a
    network whose scorer follows the scorer protocol (operations_lp: ``query`` and ``score_kind``), most probable first, without the
    [B, N] matrix of model(g, subj, rel).  rel follows the loaders' convention (r + num_rel asks for heads).  Eval mode, no autograd,
    one model.embed(g) and one score_func.query.  label_index: a sampler.LabelIndex whose known objects of (subj[b], rel[b]) are
    excluded (the filter of predict_1n with no target); None for raw results.  Probabilities are sigmoid(logit), or
    sigmoid(gamma - distance) for TransE; where fewer than k objects remain the tail is object -1 with probability 0."""
    from . import functional as K
    sf = model.score_func
    kind = getattr(sf, "score_kind", None)
    if not hasattr(sf, "query") or kind not in ("dot", "l1"):
        raise MrgnasError(f"predict_topk needs a scorer with query() and a score_kind of 'dot' or 'l1'; this network scores with {type(sf).__name__}")
    if not (next(model.parameters()).is_cuda and subj.is_cuda and rel.is_cuda):
        raise MrgnasError("predict_topk runs on a HIP device (no CPU fallback)")
    if not 1 <= int(k) <= _TOPK_MAX:
        raise ValueError(f"predict_topk: 1 <= k <= {_TOPK_MAX} (got {k}); for a longer list run the dense forward, model(g, subj, rel), "
                         "and torch.topk")
    with torch.no_grad():
        model.eval()
        s, r = subj.int().contiguous(), rel.int().contiguous()
        ent, rel_emb = model.embed(g)
        ent = f32c(ent)
        q = f32c(sf.query(K.gather_rows(ent, s), K.gather_rows(f32c(rel_emb), r)))
        bias = getattr(sf, "score_bias", None)
        if label_index is None:
            ids, vals = query_topk(q, ent, k, kind=kind, bias=bias)
        else:
            side = _LabelSide(label_index)
            when = torch.full((s.numel(),), -1, dtype=torch.int32, device=q.device)
            qkey = (s.long() * side.num_rels + r.long()).contiguous()
            ids, vals = query_topk(q, ent, k, side, when, qkey, kind, bias=bias)
        prob = torch.sigmoid(sf.gamma - vals) if kind == "l1" else torch.sigmoid(vals)
        return ids, torch.where(ids >= 0, prob, torch.zeros_like(prob))


def _both_passes(embedding, w, test, eval_bz, known, protocol):
    """cat(ranks_s, ranks_o) over the test triples, at most eval_bz queries per launch."""
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    T, step = test.shape[0], max(int(eval_bz), 1)
    out = []
    for fixed, tgt, side, when_all in ((o, s, known.subject if known else None, None), (s, o, known.object if known else None, T)):
        if known is None:
            when = None
        elif protocol == "standard":
            when = torch.full((T,), -1, dtype=torch.int32, device=test.device)
        else:
            when = (torch.arange(T, dtype=torch.int32, device=test.device) if when_all is None
                    else torch.full((T,), when_all, dtype=torch.int32, device=test.device))
        for b in range(0, T, step):
            e = min(T, b + step)
            out.append(distmult_ranks(embedding, w, fixed[b:e], r[b:e], tgt[b:e], side, None if when is None else when[b:e]))
    return torch.cat(out) if out else torch.empty(0, dtype=torch.int64, device=test.device)


def _summarise(ranks, hits):
    """(mrr, [hits@k]) as Python floats: float64 on the device, ONE device -> host copy."""
    rd = ranks.double()
    ks = torch.tensor([float(k) for k in hits], dtype=torch.float64, device=ranks.device)
    vals = torch.cat((rd.reciprocal().mean().view(1), (rd.unsqueeze(0) <= ks.unsqueeze(1)).double().mean(dim=1))).tolist()
    return vals[0], vals[1:]


def _test_on(embedding, test_triplets):
    if not embedding.is_cuda:
        raise MrgnasError("calc_mrr runs on a HIP device (no CPU fallback); got embeddings on " + str(embedding.device))
    return torch.as_tensor(test_triplets).long().reshape(-1, 3).to(embedding.device)


def calc_raw_mrr(embedding, w, test_triplets, hits=[], eval_bz=100):
    """Raw MRR and Hits@k (reference utils/utils_rgcn.py:241-264; returns (mrr, hit_k) where the reference returns mrr alone)."""
    with torch.no_grad():
        test = _test_on(embedding, test_triplets)
        if test.numel() and (int(test.min()) < 0 or int(test[:, (0, 2)].max()) >= embedding.shape[0] or int(test[:, 1].max()) >= w.shape[0]):
            raise ValueError("calc_raw_mrr: an entity or relation id is out of range")
        return _summarise(_both_passes(embedding, w, test, eval_bz, None, "reference"), hits)


def calc_filtered_mrr(embedding, w, train_triplets, valid_triplets, test_triplets, hits=[], eval_bz=100, protocol="reference"):
    """Filtered MRR and Hits@k (reference utils/utils_rgcn.py:342-367).  protocol: "reference" (the reference's removal order, see
    above) or "standard" (every known triple but the query's own)."""
    if protocol not in ("reference", "standard"):
        raise ValueError("calc_filtered_mrr: protocol is 'reference' or 'standard'")
    with torch.no_grad():
        test = _test_on(embedding, test_triplets)
        known = KnownTriples(torch.as_tensor(train_triplets).to(test.device), torch.as_tensor(valid_triplets).to(test.device), test,
                             embedding.shape[0], w.shape[0])
        return _summarise(_both_passes(embedding, w, test, eval_bz, known, protocol), hits)


def calc_mrr(embedding, w, train_triplets, valid_triplets, test_triplets, hits=[], eval_bz=100, eval_p="filtered", protocol="reference"):
    """The reference's calc_mrr (utils/utils_rgcn.py:375-380) on the device: (mrr, hit_k) as Python floats.  eval_bz only bounds the
    number of queries per launch; the result does not depend on it."""
    if eval_p == "filtered":
        return calc_filtered_mrr(embedding, w, train_triplets, valid_triplets, test_triplets, hits, eval_bz, protocol)
    return calc_raw_mrr(embedding, w, test_triplets, hits, eval_bz)


def infer_graph(test_graph, test_src_in, test_rel, test_node_id, model, train_data, valid_data, test_data, device, eval_bz=1000,
                eval_p="filtered"):
    """infer_graph of the search driver (reference search/mr_lp_search.py:258-278): the network in eval mode, one forward without
    autograd, calc_mrr with hits at 1 / 3 / 10.  model: supernet.SearchNetwork (anything whose forward(graph, node_id, src_in,
    edge_type) returns (entity embeddings, relation embeddings))."""
    model.eval()
    with torch.no_grad():
        test_src_in = torch.as_tensor(test_src_in).to(device)
        ent_embed, rel_embed = model(test_graph.to(device), test_node_id, test_src_in, test_rel.to(device))
        return calc_mrr(ent_embed, rel_embed, torch.as_tensor(train_data).long(), torch.as_tensor(valid_data).long(), test_data,
                        hits=[1, 3, 10], eval_bz=eval_bz, eval_p=eval_p)
