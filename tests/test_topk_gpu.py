"""Top-k link prediction without a [Q, N] tensor on the device: mrg_rows_topk (EPI_TOPK on the row GEMM, csrc/topk.hip), mrg_transe_topk
(L1_TOPK of l1_sweep_k, csrc/transe_1n.hip), the shared selection and merge (csrc/topk_parts.hpp), evaluation.query_topk / predict_topk
and FixedNetwork.predict_topk -- against float64 (exactly on dyadic data, within the rank bands on floats), against the rank sweeps
(position j + 1 is the rank of entry j) and for memory.  Tile edges: 128 x 224 ("dot"), 64 x 64 ("l1"); column block 28 672; split
core from D = 52, exact core below and for D % 4 != 0."""
import functools

import numpy as np
import pytest
import torch

from mr_gnas_amd import evaluation as EV, supernet as S
from mr_gnas_amd.sampler import LabelIndex
import l1_ref as L1
import mrr_ref as MR
import topk_ref as TK
from test_fused_scorers_gpu import CONVE_ARGS, Side, genotype, tiny_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
BCE_COLS = 7 * 32 * 128
KINDS = ("dot", "l1")
PAD = {"dot": float("-inf"), "l1": float("inf")}


def make_filter(Q, N, g):
    """The index of test_fused_scorers_gpu._dyadic_case without targets: query i has its own key 3 i; by i % 4 a list of tile-edge
    and random members with gone_at below, at and above `when`, a list of half the entities, an empty list, an unknown key.  Query 1
    has everything filtered, query 2 is unfiltered (key -1), query Q // 2 repeats query 0."""
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g)
    qkey = 3 * torch.arange(Q)
    when = ri(-1, 10, (Q,))
    edges = [c for c in (0, 31, 32, 63, 64, 127, 128, 223, 224, 447, 448, N - 1) if c < N]
    lists = {}
    for i in range(Q):
        kind = i % 4
        if i == 1:
            lists[3 * i] = (torch.arange(N), torch.full((N,), MR.INT32_MAX))
        elif kind == 0:
            m = torch.unique(torch.cat((torch.tensor(edges), ri(0, N, (N // 10 + 1,)))))
            lists[3 * i] = (m, ri(0, 10, (m.numel(),)))
        elif kind == 1:
            m = torch.unique(ri(0, N, (N // 2 + 1,)))
            lists[3 * i] = (m, ri(0, 10, (m.numel(),)))
        elif kind == 2:
            lists[3 * i] = (torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64))
    if Q > 2:
        qkey[2] = -1
    if Q > 4:
        qkey[Q // 2], when[Q // 2] = qkey[0], when[0]
    keys = torch.tensor(sorted(lists), dtype=torch.int64)
    counts = torch.tensor([lists[int(k)][0].numel() for k in keys], dtype=torch.int64)
    rowptr = torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0)))
    members = torch.cat([lists[int(k)][0] for k in keys])
    gone_at = torch.cat([lists[int(k)][1] for k in keys])
    allowed = TK.allowed_mask(N, qkey, when, keys, rowptr, members, gone_at)
    return dict(qkey=qkey.to(DEV), when=when.int().to(DEV), side=Side(keys, rowptr, members, gone_at), allowed=allowed)


@functools.lru_cache(maxsize=8)
def dyadic_case(Q, N, D, plant=False):
    """Entries j / 4, j in [-8, 8]: every logit and every distance is exact in any order of summation, in float32 and on the split
    core, and ties are massive.  The float64 lists are computed once, for k = 64; a shorter list is their prefix.  plant: entity N - 2
    is query 0's row (distance 0) and entity N - 3 the row of the largest possible logit of query 3."""
    g = torch.Generator().manual_seed(1000003 * Q + 1009 * N + D)
    ent = torch.randint(-8, 9, (N, D), generator=g).float() / 4
    q = torch.randint(-8, 9, (Q, D), generator=g).float() / 4
    if Q > 4:
        q[Q // 2] = q[0]
    if plant:
        ent[N - 2] = q[0]
        ent[N - 3] = torch.where(q[3] < 0, -2.0, 2.0)
    c = make_filter(Q, N, g)
    c.update(q=q.to(DEV), ent=ent.to(DEV), N=N)
    for kind in KINDS:
        x = TK.scores64(kind, q, ent)
        c[kind] = TK.topk64(kind, x, c["allowed"], 64)
        c[kind + "_raw"] = TK.topk64(kind, x, torch.ones_like(c["allowed"]), 64)
    return c


def run_topk(c, k, kind, filtered=True, q=None):
    q = c["q"] if q is None else q
    if filtered:
        ids, vals = EV.query_topk(q, c["ent"], k, c["side"], c["when"], c["qkey"], kind=kind)
    else:
        ids, vals = EV.query_topk(q, c["ent"], k, kind=kind)
    assert ids.dtype == torch.int64 and vals.dtype == torch.float32 and ids.shape == vals.shape == (q.shape[0], k)
    return ids.cpu(), vals.cpu()


def check_exact(c, k, kind, what):
    for filtered in (True, False):
        want_ids, want_vals = c[kind if filtered else kind + "_raw"]
        ids, vals = run_topk(c, k, kind, filtered)
        tag = f"{what} {kind} k {k} {'filtered' if filtered else 'raw'}"
        assert torch.equal(ids, want_ids[:, :k]), f"{tag}: {int((ids != want_ids[:, :k]).sum())} ids differ"
        assert torch.equal(vals.double(), want_vals[:, :k]), f"{tag}: values differ"
        pad = ids < 0
        assert bool((vals[pad] == PAD[kind]).all()) and bool(torch.isfinite(vals[~pad]).all())
        if filtered and ids.shape[0] > 1:
            assert bool((ids[1] == -1).all())                                  # everything filtered
        if filtered and ids.shape[0] > 4:
            assert torch.equal(ids[ids.shape[0] // 2], ids[0])                 # the repeated query
        if not filtered:
            assert int(pad.sum()) == ids.shape[0] * max(0, k - c["N"])         # k > N: the tail alone is padding


@pytest.mark.parametrize("N,D", [(N, D) for N in (1, 31, 33, 64, 65, 223, 224, 225, 449) for D in (1, 33, 48, 52, 200)])
def test_dyadic_topk_is_exact(N, D):
    for Q in (1, 63, 65, 129, 300):
        c = dyadic_case(Q, N, D)
        for kind in KINDS:
            for k in (1, 3, 10, 64):
                check_exact(c, k, kind, f"Q {Q} N {N} D {D}")


@pytest.mark.parametrize("D", [1, 33])
def test_a_second_column_block_merges_into_the_running_list(D):
    """D = 1: a handful of distinct values, so the second block's entries tie with the running list's and must stay behind its lower
    ids.  D = 33: the planted rows of the second block must come first."""
    N = BCE_COLS + 65
    c = dyadic_case(9, N, D, plant=True)
    if D == 33:
        assert int(c["l1_raw"][0][0, 0]) == N - 2 and int(c["dot_raw"][0][3, 0]) == N - 3
    for kind in KINDS:
        assert bool((c[kind + "_raw"][0] < BCE_COLS).any())
        for k in (3, 64):
            check_exact(c, k, kind, f"two column blocks D {D}")


def test_more_queries_than_one_row_chunk():
    c = dyadic_case(8192 + 130, 33, 4)
    for kind in KINDS:
        check_exact(c, 10, kind, "two row chunks")


def test_an_all_zero_table_lists_the_lowest_ids():
    N, Q, D = 300, 66, 33
    ent = torch.zeros(N, D, device=DEV)
    q = torch.randn(Q, D, generator=torch.Generator().manual_seed(1)).to(DEV)
    # one list for every query: the even ids, always in force -> the odd ids remain
    side = Side(torch.tensor([0]), torch.tensor([0, N // 2]), torch.arange(0, N, 2), torch.zeros(N // 2))
    when = torch.full((Q,), -1, dtype=torch.int32, device=DEV)
    qkey = torch.zeros(Q, dtype=torch.int64, device=DEV)
    for kind in KINDS:
        for k in (10, 64):
            ids, vals = EV.query_topk(q, ent, k, kind=kind)
            assert torch.equal(ids.cpu(), torch.arange(k).expand(Q, k))
            if kind == "dot":
                assert bool((vals == 0).all())
            else:
                assert bool((vals == vals[:, :1]).all())
            ids, _ = EV.query_topk(q, ent, k, side, when, qkey, kind=kind)
            assert torch.equal(ids.cpu(), (2 * torch.arange(k) + 1).expand(Q, k))


@pytest.mark.parametrize("D", [33, 64])
def test_duplicated_entity_rows_tie_by_id(D):
    """Copies of one random row at ids 10, 150 and 290 (three different tiles of the L1 sweep, two of the row GEMM's): wherever one is
    listed the others follow at once, in id order, with bitwise the same value."""
    N, Q, k = 300, 70, 10
    gen = torch.Generator().manual_seed(D)
    ent, q = torch.randn(N, D, generator=gen), torch.randn(Q, D, generator=gen)
    ent[150] = ent[290] = ent[10]
    q[:20] = ent[10] + 0.1 * q[:20]                            # queries that have the row near the top
    ent, q = ent.to(DEV), q.to(DEV)
    for kind in KINDS:
        ids, vals = (t.cpu() for t in EV.query_topk(q, ent, k, kind=kind))
        seen = 0
        for i in range(Q):
            at = (ids[i] == 10).nonzero()
            if at.numel() and int(at) + 2 < k:
                p = int(at)
                assert ids[i, p:p + 3].tolist() == [10, 150, 290] and float(vals[i, p]) == float(vals[i, p + 1]) == float(vals[i, p + 2])
                seen += 1
        assert seen >= 20, kind


@pytest.mark.parametrize("D", [52, 200])
def test_unaligned_query_rows_take_the_exact_core_with_the_same_result(D):
    c = dyadic_case(129, 449, D)
    buf = torch.empty(129 * D + 1, device=DEV)
    q = buf[1:].view(129, D)
    q.copy_(c["q"])
    assert q.data_ptr() % 16 != 0 and q.is_contiguous() and c["q"].data_ptr() % 16 == 0
    for kind in KINDS:
        for filtered in (True, False):
            a, b = run_topk(c, 10, kind, filtered), run_topk(c, 10, kind, filtered, q=q)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert torch.equal(a[0], c[kind if filtered else kind + "_raw"][0][:, :10])


# ---- standard-normal floats: consistency with the rank sweeps and the float64 band ------------------------------------------------------
FLOAT_SHAPES = [(129, 449, 200, 10), (129, 449, 33, 10), (65, 225, 52, 64)]


@functools.lru_cache(maxsize=4)
def float_case(Q, N, D):
    g = torch.Generator().manual_seed(0)
    ent, q = torch.randn(N, D, generator=g), torch.randn(Q, D, generator=g)
    c = make_filter(Q, N, torch.Generator().manual_seed(Q + N + D))
    c.update(q=q.to(DEV), ent=ent.to(DEV), q_cpu=q, ent_cpu=ent, N=N)
    return c


@pytest.mark.parametrize("Q,N,D,k", FLOAT_SHAPES)
def test_two_calls_are_bitwise_equal(Q, N, D, k):
    c = float_case(Q, N, D)
    for kind in KINDS:
        a, b = run_topk(c, k, kind), run_topk(c, k, kind)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("Q,N,D,k", FLOAT_SHAPES)
def test_position_is_the_rank_the_rank_sweeps_give(Q, N, D, k):
    c = float_case(Q, N, D)
    for kind in KINDS:
        for filtered in (True, False):
            ids, _ = run_topk(c, k, kind, filtered)
            assert int((ids >= 0).sum()) > Q * min(k, N) // 2
            for j in range(k):
                valid = ids[:, j] >= 0
                t = ids[:, j].clamp(min=0).to(DEV)
                if filtered:
                    ranks = EV.query_ranks(c["q"], c["ent"], t, c["side"], c["when"], c["qkey"], kind=kind).cpu()
                else:
                    ranks = EV.query_ranks(c["q"], c["ent"], t, kind=kind).cpu()
                assert bool((ranks[valid] == j + 1).all()), f"{kind} filtered {filtered} position {j}: {int((ranks[valid] != j + 1).sum())} ranks differ"


def check_band(kind, q, ent, ids, vals, allowed, what, wide_limit=0.05):
    """Every listed entity's position lies in its admissible float64 interval and its value within delta of the float64 score; before
    that: the band is not vacuous -- in float64 alone at most 5 % of the (query, position) pairs of the float64 list have an interval
    wider than one value (2.5 % measured on the CPU for manual_seed(0) normal data at FLOAT_SHAPES and (33, 2049, 200, 10)).
    wide_limit None: the share is printed only (a network's embeddings are not standard normal: an untrained TransE network's
    distances lie close together, 12 % of its positions have a wider band)."""
    k = ids.shape[1]
    x = TK.scores64(kind, q, ent)
    ref_ids, _ = TK.topk64(kind, x, allowed, k)
    lo, hi = TK.position_band(kind, q, ent, ref_ids, allowed)
    rv = ref_ids >= 0
    wide = float(((hi > lo) & rv).sum()) / max(int(rv.sum()), 1)
    print(f"{what} {kind}: {100 * wide:.2f} % of the float64 list's positions have a band wider than one value")
    assert wide_limit is None or wide <= wide_limit
    assert torch.equal(ids >= 0, rv)                                           # as many entries as allowed entities, padding behind them
    valid = ids >= 0
    lo, hi = TK.position_band(kind, q, ent, ids, allowed)
    pos = torch.arange(1, k + 1).expand_as(ids)
    bad = valid & ((pos < lo) | (pos > hi))
    assert not bool(bad.any()), f"{what} {kind}: {int(bad.sum())} positions outside the band"
    assert bool(allowed.gather(1, ids.clamp(min=0))[valid].all())              # nothing filtered is listed
    delta = TK.delta64(kind, q, ent)
    err = (vals.double() - x.gather(1, ids.clamp(min=0))).abs()
    assert bool((err <= delta)[valid].all()), f"{what} {kind}: value error {float(err[valid].max()):.3e}"
    assert bool((vals[~valid] == PAD[kind]).all())
    return x, delta


@pytest.mark.parametrize("Q,N,D,k", FLOAT_SHAPES)
def test_float_lists_lie_in_the_float64_band(Q, N, D, k):
    c = float_case(Q, N, D)
    for kind in KINDS:
        for filtered in (True, False):
            ids, vals = run_topk(c, k, kind, filtered)
            allowed = c["allowed"] if filtered else torch.ones_like(c["allowed"])
            check_band(kind, c["q_cpu"], c["ent_cpu"], ids, vals, allowed, f"Q {Q} N {N} D {D} k {k} {'filtered' if filtered else 'raw'}")


# ---- the network ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score_func", ["sf_DisMult", "sf_ConvE", "sf_TransE"])
def test_predict_topk_of_a_small_network(score_func):
    N, Rg, D, tri, g = tiny_graph()
    li = LabelIndex(tri, Rg, N, DEV)
    torch.manual_seed(3)
    net = S.FixedNetwork(DEV, genotype(score_func), N, Rg, D, D, 5, score_args=dict(CONVE_ARGS)).to(DEV)
    S.xavier_init_(net)
    net.train()
    B, k = 96, 10
    subj = torch.from_numpy(np.concatenate([tri[:B // 2, 0], tri[:B // 2, 2]])).to(DEV)
    rel = torch.from_numpy(np.concatenate([tri[:B // 2, 1], tri[:B // 2, 1] + Rg])).to(DEV)      # the second half asks for heads
    sf = net.score_func
    kind = sf.score_kind
    if kind == "l1":                                           # gamma in the middle of the batch's distances: probabilities that differ
        with torch.no_grad():
            net.eval()
            e0, r0 = net.embed(g)
            sf.gamma = float(torch.round(L1.dist64(e0[subj] + r0[rel], e0).median()))
            net.train()
    objs, prob = net.predict_topk(g, subj, rel, k, li)
    assert not net.training and not objs.requires_grad and not prob.requires_grad
    assert objs.dtype == torch.int64 and prob.dtype == torch.float32 and objs.shape == prob.shape == (B, k)
    with torch.no_grad():
        ent, rel_emb = net.embed(g)
        q = sf.query(ent[subj], rel_emb[rel]).contiguous()
    raw = EV.predict_topk(net, g, subj, rel, k)
    want = EV.query_topk(q, ent, k, kind=kind)
    assert torch.equal(raw[0], want[0])
    assert torch.equal(raw[1], torch.sigmoid(sf.gamma - want[1]) if kind == "l1" else torch.sigmoid(want[1]))
    side = EV._LabelSide(li)
    qkey = (subj.long() * side.num_rels + rel.long()).cpu()
    when = torch.full((B,), -1, dtype=torch.int64)
    allowed = TK.allowed_mask(N, qkey, when, side.keys.cpu(), side.rowptr.cpu(), side.members.cpu(), side.gone_at.cpu())
    known = ~allowed
    assert bool(known.any(dim=1).sum() >= B // 2)              # the queries come from the triples: they have known objects
    assert not torch.equal(raw[0], objs)                       # ... some of which the raw list names
    q_cpu, ent_cpu = q.cpu(), ent.cpu()
    for (ids, p), ok, what in (((objs, prob), allowed, "filtered"), (raw, torch.ones_like(allowed), "raw")):
        ids, p = ids.cpu(), p.cpu()
        vals = EV.query_topk(q, ent, k, *((side, when.int().to(DEV), qkey.to(DEV)) if what == "filtered" else ()), kind=kind)[1].cpu()
        x, delta = check_band(kind, q_cpu, ent_cpu, ids, vals, ok, f"{score_func} {what}", wide_limit=None)
        assert bool((ids >= 0).all())
        assert not bool(known.gather(1, ids).any()) or what == "raw"           # no known object of (s, r) is listed
        logit = x.gather(1, ids)
        p64 = torch.sigmoid(sf.gamma - logit if kind == "l1" else logit)
        assert bool(((p.double() - p64).abs() <= delta / 4 + 2.0 ** -23).all()), f"{score_func} {what}: {float((p.double() - p64).abs().max()):.3e}"
        assert float(p.max()) > float(p.min())


def test_padded_objects_have_probability_zero():
    N, Rg, D, tri, g = tiny_graph()
    torch.manual_seed(3)
    net = S.FixedNetwork(DEV, genotype("sf_TransE"), N, Rg, D, D, 5, score_args={"gamma": 12.0}).to(DEV)
    S.xavier_init_(net)
    full = np.stack([np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64), np.arange(N)], 1)      # (0, 0, o) for all o but the last three
    li = LabelIndex(full[:N - 3], Rg, N, DEV)
    subj, rel = torch.zeros(2, dtype=torch.int64, device=DEV), torch.tensor([0, 1], device=DEV)
    objs, prob = net.predict_topk(g, subj, rel, 5, li)
    assert objs[0, 3:].tolist() == [-1, -1] and sorted(objs[0, :3].tolist()) == [N - 3, N - 2, N - 1] and prob[0, 3:].tolist() == [0.0, 0.0]
    assert bool((objs[1] >= 0).all())


def test_peak_memory_stays_far_below_a_query_by_entity_matrix():
    Q, N, D, k = 4096, 14541, 64, 10
    gen = torch.Generator().manual_seed(0)
    ent, q = ((0.3 * torch.randn(n, D, generator=gen)).to(DEV) for n in (N, Q))
    for kind in KINDS:
        EV.query_topk(q[:8], ent, k, kind=kind)                # the library is loaded
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ids, vals = EV.query_topk(q, ent, k, kind=kind)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        print(f"{kind}: peak rise {rise / 2 ** 20:.1f} MiB, [Q, N] float {Q * N * 4 / 2 ** 20:.1f} MiB")
        assert rise < Q * N * 4 // 4
        assert bool((ids >= 0).all()) and bool((ids < N).all())
