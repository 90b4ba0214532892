"""calc_mrr on HIP (mr_gnas_amd.evaluation, csrc/rank.hip: mrg_distmult_rank) on the device: the reference's ranks on the golden
fixtures, exact ranks on integer data across the kernels' shape edges, duplicate rows and an all-zero table, a float64 band on random
floats, and the drivers calc_mrr / infer_graph."""
import functools

import pytest
import torch

from conftest import load_golden
from mr_gnas_amd import _lib, evaluation as EV, graph as G, supernet as S
from mr_gnas_amd._lib import call, ptr, stream_of
import mrr_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rank_call(ent, rel, a, r, t, qkey=None, when=None, keys=None, rowptr=None, members=None, gone_at=None):
    """mrg_distmult_rank itself on CPU inputs (moved to the device here); the index is passed as given, qkey included."""
    d = lambda x, dt: None if x is None else x.to(dt).contiguous().to(DEV)
    ent, rel = d(ent, torch.float32), d(rel, torch.float32)
    a, r, t, when, rowptr, members, gone_at = (d(x, torch.int32) for x in (a, r, t, when, rowptr, members, gone_at))
    qkey, keys = d(qkey, torch.int64), d(keys, torch.int64)
    Q, (N, D), U = a.numel(), ent.shape, 0 if keys is None else keys.numel()
    ranks = torch.zeros(Q, dtype=torch.int64, device=DEV)
    nbytes = _lib.load().mrg_distmult_rank_workspace_bytes(Q, N, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    call("mrg_distmult_rank", (ptr(ent), ptr(rel), ptr(a), ptr(r), ptr(t), ptr(qkey), ptr(when), ptr(keys), ptr(rowptr), ptr(members),
                               ptr(gone_at), U, Q, N, D, ptr(ranks), ptr(ws), nbytes, stream_of(ent)))
    return ranks.cpu()


# ---- goldens ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mrr_small", "mrr_odd"])
def test_golden_ranks_and_metrics(case):
    """Ranks equal the reference's exactly (both protocols, both passes); mrr within 2T * 2^-23 of its float32 mean; hits equal."""
    z = load_golden(case)
    emb, w, test = z["emb"].to(DEV), z["w"].to(DEV), z["test"].to(DEV)
    T = test.shape[0]
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    known = EV.KnownTriples(z["train"].to(DEV), z["valid"].to(DEV), test, emb.shape[0], w.shape[0])
    when_s = torch.arange(T, dtype=torch.int32, device=DEV)
    when_o = torch.full((T,), T, dtype=torch.int32, device=DEV)
    assert torch.equal(EV.distmult_ranks(emb, w, o, r, s).cpu(), z["raw_ranks_s"])
    assert torch.equal(EV.distmult_ranks(emb, w, s, r, o).cpu(), z["raw_ranks_o"])
    assert torch.equal(EV.distmult_ranks(emb, w, o, r, s, known.subject, when_s).cpu(), z["filtered_ranks_s"])
    assert torch.equal(EV.distmult_ranks(emb, w, s, r, o, known.object, when_o).cpu(), z["filtered_ranks_o"])
    for eval_p in ("filtered", "raw"):
        mrr, hits = EV.calc_mrr(emb, w, z["train"], z["valid"], z["test"], hits=[1, 3, 10], eval_bz=100, eval_p=eval_p)
        assert isinstance(mrr, float) and all(isinstance(h, float) for h in hits)
        print(f"{case} {eval_p}: mrr {mrr!r} reference {float(z[eval_p + '_mrr'])!r}")
        assert abs(mrr - float(z[eval_p + "_mrr"])) <= 2 * T * 2.0 ** -23
        assert torch.tensor(hits, dtype=torch.float32).tolist() == z[eval_p + "_hits"].float().tolist()      # the reference's are float32 means


# ---- exact shapes with integer data ------------------------------------------------------------------------------------------------
R_INT = 3


@functools.lru_cache(maxsize=None)
def _int_case(Q, N, D):
    """Embeddings in {-2 .. 2}: every product and sum is exact on both cores and ties are massive.  Returns the inputs and the expected
    ranks from an int64 restatement."""
    g = torch.Generator().manual_seed(1000003 * Q + 1009 * N + D)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g)
    ent, rel = ri(-2, 3, (N, D)), ri(-2, 3, (R_INT, D))
    a, r, t = ri(0, N, (Q,)), ri(0, R_INT, (Q,)), ri(0, N, (Q,))
    t[0], t[Q - 1] = 0, N - 1                                            # targets in column 0 and N - 1 (Q = 1: N - 1)
    if Q > 4:
        a[Q // 2], r[Q // 2], t[Q // 2] = a[0], r[0], t[0]                # a repeated query
    qkey = a * R_INT + r
    when = ri(-1, 10, (Q,))
    if Q > 4:
        when[Q // 2] = when[0]
    edges = [c for c in (0, 31, 32, 223, 224, 447, 448, N - 1) if c < N]   # first / last column of a tile and of a column block
    lists = {}
    if Q > 1:                                                            # query 1: everything but the target filtered, rank 1
        lists[int(qkey[1])] = (torch.arange(N), torch.full((N,), MR.INT32_MAX))
    for i in range(Q):
        k = int(qkey[i])
        if k in lists:
            continue
        kind = i % 4
        if kind == 0:                                                  # the tile and block edges plus a random tenth
            m = torch.unique(torch.cat((torch.tensor(edges), ri(0, N, (N // 10 + 1,)))))
            lists[k] = (m, ri(0, 10, (m.numel(),)))                      # gone_at below, equal to and above `when`
        elif kind == 1:
            m = torch.unique(ri(0, N, (N // 2 + 1,)))
            lists[k] = (m, ri(0, 10, (m.numel(),)))
        elif kind == 2:
            lists[k] = (torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64))      # a key with an empty list
        # kind 3: the key is not in the index
    if Q > 2:
        qkey[2] = -1                                                     # unfiltered by request
    keys = torch.tensor(sorted(lists), dtype=torch.int64)
    counts = torch.tensor([lists[int(k)][0].numel() for k in keys], dtype=torch.int64)
    rowptr = torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0)))
    members = torch.cat([lists[int(k)][0] for k in keys]) if len(lists) else torch.empty(0, dtype=torch.int64)
    gone_at = torch.cat([lists[int(k)][1] for k in keys]) if len(lists) else torch.empty(0, dtype=torch.int64)
    x = (ent[a] * rel[r]) @ ent.T                                        # int64, exact
    allowed = MR.allowed_mask(N, qkey, when, t, keys, rowptr, members, gone_at)
    return dict(ent=ent, rel=rel, a=a, r=r, t=t, qkey=qkey, when=when, keys=keys, rowptr=rowptr, members=members, gone_at=gone_at,
                expect=MR.exact_ranks(x, t, allowed), expect_raw=MR.exact_ranks(x, t, torch.ones_like(allowed)))


@pytest.mark.parametrize("D", [4, 50, 52, 64, 200])
@pytest.mark.parametrize("N", [1, 33, 224, 225, 449])
def test_integer_data_ranks_are_exact(N, D):
    for Q in (1, 127, 129, 300):
        c = _int_case(Q, N, D)
        got = rank_call(c["ent"], c["rel"], c["a"], c["r"], c["t"], c["qkey"], c["when"], c["keys"], c["rowptr"], c["members"], c["gone_at"])
        assert torch.equal(got, c["expect"]), f"filtered Q {Q} N {N} D {D}: {int((got != c['expect']).sum())} of {Q} ranks differ"
        if Q > 1:
            assert int(got[1]) == 1                                      # everything but the target filtered
        if Q > 4:
            assert int(got[Q // 2]) == int(got[0])                       # the repeated query
        raw = rank_call(c["ent"], c["rel"], c["a"], c["r"], c["t"])
        assert torch.equal(raw, c["expect_raw"]), f"raw Q {Q} N {N} D {D}"
        assert int(got.min()) >= 1 and int(raw.max()) <= N


@pytest.mark.parametrize("D", [4, 52])
def test_more_queries_than_one_sweep_launch(D):
    """The entry point walks the queries in chunks of 8192 per sweep launch: a second, partial chunk on both cores."""
    Q, N = 8192 + 130, 33
    c = _int_case(Q, N, D)
    got = rank_call(c["ent"], c["rel"], c["a"], c["r"], c["t"], c["qkey"], c["when"], c["keys"], c["rowptr"], c["members"], c["gone_at"])
    assert torch.equal(got, c["expect"]), f"{int((got != c['expect']).sum())} of {Q} ranks differ, first at {int((got != c['expect']).nonzero()[0])}"


# ---- edge inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [52, 50])
def test_duplicate_entity_rows_tie_exactly(D):
    """Copies of one row at several ids score bit-identically on both cores, whichever of them is the target: the rank counts exactly
    the copies at lower ids.  Every other row scores lower: the fixed entity's row is v, the copies are 2 v, the rest 0 and the relation
    is all ones, so the scores are |v|^2, 2 |v|^2 and 0."""
    N, Q = 300, 140
    v = torch.randn(D, generator=torch.Generator().manual_seed(7))
    ent, rel = torch.zeros(N, D), torch.ones(1, D)
    ent[150] = v
    copies = torch.tensor([3, 31, 32, 40, 41, 223, 224, 299])
    ent[copies] = 2 * v
    which = torch.arange(Q) % copies.numel()
    a, r = torch.full((Q,), 150), torch.zeros(Q, dtype=torch.int64)
    got = rank_call(ent, rel, a, r, copies[which])
    assert torch.equal(got, 1 + which), f"D {D}: {got.tolist()}"
    # and filtered: the copies at 31 and 224 are filtered for every query but their own
    keys, rowptr = torch.tensor([150]), torch.tensor([0, 2])
    members, gone_at, when = torch.tensor([31, 224]), torch.tensor([5, 5]), torch.zeros(Q, dtype=torch.int64)
    got = rank_call(ent, rel, a, r, copies[which], a.clone(), when, keys, rowptr, members, gone_at)
    allowed = MR.allowed_mask(N, a, when, copies[which], keys, rowptr, members, gone_at)
    expect = 1 + torch.stack([allowed[i, copies[copies < copies[which[i]]]].sum() for i in range(Q)])
    assert torch.equal(got, expect), f"D {D} filtered: {got.tolist()}"


def test_all_zero_table():
    """Every score is +0: rank = 1 + the number of unfiltered lower ids."""
    N, D, Q = 260, 52, 130
    g = torch.Generator().manual_seed(11)
    ent, rel = torch.zeros(N, D), torch.zeros(2, D)
    a, r, t = torch.randint(0, N, (Q,), generator=g), torch.randint(0, 2, (Q,), generator=g), torch.randint(0, N, (Q,), generator=g)
    qkey = a * 2 + r
    keys = torch.unique(qkey[::2])
    counts = torch.randint(1, 40, (keys.numel(),), generator=g)
    rowptr = torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0)))
    members = torch.cat([torch.sort(torch.randperm(N, generator=g)[:int(c)]).values for c in counts])
    gone_at = torch.randint(0, 6, (members.numel(),), generator=g)
    when = torch.randint(-1, 6, (Q,), generator=g)
    allowed = MR.allowed_mask(N, qkey, when, t, keys, rowptr, members, gone_at)
    expect = 1 + torch.stack([allowed[i, :int(t[i])].sum() for i in range(Q)])
    assert torch.equal(rank_call(ent, rel, a, r, t, qkey, when, keys, rowptr, members, gone_at), expect)
    assert torch.equal(rank_call(ent, rel, a, r, t), 1 + t)


# ---- random floats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,Q,cap", [(161, 52, 200, 0.05), (333, 50, 200, 0.05), (1000, 200, 300, 0.25)])
def test_random_floats_stay_in_the_float64_band(N, D, Q, cap):
    """Every rank lies in [1 + #(x > t + delta_q), #(x >= t - delta_q)] over the unfiltered candidates, x in float64."""
    R = 7
    g = torch.Generator().manual_seed(1234)
    emb, w = torch.randn(N, D, generator=g), torch.randn(R, D, generator=g)
    tri = lambda n: torch.stack((torch.randint(0, N, (n,), generator=g), torch.randint(0, R, (n,), generator=g),
                                 torch.randint(0, N, (n,), generator=g)), 1)
    train, test = tri(20 * N), tri(Q)
    known = EV.KnownTriples(train, train[:0], test, N, R)
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    when = torch.full((Q,), Q, dtype=torch.int32)
    side = known.object
    allowed = MR.allowed_mask(N, s * R + r, when, o, side.keys, side.rowptr, side.members, side.gone_at)
    lo, hi = MR.rank_band(emb, w, s, r, o, allowed)
    wide = float((hi > lo).double().mean())
    print(f"N {N} D {D} Q {Q}: share of queries with a band wider than one value {wide:.4f} (cap {cap}), widest {int((hi - lo).max()) + 1}")
    assert wide <= cap                                                   # the reference stays sharp enough to mean something
    assert int((~allowed).sum()) > 0
    got = rank_call(emb, w, s, r, o, s * R + r, when, side.keys, side.rowptr, side.members, side.gone_at)
    bad = (got < lo) | (got > hi)
    assert not bool(bad.any()), f"{int(bad.sum())} of {Q} ranks outside the band, e.g. {got[bad][:4].tolist()} vs {lo[bad][:4].tolist()}..{hi[bad][:4].tolist()}"


# ---- drivers ---------------------------------------------------------------------------------------------------------------------------
def test_calc_mrr_does_not_depend_on_eval_bz():
    z = load_golden("mrr_small")
    emb, w = z["emb"].to(DEV), z["w"].to(DEV)
    for eval_p, protocol in (("filtered", "reference"), ("filtered", "standard"), ("raw", "reference")):
        one = EV.calc_mrr(emb, w, z["train"], z["valid"], z["test"], hits=[1, 3, 10], eval_bz=7, eval_p=eval_p, protocol=protocol)
        two = EV.calc_mrr(emb, w, z["train"], z["valid"], z["test"], hits=[1, 3, 10], eval_bz=1000, eval_p=eval_p, protocol=protocol)
        assert one == two
    ref = EV.calc_mrr(emb, w, z["train"], z["valid"], z["test"], hits=[1, 3, 10], eval_bz=1000)
    std = EV.calc_mrr(emb, w, z["train"], z["valid"], z["test"], hits=[1, 3, 10], eval_bz=1000, protocol="standard")
    assert std[0] > ref[0]                                               # the standard protocol filters more: not the reference's number


def test_infer_graph_is_calc_mrr_of_the_eval_forward():
    z = load_golden("supernet_tiny")
    n = z["node_id"].numel()
    g = G.RelGraph(n, z["src"], z["dst"], z["edge_type"], z["norm"], device=DEV)
    torch.manual_seed(0)
    net = S.SearchNetwork(DEV, z["Nall"], z["R"], z["layers"], 1, 2, 2, z["D"], z["D0"], z["nbase"], 9.0, 0.0, 0.0).to(DEV)
    net.load_alpha([z[f"alpha/{i}"].to(DEV) for i in range(5)])
    data = z["data"].long()
    data = data[(data[:, 0] < n) & (data[:, 2] < n)]
    train, valid, test = data[: data.shape[0] // 2], data[data.shape[0] // 2: data.shape[0] * 3 // 4], data[data.shape[0] * 3 // 4:]
    assert test.shape[0] > 0
    got = EV.infer_graph(g, z["src_in"].numpy(), z["edge_type"], z["node_id"].to(DEV), net, train.numpy(), valid.numpy(), test, DEV, eval_bz=1000)
    assert not net.training
    with torch.no_grad():
        ent, rel = net(g, z["node_id"].to(DEV), z["src_in"].to(DEV), z["edge_type"].to(DEV))
    assert got == EV.calc_mrr(ent, rel, train, valid, test, hits=[1, 3, 10], eval_bz=1000)
    assert 0.0 < got[0] <= 1.0 and len(got[1]) == 3
