"""The 1-N loss and evaluation without [B, N] tensors for TransE and ConvE on the device: csrc/transe_1n.hip (the register-tiled L1 sweep
with its loss, logit-gradient and counting epilogues), mrg_rows_rank, functional.transe_bce_all / dot_bce_all, FixedNetwork.loss_1n and
evaluation.query_ranks / predict_1n, against float64, against the dense device path and against the reference's own numbers.
Tile edges of the L1 sweep: 64 queries, 64 entities, 32 columns per slice."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_param_grad, load_golden, sub
from mr_gnas_amd import _lib, evaluation as EV, functional as K, graph as G, supernet as S
from mr_gnas_amd.sampler import LabelIndex
import l1_ref as L1
import mrr_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 3


def genotype(score_func):
    return [S.Genotype(alpha_cell=[('pre_sub', 1, 0), ('f_sparse_comp', 2, 1), ('f_sparse_comp', 3, 2), ('a_max', 4, 2), ('a_max', 5, 3),
                                   ('f_sparse_last', 6, 5), ('f_sparse_last', 7, 5)], concat_node=[4, 5, 6, 7], score_func=score_func)]


def rel_err(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def make_index(N, B, seed):
    """make_index of test_fused_bce_gpu.py with the straddling key on this sweep's tile edge: key (0, 0) lists every entity, key (1, 0)
    lists entities 63 and 64 where they exist, every key (s, R - 1) is unknown; rows 0 and 3 of the batch are identical."""
    rng = np.random.default_rng(seed)
    T = 3 * N
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, max(R - 1, 1), T), rng.integers(0, N, T)], 1)
    extra = [(0, 0, o) for o in range(N)] + [(min(1, N - 1), 0, o) for o in (63, 64) if o < N]
    tri = np.concatenate([tri, np.asarray(extra, dtype=tri.dtype)])
    subj, rel = rng.integers(0, N, B), rng.integers(0, 2 * R, B)
    fixed = [(0, 0), (min(1, N - 1), 0), (int(rng.integers(0, N)), R - 1), (0, 0)]
    for i, (s, r) in enumerate(fixed[:B]):
        subj[i], rel[i] = s, r
    sr2o = {}
    for s, r, o in tri.tolist():
        sr2o.setdefault((s, r), set()).add(o)
        sr2o.setdefault((o, r + R), set()).add(s)
    y = np.zeros((B, N), dtype=np.float64)
    for i in range(B):
        y[i, sorted(sr2o.get((int(subj[i]), int(rel[i])), ()))] = 1.0
    li = LabelIndex(tri, R, N, DEV)
    return li, torch.from_numpy(subj).to(DEV), torch.from_numpy(rel).to(DEV), torch.from_numpy(y).to(DEV)


def smoothed(y01, li, label_smooth):
    v0, v1 = li.label_values(label_smooth)
    return y01 * (v1 - v0) + v0


def float_case(B, N, D, seed):
    """Random float operands scaled so that the float64 distances span at most 13, and the gamma in the middle of them: |gamma - dist| <= 7."""
    gen = torch.Generator().manual_seed(seed)
    ent, sub_e, relb = (torch.randn(n, D, generator=gen) for n in (N, B, B))
    d = L1.dist64(sub_e + relb, ent)
    f = min(1.0, 13.0 / max(float(d.max() - d.min()), 1e-30))
    ent, sub_e, relb = ((f * t).to(DEV) for t in (ent, sub_e, relb))
    d = L1.dist64((sub_e + relb), ent)
    gamma = float(np.float32(0.5 * float(d.max() + d.min())))
    assert float((gamma - d).abs().max()) <= 7.0
    return ent, sub_e, relb, gamma


def run(fn, ent, sub_e, relb, upstream=3.0):
    e, s, r = (t.detach().clone().requires_grad_(True) for t in (ent, sub_e, relb))
    loss = fn(e, s, r)
    (upstream * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), e.grad, s.grad, r.grad


def dense_fn(li, subj, rel, gamma, label_smooth):
    return lambda e, s, r: F.binary_cross_entropy(K.transe_scores_all(e, s, r, gamma), li.labels(subj, rel, label_smooth))


def fused_fn(li, subj, rel, gamma, label_smooth, col_chunk=None):
    return lambda e, s, r: K.transe_bce_all(e, s, r, gamma, li, subj, rel, label_smooth, col_chunk)


def check_against_f64(got, ref, what):
    assert got[0].dtype == torch.float32 and got[0].dim() == 0
    l64 = float(ref[0])
    print(f"{what}: loss {float(got[0]):.9g} vs {l64:.9g}; rel_err g_ent {rel_err(got[1], ref[1]):.2e} g_sub {rel_err(got[2], ref[2]):.2e} "
          f"g_rel {rel_err(got[3], ref[3]):.2e}")
    assert abs(float(got[0]) - l64) <= 1e-4 * max(1.0, l64), what
    for name, g, r in zip(("g_ent", "g_sub", "g_rel"), got[1:], ref[1:]):
        assert rel_err(g, r) <= 1e-4, f"{what} {name}: {rel_err(g, r):.3e}"


# ---- TransE: loss and gradients ------------------------------------------------------------------------------------------------------
# every B of {1, 63, 65, 129}, every N of {1, 63, 64, 65, 449}, every D of {1, 31, 33, 64, 200} (D = 64, 200: float4 staging);
# N = 28 672 + 65 sweeps a second column block (csrc/sweep_host.hpp: BCE_COLS) with both kinds of staging
SHAPES = [(1, 449, 33), (63, 63, 64), (65, 64, 200), (129, 65, 31), (129, 1, 1), (63, 449, 200), (65, 65, 1), (1, 64, 31),
          (5, 28672 + 65, 4), (5, 28672 + 65, 33)]
# label smoothing 0.1 for N >= 10 only: below, the smoothed labels leave [0, 1] and torch's binary_cross_entropy, the dense path's
# loss, rejects them (tests/test_fused_bce_gpu.py)
CASES = [(B, N, D, ls) for B, N, D in SHAPES for ls in (0.0, 0.1) if ls == 0.0 or N >= 10]


@pytest.mark.parametrize("B,N,D,label_smooth", CASES)
def test_transe_float64_accuracy_without_saturation(B, N, D, label_smooth):
    li, subj, rel, y01 = make_index(N, B, seed=B + N)
    if B >= 4:
        assert bool((y01[0] == 1).all()) and float(y01[2].sum()) == 0 and torch.equal(y01[0], y01[3])
        assert N <= 64 or (float(y01[1, 63]) == 1 and float(y01[1, 64]) == 1)
    ent, sub_e, relb, gamma = float_case(B, N, D, seed=D)
    ref = L1.transe_loss64(ent, sub_e, relb, smoothed(y01, li, label_smooth), gamma)
    check_against_f64(run(dense_fn(li, subj, rel, gamma, label_smooth), ent, sub_e, relb), ref, "dense")     # the inputs are fair
    check_against_f64(run(fused_fn(li, subj, rel, gamma, label_smooth), ent, sub_e, relb), ref, "fused")


def int_case(B, N, D, seed):
    """Integer-valued operands: every distance is exact and many coordinates of obj and ent coincide (sgn(0) = 0 in play).  Query 0 is
    entity 5's row (dist 0, x = gamma); query 1 is all 3 against entity 6 all -1 (dist 4 D); from D = 40 on query 2 is entity 7's row
    plus one in 38 coordinates (dist 38: a cell that does not saturate under gamma = 40 however wide the rows are)."""
    gen = torch.Generator().manual_seed(seed)
    ent = torch.randint(-1, 2, (N, D), generator=gen).float()
    sub_e = torch.randint(-1, 2, (B, D), generator=gen).float()
    relb = torch.randint(-1, 3, (B, D), generator=gen).float()
    sub_e[0], relb[0] = ent[5], 0.0
    sub_e[1], relb[1], ent[6] = 1.0, 2.0, -1.0
    if D >= 40:
        sub_e[2], relb[2] = ent[7], 0.0
        relb[2, :38] = 1.0
    return ent.to(DEV), sub_e.to(DEV), relb.to(DEV)


@pytest.mark.parametrize("D", [4, 53, 200])
def test_transe_drop_in_equality_with_the_dense_path_saturation_included(D):
    B, N, gamma = 129, 449, 40.0
    li, subj, rel, y01 = make_index(N, B, seed=7)
    ent, sub_e, relb = int_case(B, N, D, seed=D)
    x = gamma - L1.dist64(sub_e + relb, ent)
    if D >= 53:
        assert float(x.max()) >= 17 and float(x.min()) <= -104
    else:
        assert float(x.max()) == gamma and float(x.min()) == gamma - 4 * D
    assert float(((sub_e + relb).unsqueeze(1) == ent.unsqueeze(0)).float().mean()) > 0.1     # obj == ent coordinates
    dense = run(dense_fn(li, subj, rel, gamma, 0.1), ent, sub_e, relb)
    fused = run(fused_fn(li, subj, rel, gamma, 0.1), ent, sub_e, relb)
    print(f"D={D}: loss fused {float(fused[0]):.9g} dense {float(dense[0]):.9g}; "
          + " ".join(f"{n} {rel_err(g, r):.2e}" for n, g, r in zip(("g_ent", "g_sub", "g_rel"), fused[1:], dense[1:])))
    assert abs(float(fused[0]) - float(dense[0])) <= 1e-6 * float(dense[0])
    for name, g, r in zip(("g_ent", "g_sub", "g_rel"), fused[1:], dense[1:]):
        assert rel_err(g, r) <= 1e-5, f"{name}: {rel_err(g, r):.3e}"
    with torch.no_grad():
        p = K.transe_scores_all(ent, sub_e, relb, gamma)
        sat = (p == 0) | (p == 1)
        assert bool((p == 1).any()) and (D < 53 or bool((p == 0).any()))
        obj = (sub_e + relb).contiguous()
        qkey = (subj.long() * (2 * R) + rel.long()).contiguous()
        v0, v1 = li.label_values(0.1)
        one = torch.ones(1, device=DEV)
        dl = K.transe_bce_dlogit(obj, ent, gamma, li, qkey, v0, v1, 0, N, one)
        assert dl.shape == (B, N) and bool((dl[sat] == 0).all()) and (D < 53 or bool((dl[~sat] != 0).any()))
        part = K.transe_bce_dlogit(obj, ent, gamma, li, qkey, v0, v1, 64, 449, one)       # a column range is the same numbers
        assert torch.equal(part, dl[:, 64:449])


def test_transe_chunking_does_not_matter():
    B, N, D = 129, 449, 33
    li, subj, rel, _ = make_index(N, B, seed=3)
    ent, sub_e, relb, gamma = float_case(B, N, D, seed=11)
    base = run(fused_fn(li, subj, rel, gamma, 0.1, None), ent, sub_e, relb)
    for col_chunk in (64, 128, 449):
        got = run(fused_fn(li, subj, rel, gamma, 0.1, col_chunk), ent, sub_e, relb)
        assert torch.equal(got[0], base[0])
        for name, g, r in zip(("g_ent", "g_sub", "g_rel"), got[1:], base[1:]):
            assert rel_err(g, r) <= 1e-6, f"col_chunk {col_chunk} {name}: {rel_err(g, r):.3e}"


def test_transe_a_batch_that_crosses_a_row_chunk():
    B, N, D = 8192 + 5, 33, 4
    li, subj, rel, y01 = make_index(N, B, seed=5)
    ent, sub_e, relb, gamma = float_case(B, N, D, seed=13)
    ref = L1.transe_loss64(ent, sub_e, relb, smoothed(y01, li, 0.1), gamma)
    check_against_f64(run(fused_fn(li, subj, rel, gamma, 0.1), ent, sub_e, relb), ref, "fused, two row chunks")


@pytest.mark.parametrize("D", [33, 64])
def test_transe_loss_and_gradients_are_bitwise_repeatable(D):
    B, N = 129, 449
    li, subj, rel, _ = make_index(N, B, seed=9)
    ent, sub_e, relb, gamma = float_case(B, N, D, seed=17)
    a = run(fused_fn(li, subj, rel, gamma, 0.1, 128), ent, sub_e, relb)
    b = run(fused_fn(li, subj, rel, gamma, 0.1, 128), ent, sub_e, relb)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_transe_peak_memory_stays_far_below_a_batch_by_entity_matrix():
    """Peak allocation of forward + backward beyond what was there before and the gradients left behind: fused at most a quarter of a
    [B, N] float matrix (the dl slice is 8 MiB against 78 MiB; no transpose, no split table), dense at least two."""
    B, N, D, col_chunk, gamma = 1024, 20000, 52, 2048, 20.0
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, 3 * N), rng.integers(0, R, 3 * N), rng.integers(0, N, 3 * N)], 1)
    li = LabelIndex(tri, R, N, DEV)
    subj, rel = torch.from_numpy(tri[:B, 0]).to(DEV), torch.from_numpy(tri[:B, 1]).to(DEV)
    gen = torch.Generator().manual_seed(0)
    ent, sub_e, relb = ((0.3 * torch.randn(n, D, generator=gen)).to(DEV) for n in (N, B, B))
    matrix = B * N * 4

    def extra(fn):
        e, s, r = (t.detach().clone().requires_grad_(True) for t in (ent, sub_e, relb))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn(e, s, r)
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        return peak - before - sum(t.grad.numel() * 4 for t in (e, s, r)), float(loss.detach())

    fused, lf = extra(fused_fn(li, subj, rel, gamma, 0.1, col_chunk))
    dense, ld = extra(dense_fn(li, subj, rel, gamma, 0.1))
    print(f"peak beyond inputs and gradients: fused {fused / 2 ** 20:.1f} MiB, dense {dense / 2 ** 20:.1f} MiB, [B, N] {matrix / 2 ** 20:.1f} MiB")
    assert abs(lf - ld) <= 1e-4 * max(1.0, ld)
    assert fused <= 0.25 * matrix
    assert dense >= 2 * matrix


# ---- TransE: ranks ---------------------------------------------------------------------------------------------------------------
R_INT = 3


class Side:
    """A filter index given as plain tensors, in the layout evaluation.query_ranks reads."""

    def __init__(self, keys, rowptr, members, gone_at, num_rels=R_INT):
        self.keys, self.num_rels = keys.long().to(DEV), num_rels
        self.rowptr, self.members, self.gone_at = (t.int().contiguous().to(DEV) for t in (rowptr, members, gone_at))


@functools.lru_cache(maxsize=None)
def _dyadic_case(Q, N, D):
    """Entries k / 4: every distance is exact in any order of summation and ties are massive.  The index of test_mrr_gpu.py's _int_case
    on this sweep's edges: gone_at below, equal to and above `when`, an empty list, an unknown key, an unfiltered query, a query with
    everything but the target filtered.  Returns the inputs and the expected ranks from the float64 distances."""
    g = torch.Generator().manual_seed(1000003 * Q + 1009 * N + D)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g)
    ent, obj = ri(-8, 9, (N, D)).float() / 4, ri(-8, 9, (Q, D)).float() / 4
    a, r, t = ri(0, N, (Q,)), ri(0, R_INT, (Q,)), ri(0, N, (Q,))
    t[0], t[Q - 1] = 0, N - 1
    if Q > 4:
        a[Q // 2], r[Q // 2], t[Q // 2], obj[Q // 2] = a[0], r[0], t[0], obj[0]      # a repeated query
    qkey = a * R_INT + r
    when = ri(-1, 10, (Q,))
    if Q > 4:
        when[Q // 2] = when[0]
    edges = [c for c in (0, 63, 64, 127, 128, 447, 448, N - 1) if c < N]
    lists = {}
    if Q > 1:
        lists[int(qkey[1])] = (torch.arange(N), torch.full((N,), MR.INT32_MAX))
    for i in range(Q):
        k = int(qkey[i])
        if k in lists:
            continue
        kind = i % 4
        if kind == 0:
            m = torch.unique(torch.cat((torch.tensor(edges), ri(0, N, (N // 10 + 1,)))))
            lists[k] = (m, ri(0, 10, (m.numel(),)))
        elif kind == 1:
            m = torch.unique(ri(0, N, (N // 2 + 1,)))
            lists[k] = (m, ri(0, 10, (m.numel(),)))
        elif kind == 2:
            lists[k] = (torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64))
    if Q > 2:
        qkey[2] = -1
    keys = torch.tensor(sorted(lists), dtype=torch.int64)
    counts = torch.tensor([lists[int(k)][0].numel() for k in keys], dtype=torch.int64)
    rowptr = torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0)))
    members = torch.cat([lists[int(k)][0] for k in keys]) if len(lists) else torch.empty(0, dtype=torch.int64)
    gone_at = torch.cat([lists[int(k)][1] for k in keys]) if len(lists) else torch.empty(0, dtype=torch.int64)
    d = L1.dist64(obj.to(DEV), ent.to(DEV)).cpu()
    allowed = MR.allowed_mask(N, qkey, when, t, keys, rowptr, members, gone_at)
    return dict(ent=ent.to(DEV), obj=obj.to(DEV), t=t.to(DEV), qkey=qkey.to(DEV), when=when.int().to(DEV),
                side=Side(keys, rowptr, members, gone_at) if len(lists) else None,
                expect=MR.exact_ranks(-d, t, allowed), expect_raw=MR.exact_ranks(-d, t, torch.ones_like(allowed)))


def l1_ranks(c, filtered=True):
    if filtered and c["side"] is not None:
        return EV.query_ranks(c["obj"], c["ent"], c["t"], c["side"], c["when"], c["qkey"], kind="l1").cpu()
    return EV.query_ranks(c["obj"], c["ent"], c["t"], kind="l1").cpu()


# (N = 28 672 + 65: the L1 rank sweep goes through a second column block)
@pytest.mark.parametrize("N,D", [(N, D) for N in (1, 63, 64, 65, 449) for D in (1, 33, 200)] + [(28672 + 65, 1), (28672 + 65, 33)])
def test_transe_dyadic_ranks_are_exact(N, D):
    for Q in (1, 63, 65, 300):
        c = _dyadic_case(Q, N, D)
        got = l1_ranks(c)
        assert torch.equal(got, c["expect"]), f"filtered Q {Q} N {N} D {D}: {int((got != c['expect']).sum())} of {Q} ranks differ"
        if Q > 1:
            assert int(got[1]) == 1                                      # everything but the target filtered
        if Q > 4:
            assert int(got[Q // 2]) == int(got[0])                       # the repeated query
        raw = l1_ranks(c, filtered=False)
        assert torch.equal(raw, c["expect_raw"]), f"raw Q {Q} N {N} D {D}"
        assert int(got.min()) >= 1 and int(raw.max()) <= N


def test_transe_more_queries_than_one_sweep_launch():
    c = _dyadic_case(8192 + 130, 33, 4)
    got = l1_ranks(c)
    assert torch.equal(got, c["expect"]), f"{int((got != c['expect']).sum())} ranks differ"


@pytest.mark.parametrize("D", [33, 64])
def test_transe_duplicates_of_the_target_row_tie_exactly(D):
    """Copies of one random row at ids 10, 150 and 290: whichever is the target, its distance (one thread per query) equals the sweep's
    for the copies bit for bit, so the rank counts exactly the copies at lower ids."""
    N, Q = 300, 70
    gen = torch.Generator().manual_seed(D)
    ent, obj = torch.randn(N, D, generator=gen), torch.randn(Q, D, generator=gen)
    ent[150] = ent[290] = ent[10]
    ent, obj = ent.to(DEV), obj.to(DEV)
    ranks = [EV.query_ranks(obj, ent, torch.full((Q,), t, dtype=torch.int32, device=DEV), kind="l1") for t in (10, 150, 290)]
    assert torch.equal(ranks[1], ranks[0] + 1) and torch.equal(ranks[2], ranks[0] + 2)
    assert int(ranks[0].min()) >= 1 and int(ranks[0].max()) > 1


def test_transe_an_all_zero_table_ranks_by_entity_id():
    N, Q, D = 130, 66, 33
    ent = torch.zeros(N, D, device=DEV)
    obj = torch.randn(Q, D, generator=torch.Generator().manual_seed(1)).to(DEV)
    t = (torch.arange(Q, device=DEV) * 2 - 1).clamp(min=0).int()
    assert torch.equal(EV.query_ranks(obj, ent, t, kind="l1"), 1 + t.long())
    # one list for every query: the even ids, always in force -> only the odd lower ids count
    side = Side(torch.tensor([0]), torch.tensor([0, N // 2]), torch.arange(0, N, 2), torch.zeros(N // 2))
    when = torch.full((Q,), -1, dtype=torch.int32, device=DEV)
    got = EV.query_ranks(obj, ent, t, side, when, torch.zeros(Q, dtype=torch.int64, device=DEV), kind="l1")
    assert torch.equal(got, 1 + (t.long() // 2))


@pytest.mark.parametrize("Q,N,D", [(65, 449, 200), (300, 65, 33), (63, 64, 1)])
def test_transe_float_ranks_lie_in_the_float64_band(Q, N, D):
    c = dict(_dyadic_case(Q, N, D))
    gen = torch.Generator().manual_seed(Q + N + D)
    c["ent"], c["obj"] = torch.randn(N, D, generator=gen).to(DEV), torch.randn(Q, D, generator=gen).to(DEV)
    d = L1.dist64(c["obj"], c["ent"]).cpu()
    side = c["side"]
    allowed = MR.allowed_mask(N, c["qkey"].cpu(), c["when"].cpu(), c["t"].cpu(), side.keys.cpu(), side.rowptr.cpu(), side.members.cpu(),
                              side.gone_at.cpu())
    for got, ok in ((l1_ranks(c), allowed), (l1_ranks(c, filtered=False), torch.ones_like(allowed))):
        lo, hi = L1.l1_rank_band(d, c["t"].cpu(), ok, D)
        assert bool(((got >= lo) & (got <= hi)).all()), f"{int(((got < lo) | (got > hi)).sum())} of {Q} ranks outside the band"
    assert int(got.max()) > 1


# ---- rows into the DistMult sweeps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [50, 52])
def test_rows_rank_equals_distmult_rank_on_the_same_rows(D):
    from test_mrr_gpu import _int_case
    for Q, N in ((129, 449), (300, 225), (1, 33)):
        c = _int_case(Q, N, D)
        emb, w = c["ent"].float().to(DEV), c["rel"].float().to(DEV)
        a, r, t = (c[k].to(DEV) for k in ("a", "r", "t"))
        side = Side(c["keys"], c["rowptr"], c["members"], c["gone_at"])
        when = c["when"].int().to(DEV)
        q = (emb[a] * w[r]).contiguous()
        want = EV.distmult_ranks(emb, w, a, r, t, side, when)
        # distmult_ranks derives qkey = a * num_rels + r itself (the case's unfiltered query 2 is filtered there): hand over the same keys
        got = EV.query_ranks(q, emb, t, side, when, a.long() * R_INT + r.long())
        assert torch.equal(got, want)
        assert torch.equal(EV.query_ranks(q, emb, t), EV.distmult_ranks(emb, w, a, r, t))
        assert torch.equal(EV.query_ranks(q, emb, t).cpu(), c["expect_raw"])
        assert torch.equal(EV.query_ranks(q, emb, t, side, when, c["qkey"].to(DEV)).cpu(), c["expect"])


@pytest.mark.parametrize("D", [50, 64])
def test_dot_bce_all_is_distmult_bce_all_from_the_query_rows_on(D):
    from test_fused_bce_gpu import float_case as dm_case, make_index as dm_index
    B, N = 129, 449
    li, subj, rel, _ = dm_index(N, B, seed=3)
    ent, sub_e, relb = dm_case(B, N, D, seed=11)
    want = run(lambda e, s, r: K.distmult_bce_all(e, s, r, li, subj, rel, 0.1), ent, sub_e, relb)
    got = run(lambda e, s, r: K.dot_bce_all(e, s * r, li, subj, rel, 0.1), ent, sub_e, relb)
    assert torch.equal(got[0], want[0])
    for name, g, r in zip(("g_ent", "g_sub", "g_rel"), got[1:], want[1:]):
        assert rel_err(g, r) <= 1e-6, f"{name}: {rel_err(g, r):.3e}"


# ---- the reference's own numbers ----------------------------------------------------------------------------------------------------
def index_of_dense_labels(label, subj, rel, num_rel, num_ent):
    """A LabelIndex whose lists are the non-zero columns of the rows of a dense label matrix, keys subj * 2R + rel (distinct)."""
    key = subj.long() * (2 * num_rel) + rel.long()
    assert torch.unique(key).numel() == key.numel()
    order = torch.argsort(key)
    li = LabelIndex.__new__(LabelIndex)
    li.num_rel, li.num_ent = int(num_rel), int(num_ent)
    li.keys = key[order].contiguous().to(DEV)
    rows = [torch.nonzero(label[int(i)]).reshape(-1) for i in order]
    li.rowptr = torch.tensor([0] + np.cumsum([r.numel() for r in rows]).tolist(), dtype=torch.int32, device=DEV)
    li.objs = torch.cat(rows).int().contiguous().to(DEV)
    return li


def fixture_step(z, score_args):
    genotype_ = eval(z["genotype"], {"Genotype": S.Genotype})
    g = G.RelGraph(z["N"], z["src"], z["dst"], z["etype"], z["norm"], device=DEV)
    net = S.FixedNetwork(DEV, genotype_, z["N"], z["R"], z["D"], z["D0"], z["nbase"], score_args=score_args).to(DEV)
    net.load_state_dict({**sub(z, "param/"), **sub(z, "buffer0/")})
    net.train()
    subj, rel = z["subj"].to(DEV), z["rel"].to(DEV)
    li = index_of_dense_labels(z["label"], z["subj"], z["rel"], z["R"], z["N"])
    assert torch.equal(li.labels(subj, rel).cpu(), z["label"])
    loss = net.loss_1n(g, subj, rel, li)
    loss.backward()
    return net, loss


def check_fixture_step(z, net, loss, what):
    torch.testing.assert_close(loss.detach().cpu(), z["loss"], rtol=1e-4, atol=1e-6)
    assert sorted(n for n, _ in net.named_parameters()) == sorted(sub(z, "gparam/"))
    for n, p in net.named_parameters():
        assert_param_grad(z, n, p.grad if p.grad is not None else torch.zeros_like(p), 5e-4, 5e-6, what)
    bufs = dict(net.named_buffers())
    for n, ref in sub(z, "buffer/").items():                   # one BatchNorm update per step, not two
        torch.testing.assert_close(bufs[n].cpu(), ref, rtol=1e-4, atol=1e-5)


def test_loss_1n_conve_matches_the_reference():
    z = load_golden("fixednet_conve")
    D, F_, ks, k_w, k_h = (int(v) for v in z["score_args"])
    args = {"gamma": 40.0, "embed_dim": D, "conve_hid_drop": 0.0, "feat_drop": 0.0, "num_filt": F_, "ker_sz": ks, "k_w": k_w, "k_h": k_h}
    _lib.meter.start(["mrg_conve_conv_fwd", "mrg_distmult_bce_fwd", "mrg_linear_fwd"])
    net, loss = fixture_step(z, args)
    rec = _lib.meter.stop()
    assert rec["mrg_conve_conv_fwd"]["launches"] == 1 and rec["mrg_distmult_bce_fwd"]["launches"] == 1
    check_fixture_step(z, net, loss, "fixednet_conve")


def test_loss_1n_transe_matches_the_reference():
    z = load_golden("fixednet_transe")
    assert float(z["unsaturated_fraction"]) > 0.5
    _lib.meter.start(["mrg_transe_bce_fwd", "mrg_transe_score_fwd"])
    net, loss = fixture_step(z, {"gamma": float(z["gamma"])})
    rec = _lib.meter.stop()
    assert rec["mrg_transe_bce_fwd"]["launches"] == 1 and "mrg_transe_score_fwd" not in rec
    check_fixture_step(z, net, loss, "fixednet_transe")


# ---- the network and the evaluation pass -----------------------------------------------------------------------------------------------
def tiny_graph():
    N, T, Rg, D = 200, 1500, 7, 64
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, Rg, T), rng.integers(0, N, T)], 1)
    return N, Rg, D, tri, G.build_train_graph(N, Rg, tri).to(DEV)


CONVE_ARGS = {"embed_dim": 64, "k_h": 8, "k_w": 8, "ker_sz": 3, "num_filt": 4, "conve_hid_drop": 0.3, "feat_drop": 0.3}


def module_of(name):
    """The group of a parameter: its module, as test_fixed_network_loss_fused_matches_loss_on_dense_labels groups them (a module's
    parameters are the columns of one augmented weight; alone, a bias in front of a BatchNorm has a gradient that is mathematically
    zero and no reference magnitude to be relative to).  ConvE's bn0 is such a case as a whole module: its one-channel scale and shift
    act on the image in front of the convolution, and BN1 behind the convolution cancels both (tests/test_conve_gpu.py: CANCELLING).
    bn0 and conv2d are one affine map in front of BN1, so they form one group."""
    module = name.rsplit(".", 1)[0]
    return "score_func.conv2d" if module == "score_func.bn0" else module


@pytest.mark.parametrize("score_func", ["sf_DisMult", "sf_TransE", "sf_ConvE"])
def test_loss_1n_matches_loss_on_dense_labels(score_func):
    N, Rg, D, tri, g = tiny_graph()
    B = 96
    li = LabelIndex(tri, Rg, N, DEV)
    subj = torch.from_numpy(np.concatenate([tri[:B // 2, 0], tri[:B // 2, 2]])).to(DEV)
    rel = torch.from_numpy(np.concatenate([tri[:B // 2, 1], tri[:B // 2, 1] + Rg])).to(DEV)
    torch.manual_seed(1)
    net = S.FixedNetwork(DEV, genotype(score_func), N, Rg, D, D, 5, dropout_cell=0.0, drop_aggr=0.0, score_args=dict(CONVE_ARGS)).to(DEV)
    S.xavier_init_(net)
    net.train()
    if score_func == "sf_DisMult":
        with torch.no_grad():
            net.rel_wt.mul_(0.05)                              # moderate logits: no saturation
    if score_func == "sf_TransE":                              # gamma in the middle of the batch's distances
        with torch.no_grad():
            ent, rel_emb = net.embed(g)
            net.score_func.gamma = float(torch.round(L1.dist64(ent[subj] + rel_emb[rel], ent).median()))
    torch.manual_seed(5)
    loss_d = net._loss(g, subj, rel, li.labels(subj, rel, 0.1))
    loss_d.backward()
    ref = {k: (p.grad.clone() if p.grad is not None else None) for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    torch.manual_seed(5)                                       # ConvE: the same dropout draws
    loss_f = net.loss_1n(g, subj, rel, li, 0.1)
    loss_f.backward()
    torch.cuda.synchronize()
    loss_f, loss_d = float(loss_f.detach()), float(loss_d.detach())
    print(f"{score_func}: loss 1-N {loss_f:.9g} dense {loss_d:.9g}")
    assert abs(loss_f - loss_d) <= 1e-4 * max(1.0, loss_d)
    groups = {}                                                # per module, as test_fixed_network_loss_fused_matches_loss_on_dense_labels groups them
    for k, p in net.named_parameters():
        assert (p.grad is None) == (ref[k] is None), k
        if p.grad is not None:
            groups.setdefault(module_of(k), []).append((p.grad.reshape(-1), ref[k].reshape(-1)))
    for k, parts in groups.items():
        got, want = torch.cat([a for a, _ in parts]), torch.cat([b for _, b in parts])
        print(f"  {k}: rel_err {rel_err(got, want):.2e} (max abs reference {float(want.abs().max()):.2e})")
        assert float(want.abs().max()) > 0 and rel_err(got, want) <= 1e-4, f"{k}: {rel_err(got, want):.3e}"
    assert len(groups) >= 6


class IntegerNet(S.FixedNetwork):
    """The tiny network with prepared integer-valued embeddings after the cells."""

    def embed(self, g):
        return self.int_ent, self.int_rel


@pytest.mark.parametrize("score_func", ["sf_DisMult", "sf_TransE"])
def test_predict_1n_matches_predict_where_float32_sigmoid_is_injective(score_func):
    N, Rg, D, tri, g = tiny_graph()
    li = LabelIndex(tri, Rg, N, DEV)
    net = IntegerNet(DEV, genotype(score_func), N, Rg, D, D, 5, score_args={"gamma": 12.0}).to(DEV)
    gen = torch.Generator().manual_seed(2)
    cols = 16 if score_func == "sf_DisMult" else 8
    net.int_ent, net.int_rel = torch.zeros(N, D), torch.zeros(2 * Rg + 1, D)
    net.int_ent[:, :cols] = torch.randint(-1, 2, (N, cols), generator=gen).float()
    net.int_rel[:, :cols] = torch.randint(-1, 2, (2 * Rg + 1, cols), generator=gen).float()
    net.int_ent, net.int_rel = net.int_ent.to(DEV), net.int_rel.to(DEV)
    test = torch.from_numpy(np.concatenate([tri[:150], np.stack([tri[:150, 2], tri[:150, 1] + Rg, tri[:150, 0]], 1)]))
    s, r = test[:, 0].to(DEV), test[:, 1].to(DEV)
    if score_func == "sf_DisMult":
        x = (net.int_ent[s] * net.int_rel[r]) @ net.int_ent.t()
    else:
        x = 12.0 - L1.dist64(net.int_ent[s] + net.int_rel[r], net.int_ent)
    assert float(x.abs().max()) <= 16
    bs = 64
    batches = [test[i:i + bs] for i in range(0, test.shape[0], bs)]
    loader = [(t, li.labels(t[:, 0].to(DEV), t[:, 1].to(DEV)).cpu()) for t in batches]
    res_d, loss_d = EV.predict(loader, g, net, DEV)
    res_f, loss_f = EV.predict_1n(loader, g, net, li, DEV)
    res_t, loss_t = EV.predict_1n(batches, g, net, li, DEV)                    # triplets alone
    print(f"{score_func}: predict {res_d} {loss_d:.9g}; predict_1n {res_f} {loss_f:.9g}")
    assert res_d["count"] == test.shape[0] and res_d["mr"] > res_d["count"]   # not everything ranks first
    assert res_f == res_d and res_t == res_d
    assert abs(loss_f - loss_d) <= 1e-6 * loss_d and loss_t == loss_f


def test_predict_1n_conve_against_predict_and_the_float64_band():
    N, Rg, D, tri, g = tiny_graph()
    li = LabelIndex(tri, Rg, N, DEV)
    torch.manual_seed(3)
    net = S.FixedNetwork(DEV, genotype("sf_ConvE"), N, Rg, D, D, 5, score_args=dict(CONVE_ARGS)).to(DEV)
    S.xavier_init_(net)
    test = torch.from_numpy(np.concatenate([tri[:100], np.stack([tri[:100, 2], tri[:100, 1] + Rg, tri[:100, 0]], 1)]))
    bs = 64
    batches = [test[i:i + bs] for i in range(0, test.shape[0], bs)]
    loader = [(t, li.labels(t[:, 0].to(DEV), t[:, 1].to(DEV)).cpu()) for t in batches]
    res_d, loss_d = EV.predict(loader, g, net, DEV)
    res_f, loss_f = EV.predict_1n(batches, g, net, li, DEV)
    assert not net.training
    side = EV._LabelSide(li)
    all_ranks = []
    with torch.no_grad():
        ent, rel_emb = net.embed(g)
        for t in batches:
            s, r, o = (t[:, i].to(DEV) for i in range(3))
            q = net.score_func.query(ent[s], rel_emb[r])
            qkey = s.long() * side.num_rels + r.long()
            when = torch.full((s.numel(),), -1, dtype=torch.int32, device=DEV)
            ranks = EV.query_ranks(q, ent, o, side, when, qkey).cpu()
            allowed = MR.allowed_mask(N, qkey.cpu(), when.cpu(), o.cpu(), side.keys.cpu(), side.rowptr.cpu(), side.members.cpu(), side.gone_at.cpu())
            lo, hi = L1.rows_rank_band(q.cpu(), ent.cpu(), o.cpu(), allowed)
            assert bool(((ranks >= lo) & (ranks <= hi)).all())
            all_ranks.append(ranks)
    ranks = torch.cat(all_ranks).double()
    want = {"count": ranks.numel(), "mr": float(ranks.sum()), "mrr": float(ranks.reciprocal().sum())}
    want.update({f"hits@{k}": int((ranks <= k).sum()) for k in (1, 3, 10)})
    print(f"sf_ConvE: predict {res_d} {loss_d:.9g}; predict_1n {res_f} {loss_f:.9g}")
    assert res_f["count"] == want["count"] and all(res_f[f"hits@{k}"] == want[f"hits@{k}"] for k in (1, 3, 10))
    assert abs(res_f["mr"] - want["mr"]) <= 1e-9 * want["mr"] and abs(res_f["mrr"] - want["mrr"]) <= 1e-9 * want["mrr"]
    assert res_f["mr"] > res_f["count"]
    assert abs(loss_f - loss_d) <= 1e-4 * max(1.0, loss_d)
