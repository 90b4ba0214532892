"""calc_mrr on HIP (mr_gnas_amd.evaluation, csrc/rank.hip) without a GPU: the filter index and its removal-order semantics against
the reference's ranks (tests/golden/make_golden_mrr.py), argument validation before any launch, and the workspace rule."""
import ctypes

import pytest
import torch

from conftest import load_golden
from mr_gnas_amd import _lib, evaluation as EV
import mrr_ref as MR

P = ctypes.c_void_p
NEW = ("mrg_distmult_rank", "mrg_distmult_rank_workspace_bytes")


def test_the_entry_points_are_declared():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)


def _passes(z, known, when_s, when_o):
    """The four (a, r, target, side, when) of a fixture: pass S perturbs the subject, pass O the object."""
    s, r, o = z["test"][:, 0], z["test"][:, 1], z["test"][:, 2]
    return (("ranks_s", o, r, s, known.subject, when_s), ("ranks_o", s, r, o, known.object, when_o))


def _ranks(z, a, r, target, side, when):
    N = z["emb"].shape[0]
    if side is None:
        allowed = torch.ones(target.numel(), N, dtype=torch.bool)
    else:
        allowed = MR.allowed_mask(N, a * side.num_rels + r, when, target, side.keys, side.rowptr, side.members, side.gone_at)
    return MR.exact_ranks(MR.scores64(z["emb"], z["w"], a, r), target, allowed)


@pytest.mark.parametrize("case", ["mrr_small", "mrr_odd"])
def test_index_semantics_reproduce_the_reference_ranks(case):
    """KnownTriples on CPU tensors + a float64 restatement of the score and the rank rule = the reference's four rank vectors, exactly
    (the fixtures' seeds separate every target from every competitor by more than the float32 error bound)."""
    z = load_golden(case)
    N, R, T = z["emb"].shape[0], z["w"].shape[0], z["test"].shape[0]
    known = EV.KnownTriples(z["train"], z["valid"], z["test"], N, R)
    for side in (known.subject, known.object):
        assert side.rowptr.dtype == side.members.dtype == side.gone_at.dtype == torch.int32 and side.keys.dtype == torch.int64
        assert bool((side.keys[1:] > side.keys[:-1]).all()) and int(side.rowptr[-1]) == side.members.numel() == side.gone_at.numel()
        for u in range(side.keys.numel()):
            m = side.members[int(side.rowptr[u]):int(side.rowptr[u + 1])]
            assert m.numel() > 0 and bool((m[1:] > m[:-1]).all())
    distinct = {tuple(t) for t in torch.cat([z["train"], z["valid"], z["test"]]).tolist()}
    assert known.subject.members.numel() == known.object.members.numel() == len(distinct)
    # gone_at: the first test triple equal to the member's triple, else INT32_MAX (the duplicate test triple 1 = 0 goes at 0)
    first = {}
    for i, t in enumerate(z["test"].tolist()):
        first.setdefault(tuple(t), i)
    side = known.object
    for u in range(side.keys.numel()):
        s, r = int(side.keys[u]) // R, int(side.keys[u]) % R
        for j in range(int(side.rowptr[u]), int(side.rowptr[u + 1])):
            assert int(side.gone_at[j]) == first.get((s, r, int(side.members[j])), MR.INT32_MAX)
    when_s, when_o = torch.arange(T, dtype=torch.int32), torch.full((T,), T, dtype=torch.int32)
    for name, a, r, target, side, when in _passes(z, known, when_s, when_o):
        assert torch.equal(_ranks(z, a, r, target, side, when), z["filtered_" + name]), f"filtered {name}"
        assert torch.equal(_ranks(z, a, r, target, None, None), z["raw_" + name]), f"raw {name}"
    both = torch.cat([z["filtered_ranks_s"], z["filtered_ranks_o"]])
    assert abs(float((1.0 / both.float()).mean()) - float(z["filtered_mrr"])) <= 2 * T * 2.0 ** -23


def test_the_standard_protocol_is_another_function():
    """when = -1 (filter every known triple but the query's own) changes ranks on the small fixture: it may not be the default."""
    z = load_golden("mrr_small")
    T = z["test"].shape[0]
    known = EV.KnownTriples(z["train"], z["valid"], z["test"], z["emb"].shape[0], z["w"].shape[0])
    minus1 = torch.full((T,), -1, dtype=torch.int32)
    got = torch.cat([_ranks(z, a, r, target, side, when) for _, a, r, target, side, when in _passes(z, known, minus1, minus1)])
    ref = torch.cat([z["filtered_ranks_s"], z["filtered_ranks_o"]])
    assert int((got != ref).sum()) > 0 and bool((got <= ref).all())       # filtering more can only improve a rank


def _call(lib, ent=P(256), rel=P(256), a=P(256), r=P(256), t=P(256), qkey=None, when=None, keys=None, rowptr=None, members=None,
          gone_at=None, U=0, Q=8, N=100, D=64, ranks=P(256), ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_distmult_rank(ent, rel, a, r, t, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, ranks, ws, ws_bytes, None)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    # a required pointer is NULL -> -1; the index is required as a whole once U > 0
    for name in ("ent", "rel", "a", "r", "t", "ranks"):
        assert _call(lib, **{name: None}) == -1, name
    idx = dict(qkey=P(256), when=P(256), keys=P(256), rowptr=P(256), members=P(256), gone_at=P(256))
    for name in idx:
        assert _call(lib, U=3, **{**idx, name: None}) == -1, name
    # negative sizes, sizes the kernels do not cover, an entity count that t_idx (int32) / the grid cannot address -> -2
    assert _call(lib, Q=-1) == -2 and _call(lib, N=0) == -2 and _call(lib, N=-5) == -2 and _call(lib, D=0) == -2 and _call(lib, D=-4) == -2
    assert _call(lib, U=-1) == -2 and _call(lib, D=1028) == -2 and _call(lib, D=257) == -2
    assert _call(lib, N=2 ** 31) == -2 and _call(lib, N=2 ** 40) == -2
    assert lib.mrg_distmult_rank_workspace_bytes(-1, 10, 64) == -2 and lib.mrg_distmult_rank_workspace_bytes(8, 0, 64) == -2
    assert lib.mrg_distmult_rank_workspace_bytes(8, 100, 0) == -2
    # a shape error wins over a NULL pointer, a NULL pointer over the workspace
    assert _call(lib, ent=None, D=0) == -2 and _call(lib, ent=None, ws=None) == -1
    # workspace missing or too small -> -4
    need = lib.mrg_distmult_rank_workspace_bytes(8, 100, 64)
    assert need > 0
    assert _call(lib, ws=None) == -4 and _call(lib, ws_bytes=need - 1) == -4 and _call(lib, ws_bytes=0) == -4
    # Q == 0: nothing to do, nothing launched, whatever else is NULL
    assert _call(lib, Q=0, ent=None, ranks=None, ws=None, ws_bytes=0) == 0
    assert lib.mrg_distmult_rank_workspace_bytes(0, 100, 64) >= 0


def test_workspace_holds_no_query_by_entity_tensor():
    """FB15k-237: Q = 2 x 20 466 queries, N = 14 541, D = 200.  A [Q, N] float matrix is 2.4 GB; the workspace is the entity table's
    split plus operands of a bounded chunk of queries plus O(Q) integers."""
    lib = _lib.load()
    ws = lib.mrg_distmult_rank_workspace_bytes
    Q, N, D = 40932, 14541, 200
    ent_split = -(-D // 16) * (-(-N // 224) * 7) * 3 * 64 * 16            # k-slabs x column tiles (padded to blocks of 7) x 3 planes x 1 KB
    assert 0 < ws(Q, N, D) < 64 * 2 ** 20 + ent_split
    assert ws(Q, N, D) < Q * N // 8                                        # not even a bit per (query, candidate)
    # growth: O(Q) in the queries at fixed N, D (a few integers per query), O(N D) in the entities at fixed Q
    assert ws(10 * Q, N, D) - ws(Q, N, D) <= 9 * Q * 64
    assert ws(Q, 2 * N, D) - ws(Q, N, D) <= 2 * N * D * 6 + (1 << 20)
    # the exact-core shapes need no split at all
    assert ws(Q, N, 50) < ws(Q, N, 52) and ws(Q, N, 50) <= 2 * 8192 * 50 * 4 + Q * 24 + 4096


def test_no_cpu_fallback():
    z = load_golden("mrr_small")
    with pytest.raises(_lib.MrgnasError):
        EV.calc_mrr(z["emb"], z["w"], z["train"], z["valid"], z["test"], hits=[1, 3, 10])
    with pytest.raises(_lib.MrgnasError):
        EV.calc_mrr(z["emb"], z["w"], z["train"], z["valid"], z["test"], hits=[1], eval_p="raw")
    with pytest.raises(_lib.MrgnasError):
        EV.distmult_ranks(z["emb"], z["w"], z["test"][:, 0], z["test"][:, 1], z["test"][:, 2])
