"""The scorer-general 1-N loss and evaluation (csrc/transe_1n.hip, mrg_rows_rank, functional.transe_bce_all / dot_bce_all,
FixedNetwork.loss_1n, evaluation.query_ranks / predict_1n) without a GPU: the entry points exist, argument errors come back before any
launch, the workspaces hold no [B, N] matrix, nothing falls back to the CPU, and the scorers' ``query`` is what their forward scores."""
import ctypes

import numpy as np
import pytest
import torch

from mr_gnas_amd import _lib, evaluation as EV, functional as K, graph as G, operations_lp as O, supernet as S
from mr_gnas_amd.sampler import LabelIndex
import l1_ref as L1

P = ctypes.c_void_p
NEW = ("mrg_rows_rank", "mrg_transe_bce_workspace_bytes", "mrg_transe_bce_fwd", "mrg_transe_bce_dlogit", "mrg_transe_dist_bwd",
       "mrg_transe_rank_workspace_bytes", "mrg_transe_rank")
RANK_MAX_N = 65535 * 7 * 32


def test_the_entry_points_are_declared_and_the_abi_stays():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 23 and lib.mrg_abi_version() == 23


def _fwd(lib, obj=P(256), ent=P(256), qkey=P(256), keys=P(256), rowptr=P(256), objs=P(256), U=3, B=8, N=100, D=64, loss=P(256),
         ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_transe_bce_fwd(obj, ent, qkey, keys, rowptr, objs, U, 40.0, 0.0, 1.0, B, N, D, loss, ws, ws_bytes, None)


def _dlogit(lib, obj=P(256), ent=P(256), qkey=P(256), keys=P(256), rowptr=P(256), objs=P(256), U=3, B=8, N=100, D=64, c0=0, c1=100,
            gscale=P(256), dl=P(256), ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_transe_bce_dlogit(obj, ent, qkey, keys, rowptr, objs, U, 40.0, 0.0, 1.0, B, N, D, c0, c1, gscale, dl, ws, ws_bytes, None)


def test_loss_argument_errors_without_gpu():
    lib = _lib.load()
    need = lib.mrg_transe_bce_workspace_bytes
    for fn, required in ((_fwd, ("obj", "ent", "loss")), (_dlogit, ("obj", "ent", "gscale", "dl"))):
        for name in required + ("qkey", "keys", "rowptr", "objs"):
            assert fn(lib, **{name: None}) == -1, (fn.__name__, name)
        assert fn(lib, D=0) == -2 and fn(lib, D=-4) == -2 and fn(lib, D=1025) == -2
        assert fn(lib, N=RANK_MAX_N + 1) == -2 and fn(lib, N=0) == -2 and fn(lib, B=-1) == -2 and fn(lib, U=-1) == -2
        assert fn(lib, obj=None, D=0) == -2 and fn(lib, obj=None, ws=None) == -1
        n = need(8, 100, 64)
        assert n > 0
        assert fn(lib, ws=None) == -4 and fn(lib, ws_bytes=n - 1) == -4 and fn(lib, ws_bytes=0) == -4
        assert fn(lib, B=0, obj=None, ent=None, ws=None, ws_bytes=0) == 0
    assert _fwd(lib, N=RANK_MAX_N, ws_bytes=0) == -4                        # the largest N passes the shape check
    assert _dlogit(lib, c0=-1) == -2 and _dlogit(lib, c0=10, c1=10) == -2 and _dlogit(lib, c0=11, c1=10) == -2 and _dlogit(lib, c1=101) == -2
    assert need(-1, 10, 64) == -2 and need(8, 0, 64) == -2 and need(8, 100, 0) == -2 and need(8, RANK_MAX_N + 1, 64) == -2
    assert need(0, 100, 64) >= 0


def test_dist_bwd_argument_errors_without_gpu():
    lib = _lib.load()

    def bwd(ent_c=P(256), obj=P(256), dl=P(256), ld=100, gent=P(256), gobj=P(256), B=8, nc=100, D=64):
        return lib.mrg_transe_dist_bwd(ent_c, obj, dl, ld, gent, gobj, 0, B, nc, D, None)

    for name in ("ent_c", "obj", "dl"):
        assert bwd(**{name: None}) == -1, name
    assert bwd(B=-1) == -2 and bwd(nc=0) == -2 and bwd(D=0) == -2 and bwd(ld=99) == -2 and bwd(B=8 * 65535 + 1) == -2
    assert bwd(dl=None, D=0) == -2
    assert bwd(B=0, ent_c=None, obj=None, dl=None) == 0


def _rank(lib, which, q=P(256), ent=P(256), t=P(256), qkey=P(256), when=P(256), keys=P(256), rowptr=P(256), members=P(256),
          gone_at=P(256), U=3, Q=8, N=100, D=64, ranks=P(256), ws=P(256), ws_bytes=1 << 40):
    return getattr(lib, which)(q, ent, t, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, ranks, ws, ws_bytes, None)


@pytest.mark.parametrize("which,need", [("mrg_transe_rank", "mrg_transe_rank_workspace_bytes"),
                                        ("mrg_rows_rank", "mrg_distmult_rank_workspace_bytes")])
def test_rank_argument_errors_without_gpu(which, need):
    lib = _lib.load()
    need = getattr(lib, need)
    for name in ("q", "ent", "t", "ranks", "qkey", "when", "keys", "rowptr", "members", "gone_at"):
        assert _rank(lib, which, **{name: None}) == -1, name
    assert _rank(lib, which, D=0) == -2 and _rank(lib, which, D=1028) == -2 and _rank(lib, which, N=0) == -2
    assert _rank(lib, which, N=RANK_MAX_N + 1) == -2 and _rank(lib, which, Q=-1) == -2 and _rank(lib, which, U=-1) == -2
    assert _rank(lib, which, q=None, D=0) == -2
    n = need(8, 100, 64)
    assert n > 0 and _rank(lib, which, ws=None) == -4 and _rank(lib, which, ws_bytes=n - 1) == -4
    assert _rank(lib, which, Q=0, q=None, ent=None, ws=None, ws_bytes=0) == 0
    # raw ranks: the index may be NULL as a whole with U == 0 (the call then fails on the workspace, the next check)
    assert _rank(lib, which, U=0, qkey=None, when=None, keys=None, rowptr=None, members=None, gone_at=None, ws_bytes=0) == -4


def test_workspaces_hold_no_batch_by_entity_tensor():
    """B = 256, N = 1 M, D = 256: a [B, N] float matrix is 1 GB.  The loss workspace is two integers per query and one float64 per
    tile of 64 x 64 elements; the rank workspace does not depend on N at all."""
    lib = _lib.load()
    need = lib.mrg_transe_bce_workspace_bytes
    B, N, D = 256, 1_000_000, 256
    partials = lambda n: 8 * ((B + 63) // 64) * ((n + 63) // 64 + 1)
    assert 0 < need(B, N, D) < B * N * 4 // 16
    assert need(B, N, D) <= 8 * B + partials(N) + 1024
    assert need(B, 2 * N, D) - need(B, N, D) <= partials(N) + 256           # grows with N by the partials alone
    assert need(B, N, 4) == need(B, N, D)                                   # no operand copy: D does not enter
    rank = lib.mrg_transe_rank_workspace_bytes
    assert rank(B, N, D) == rank(B, 1, D) and 0 < rank(B, N, D) <= 24 * B + 1024


def _tiny(score_func="sf_DisMult", args=None):
    N, R, T, D = 40, 3, 120, 8
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)], 1)
    geno = [S.Genotype(alpha_cell=[('pre_sub', 1, 0), ('a_sum', 2, 1)], concat_node=[2], score_func=score_func)]
    net = S.FixedNetwork("cpu", geno, N, R, D, D, 2, score_args=args)
    return N, R, tri, net


@pytest.mark.parametrize("score_func", ["sf_DisMult", "sf_TransE", "sf_ConvE"])
def test_no_cpu_fallback(score_func):
    N, R, tri, net = _tiny(score_func, {"embed_dim": 8, "k_h": 4, "k_w": 2, "ker_sz": 2, "num_filt": 2})
    li = LabelIndex(tri, R, N, "cpu")
    subj, rel = torch.from_numpy(tri[:5, 0]), torch.from_numpy(tri[:5, 1])
    ent, w = torch.randn(N, 8), torch.randn(2 * R + 1, 8)
    with pytest.raises(_lib.MrgnasError):
        K.transe_bce_all(ent, ent[subj], w[rel], 40.0, li, subj, rel)
    with pytest.raises(_lib.MrgnasError):
        K.dot_bce_all(ent, ent[subj] * w[rel], li, subj, rel)
    with pytest.raises(_lib.MrgnasError):
        EV.query_ranks(ent[subj], ent, subj, kind="l1")
    g = G.build_train_graph(N, R, tri)
    with pytest.raises(_lib.MrgnasError):
        net.loss_1n(g, subj, rel, li)
    with pytest.raises(_lib.MrgnasError):
        EV.predict_1n([torch.from_numpy(tri[:5])], g, net, li, "cpu")


def test_loss_1n_names_a_scorer_without_a_query():
    N, R, tri, net = _tiny()

    class Bare(torch.nn.Module):
        def forward(self, all_ent, sub_emb, rel_emb):
            return torch.sigmoid(sub_emb @ all_ent.t())

    net.score_func = Bare()
    li = LabelIndex(tri, R, N, "cpu")
    with pytest.raises(_lib.MrgnasError, match="Bare"):
        net.loss_1n(None, torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), li)
    with pytest.raises(ValueError):
        EV.query_ranks(torch.zeros(1, 8), torch.zeros(4, 8), torch.zeros(1, dtype=torch.long), kind="cosine")


def test_query_is_the_row_the_forward_scores():
    gen = torch.Generator().manual_seed(0)
    sub, rel, ent = (torch.randn(n, 16, generator=gen) for n in (5, 5, 9))
    te, dm = O.sf_TransE_op({"gamma": 7.0}), O.sf_DisMult_op({})
    assert te.score_kind == "l1" and dm.score_kind == "dot" and O.sf_ConvE_op.score_kind == "dot" and te.gamma == 7.0
    assert torch.equal(te.query(sub, rel), sub + rel) and torch.equal(dm.query(sub, rel), sub * rel)
    op = O.sf_ConvE_op({"embed_dim": 16, "k_h": 4, "k_w": 4, "ker_sz": 3, "num_filt": 5})
    with torch.no_grad():
        for p in op.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=gen))
        op.bn2.running_mean.add_(0.3)
    op.eval()
    with torch.no_grad():
        q = op.query(sub, rel)
        assert q.shape == (5, 16) and float(q.min()) >= 0 and float(q.max()) > 0
        assert torch.equal(torch.sigmoid(q @ ent.t()), op(ent, sub, rel))


@pytest.mark.parametrize("D", [1, 31, 33, 64, 200])
def test_the_float32_chain_stays_within_its_bound_of_float64(D):
    gen = torch.Generator().manual_seed(D)
    obj, ent = torch.randn(65, D, generator=gen), torch.randn(129, D, generator=gen)
    d32, d64 = L1.chain_dist32(obj, ent).double(), L1.dist64(obj, ent)
    assert bool(((d32 - d64).abs() <= L1.chain_bound(D, d64)).all())
    # dyadic data: every order of summation is exact
    obj, ent = (torch.randint(-8, 9, s, generator=gen).float() / 4 for s in ((65, D), (129, D)))
    assert torch.equal(L1.chain_dist32(obj, ent).double(), L1.dist64(obj, ent))
