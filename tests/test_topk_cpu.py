"""Top-k link prediction (mrg_rows_topk, mrg_transe_topk, evaluation.query_topk / predict_topk) without a GPU: the entry points exist,
argument errors come back before any launch, the workspaces do not grow with N or hold a [Q, N] matrix, nothing falls back to the CPU,
and the float64 restatement the GPU tests compare against orders as the issue of ties demands."""
import ctypes

import numpy as np
import pytest
import torch

from mr_gnas_amd import _lib, evaluation as EV, graph as G, supernet as S
import topk_ref as TK

P = ctypes.c_void_p
NEW = ("mrg_rows_topk", "mrg_transe_topk", "mrg_rows_topk_workspace_bytes", "mrg_transe_topk_workspace_bytes")
BCE_COLS = 7 * 32 * 128
KINDS = [("mrg_rows_topk", "mrg_rows_topk_workspace_bytes"), ("mrg_transe_topk", "mrg_transe_topk_workspace_bytes")]


def test_the_entry_points_are_declared_and_the_abi_stays():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 23 and lib.mrg_abi_version() == 23


def _topk(lib, which, q=P(256), ent=P(256), qkey=P(256), when=P(256), keys=P(256), rowptr=P(256), members=P(256), gone_at=P(256), U=3,
          Q=8, N=100, D=64, k=10, ids=P(256), vals=P(256), ws=P(256), ws_bytes=1 << 40):
    return getattr(lib, which)(q, ent, qkey, when, keys, rowptr, members, gone_at, U, Q, N, D, k, ids, vals, ws, ws_bytes, None)


@pytest.mark.parametrize("which,need", KINDS)
def test_argument_errors_without_gpu(which, need):
    lib = _lib.load()
    need = getattr(lib, need)
    for name in ("q", "ent", "ids", "vals", "qkey", "when", "keys", "rowptr", "members", "gone_at"):
        assert _topk(lib, which, **{name: None}) == -1, name
    assert _topk(lib, which, k=0) == -2 and _topk(lib, which, k=65) == -2 and _topk(lib, which, k=-1) == -2
    assert _topk(lib, which, D=0) == -2 and _topk(lib, which, D=1028) == -2 and _topk(lib, which, N=0) == -2
    assert _topk(lib, which, Q=-1) == -2 and _topk(lib, which, U=-1) == -2 and _topk(lib, which, q=None, k=0) == -2
    n = need(8, 100, 64, 10)
    assert n > 0 and _topk(lib, which, ws=None) == -4 and _topk(lib, which, ws_bytes=n - 1) == -4
    assert _topk(lib, which, k=1, ws_bytes=need(8, 100, 64, 1) - 1) == -4 and _topk(lib, which, k=64, ws_bytes=need(8, 100, 64, 64) - 1) == -4
    assert _topk(lib, which, Q=0, q=None, ent=None, ws=None, ws_bytes=0) == 0
    # raw: the index may be NULL as a whole with U == 0 (the call then fails on the workspace, the next check)
    assert _topk(lib, which, U=0, qkey=None, when=None, keys=None, rowptr=None, members=None, gone_at=None, ws_bytes=0) == -4


@pytest.mark.parametrize("which,need", KINDS)
def test_workspace_queries(which, need):
    lib = _lib.load()
    need = getattr(lib, need)
    for k in (0, 65):
        assert need(256, 1000, 64, k) == -2
    assert need(256, 0, 64, 10) == -2
    # the row GEMM's cores take D <= 256 or a multiple of 4; the L1 sweep takes every D <= 1024 (the rank entry points' rule)
    assert need(256, 1000, 257, 10) == (-2 if which == "mrg_rows_topk" else need(256, 1000, 256, 10))
    assert need(256, 1000, 1025, 10) == -2 and need(-1, 1000, 64, 10) == -2
    assert need(0, 1000, 64, 10) >= 0
    # N enters through one column block only
    for Q, D, k in ((256, 256, 10), (256, 200, 64), (4096, 33, 1)):
        assert need(Q, 1_000_000, D, k) == need(Q, 2 * BCE_COLS, D, k) > 0
    # per query: the four integers of the prepared filter (the running list is the output); the partial lists are per chunk
    for D, k in ((200, 10), (64, 64), (33, 1)):
        for N in (33, 14541, 1_000_000):
            grow = need(4 * 8192, N, D, k) - need(8192, N, D, k)
            assert 0 <= grow <= 64 * 3 * 8192, (N, D, k, grow)
    # no [Q, N] matrix
    Q, N = 4096, 14541
    assert 0 < need(Q, N, 200, 10) < Q * N * 4 // 4
    assert 0 < need(256, 1_000_000, 256, 10) < 256 * 1_000_000 * 4 // 16
    assert need(256, 1_000_000, 256, 64) <= need(256, 1_000_000, 256, 10) + (16 << 20)     # the lists stay within their budget


def _tiny(score_func="sf_DisMult", args=None):
    N, R, T, D = 40, 3, 120, 8
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)], 1)
    geno = [S.Genotype(alpha_cell=[('pre_sub', 1, 0), ('a_sum', 2, 1)], concat_node=[2], score_func=score_func)]
    return N, R, tri, S.FixedNetwork("cpu", geno, N, R, D, D, 2, score_args=args)


@pytest.mark.parametrize("score_func", ["sf_DisMult", "sf_TransE", "sf_ConvE"])
def test_no_cpu_fallback(score_func):
    N, R, tri, net = _tiny(score_func, {"embed_dim": 8, "k_h": 4, "k_w": 2, "ker_sz": 2, "num_filt": 2})
    subj, rel = torch.from_numpy(tri[:5, 0]), torch.from_numpy(tri[:5, 1])
    ent = torch.randn(N, 8)
    for kind in ("dot", "l1"):
        with pytest.raises(_lib.MrgnasError):
            EV.query_topk(ent[subj], ent, 3, kind=kind)
    g = G.build_train_graph(N, R, tri)
    with pytest.raises(_lib.MrgnasError):
        EV.predict_topk(net, g, subj, rel, 3)
    with pytest.raises(_lib.MrgnasError):
        net.predict_topk(g, subj, rel, 3)


def test_k_out_of_range_names_the_dense_forward():
    q, ent = torch.zeros(2, 8), torch.zeros(5, 8)
    for k in (0, 65, -3):
        with pytest.raises(ValueError, match="dense forward"):
            EV.query_topk(q, ent, k)
    with pytest.raises(ValueError):
        EV.query_topk(q, ent, 3, kind="cosine")


def test_predict_topk_names_a_scorer_without_a_query():
    N, R, tri, net = _tiny()

    class Bare(torch.nn.Module):
        def forward(self, all_ent, sub_emb, rel_emb):
            return torch.sigmoid(sub_emb @ all_ent.t())

    net.score_func = Bare()
    with pytest.raises(_lib.MrgnasError, match="Bare"):
        net.predict_topk(None, torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), 3)


def test_the_float64_restatement_orders_ties_by_id_and_pads():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0], [2.0, 2.0, 2.0, 2.0, 2.0]], dtype=torch.float64)
    allowed = torch.tensor([[True, True, False, True, True], [False, False, False, True, False]])
    ids, vals = TK.topk64("dot", x, allowed, 4)
    assert ids.tolist() == [[1, 4, 0, 3], [3, -1, -1, -1]]
    assert vals[0].tolist() == [3.0, 3.0, 1.0, 0.0] and vals[1, 0] == 2.0 and bool((vals[1, 1:] == float("-inf")).all())
    ids, vals = TK.topk64("l1", x, allowed, 7)                  # k > N
    assert ids.tolist() == [[3, 0, 1, 4, -1, -1, -1], [3, -1, -1, -1, -1, -1, -1]] and bool((vals[0, 4:] == float("inf")).all())
    keys, rowptr = torch.tensor([2, 5]), torch.tensor([0, 2, 2])
    members, gone_at = torch.tensor([1, 3]), torch.tensor([4, 5])
    ok = TK.allowed_mask(4, torch.tensor([2, 2, 5, 7, -1]), torch.tensor([3, 4, 0, 0, 0]), keys, rowptr, members, gone_at)
    assert ok.tolist() == [[True, False, True, False], [True, True, True, False], [True] * 4, [True] * 4, [True] * 4]
