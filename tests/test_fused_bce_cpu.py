"""The 1-N DistMult loss without [B, N] tensors (csrc/bce.hip, functional.distmult_bce_all, FixedNetwork.loss_fused,
evaluation.predict_fused) without a GPU: the entry points exist, argument errors come back before any launch, the workspace holds
no [B, N] matrix, and nothing falls back to the CPU."""
import ctypes

import numpy as np
import pytest
import torch

from mr_gnas_amd import _lib, evaluation as EV, functional as K, graph as G, supernet as S
from mr_gnas_amd.sampler import LabelIndex

P = ctypes.c_void_p
NEW = ("mrg_distmult_bce_workspace_bytes", "mrg_distmult_bce_fwd", "mrg_distmult_bce_dlogit")
RANK_MAX_N = 65535 * 7 * 32


def test_the_entry_points_are_declared_and_the_abi_stays():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 23 and lib.mrg_abi_version() == 23


def _fwd(lib, q=P(256), ent=P(256), qkey=P(256), keys=P(256), rowptr=P(256), objs=P(256), U=3, B=8, N=100, D=64, loss=P(256),
         ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_distmult_bce_fwd(q, ent, qkey, keys, rowptr, objs, U, 0.0, 1.0, B, N, D, loss, ws, ws_bytes, None)


def _dlogit(lib, q=P(256), ent=P(256), qkey=P(256), keys=P(256), rowptr=P(256), objs=P(256), U=3, B=8, N=100, D=64, c0=0, c1=100,
            gscale=P(256), dl=P(256), ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_distmult_bce_dlogit(q, ent, qkey, keys, rowptr, objs, U, 0.0, 1.0, B, N, D, c0, c1, gscale, dl, ws, ws_bytes, None)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    need = lib.mrg_distmult_bce_workspace_bytes
    for fn, required in ((_fwd, ("q", "ent", "loss")), (_dlogit, ("q", "ent", "gscale", "dl"))):
        # a required pointer is NULL -> -1; the index is required as a whole once U > 0, and not at all with U == 0
        for name in required + ("qkey", "keys", "rowptr", "objs"):
            assert fn(lib, **{name: None}) == -1, (fn.__name__, name)
        # sizes the kernels do not cover -> -2, and a shape error wins over a NULL pointer
        assert fn(lib, D=0) == -2 and fn(lib, D=-4) == -2 and fn(lib, D=1028) == -2 and fn(lib, D=257) == -2
        assert fn(lib, N=RANK_MAX_N + 1) == -2 and fn(lib, N=0) == -2 and fn(lib, B=-1) == -2 and fn(lib, U=-1) == -2
        assert fn(lib, q=None, D=0) == -2 and fn(lib, q=None, ws=None) == -1
        # workspace missing or too small -> MRG_E_WORKSPACE
        n = need(8, 100, 64)
        assert n > 0
        assert fn(lib, ws=None) == -4 and fn(lib, ws_bytes=n - 1) == -4 and fn(lib, ws_bytes=0) == -4
        # B == 0: nothing to do, nothing launched, whatever else is NULL
        assert fn(lib, B=0, q=None, ent=None, ws=None, ws_bytes=0) == 0
    assert _fwd(lib, N=RANK_MAX_N, ws_bytes=0) == -4                        # the largest N passes the shape check
    # the column range of the logit gradient lies inside [0, N) and is not empty
    assert _dlogit(lib, c0=-1) == -2 and _dlogit(lib, c0=10, c1=10) == -2 and _dlogit(lib, c1=101) == -2
    assert need(-1, 10, 64) == -2 and need(8, 0, 64) == -2 and need(8, 100, 0) == -2 and need(8, RANK_MAX_N + 1, 64) == -2
    assert need(0, 100, 64) >= 0


def test_workspace_holds_no_batch_by_entity_tensor():
    """The project's largest configuration: B = 256, N = 1 M, D = 256.  A [B, N] float matrix is 1 GB; the workspace is the split of
    one block of 28 672 entity rows, two integers per query and one float64 per workgroup."""
    need = _lib.load().mrg_distmult_bce_workspace_bytes
    B, N, D = 256, 1_000_000, 256
    split_block = (D // 16) * (28672 // 32) * 3 * 64 * 16
    assert 0 < need(B, N, D) <= split_block + 8 * B + 8 * (B // 128) * (N // 224 + 2) + 4096
    assert need(B, N, D) < B * N * 4 // 16                                 # a twenty-third of ONE [B, N] float matrix
    assert need(B, 2 * N, D) - need(B, N, D) <= 8 * (B // 128) * (N // 224 + 2) + 256      # grows with N by the partials alone
    assert need(B, N, 50) < need(B, N, 52) and need(B, N, 50) <= 8 * B + 8 * (B // 128) * (N // 224 + 2) + 4096   # exact core: no split


def test_default_col_chunk_is_a_multiple_of_the_column_block_within_64_mib():
    for B in (1, 256, 1000, 8197, 10 ** 6):
        c = K.bce_default_col_chunk(B)
        assert c % 224 == 0 and c >= 224 and (c == 224 or 4 * B * c <= 64 << 20 < 4 * B * (c + 224))


def _tiny(score_func="sf_DisMult"):
    N, R, T, D = 40, 3, 120, 8
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)], 1)
    geno = [S.Genotype(alpha_cell=[('pre_sub', 1, 0), ('a_sum', 2, 1)], concat_node=[2], score_func=score_func)]
    net = S.FixedNetwork("cpu", geno, N, R, D, D, 2)
    return N, R, tri, net


def test_no_cpu_fallback():
    N, R, tri, net = _tiny()
    li = LabelIndex(tri, R, N, "cpu")
    subj, rel = torch.from_numpy(tri[:5, 0]), torch.from_numpy(tri[:5, 1])
    ent, w = torch.randn(N, 8), torch.randn(2 * R + 1, 8)
    with pytest.raises(_lib.MrgnasError):
        K.distmult_bce_all(ent, ent[subj], w[rel], li, subj, rel)
    g = G.build_train_graph(N, R, tri)
    with pytest.raises(_lib.MrgnasError):
        net.loss_fused(g, subj, rel, li)
    with pytest.raises(_lib.MrgnasError):
        EV.predict_fused([torch.from_numpy(tri[:5])], g, net, li, "cpu")


def test_loss_fused_names_a_scorer_it_does_not_cover():
    N, R, tri, net = _tiny("sf_TransE")
    li = LabelIndex(tri, R, N, "cpu")
    with pytest.raises(_lib.MrgnasError, match="sf_TransE"):
        net.loss_fused(None, torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), li)
