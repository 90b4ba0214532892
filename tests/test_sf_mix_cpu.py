"""The score-function search leg without a GPU: the C ABI's new entry points, supernet.ScoreSearchNetwork's literal path against the
reference's Cell_SF (tests/golden/make_golden_sf_mix.py), and architect.Architect driving the fifth architecture parameter."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden
from mr_gnas_amd import _lib, cell_lp as CL, evaluation as EV, functional as K, graph as G, operations_lp as O, supernet as S
from mr_gnas_amd.architect import Architect
from mr_gnas_amd.sampler import LabelIndex
import sfmix_ref as MX

NEW = ["mrg_sfmix_bce_workspace_bytes", "mrg_sfmix_bce_fwd", "mrg_sfmix_bce_grad", "mrg_sfmix_rank_workspace_bytes", "mrg_sfmix_rank"]


def test_the_five_entry_points_are_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert _lib.load().mrg_abi_version() == 23
    for name in ("sf_mix_bce_all", "sf_mix_bce_mean", "sf_mix_bce_grad"):
        assert hasattr(K, name)


def test_argument_errors_come_before_any_device_call():
    lib = _lib.load()
    P = ctypes.c_void_p
    p = P(256)
    assert lib.mrg_sfmix_bce_workspace_bytes(129, 449, 33) >= 129 * 8 + 3 * 8 * 16      # 3 x 8 tiles, two float64 each
    assert lib.mrg_sfmix_bce_workspace_bytes(129, 449, 0) == -2 and lib.mrg_sfmix_bce_workspace_bytes(129, 449, 1025) == -2
    assert lib.mrg_sfmix_bce_workspace_bytes(1, 0, 8) == -2 and lib.mrg_sfmix_rank_workspace_bytes(5, 65535 * 7 * 32 + 1, 8) == -2
    assert lib.mrg_sfmix_rank_workspace_bytes(300, 449, 33) >= 300 * 24
    labels = (p, p, p, p, 3)
    fwd = lambda *a: lib.mrg_sfmix_bce_fwd(*a)
    assert fwd(p, p, p, p, *labels, 1.0, 0.0, 1.0, 0, 9, 8, p, p, 1 << 20, None) == 0             # B == 0: nothing launched
    assert fwd(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 0, p, p, 1 << 20, None) == -2
    assert fwd(p, None, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 1 << 20, None) == -1         # qd
    assert fwd(p, p, p, None, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 1 << 20, None) == -1         # w
    assert fwd(p, p, p, p, p, None, p, p, 3, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 1 << 20, None) == -1   # a label pointer with U > 0
    assert fwd(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 16, None) == -4                 # workspace too small
    assert fwd(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, None, 1 << 20, None) == -4
    grad = lambda *a: lib.mrg_sfmix_bce_grad(*a)
    assert grad(p, p, p, p, *labels, 1.0, 0.0, 1.0, 0, 9, 8, 0, 9, p, p, p, p, p, 1 << 20, None) == 0
    assert grad(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 3, 3, p, p, p, p, p, 1 << 20, None) == -2   # empty column range
    assert grad(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 10, p, p, p, p, p, 1 << 20, None) == -2  # c1 > N
    assert grad(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 9, p, p, None, p, p, 1 << 20, None) == -1  # dl1
    assert grad(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 9, p, p, p, None, p, 1 << 20, None) == -1  # dw
    assert grad(p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 9, p, p, p, p, p, 16, None) == -4
    rank = lambda *a: lib.mrg_sfmix_rank(*a)
    side = (p, p, p, p, p, p, 3)
    assert rank(p, p, p, p, 1.0, p, *side, 0, 9, 8, p, p, 1 << 20, None) == 0                     # Q == 0
    assert rank(p, p, p, p, 1.0, p, *side, 4, 9, 2000, p, p, 1 << 20, None) == -2
    assert rank(p, p, p, p, 1.0, None, *side, 4, 9, 8, p, p, 1 << 20, None) == -1                 # t_idx
    assert rank(p, p, p, p, 1.0, p, p, p, p, p, p, None, 3, 4, 9, 8, p, p, 1 << 20, None) == -1   # gone_at with U > 0
    assert rank(p, p, p, p, 1.0, p, *side, 4, 9, 8, p, p, 16, None) == -4


def test_no_cpu_fallback():
    ent, sub = torch.zeros(9, 8), torch.zeros(4, 8)
    w, idx = torch.tensor([0.5, 0.5]), torch.zeros(4, dtype=torch.long)
    tri = np.array([[0, 0, 1], [2, 1, 3]])
    li = LabelIndex(tri, 2, 9, "cpu")
    with pytest.raises(_lib.MrgnasError):
        K.sf_mix_bce_all(ent, sub, sub, w, 3.0, li, idx, idx)
    with pytest.raises(_lib.MrgnasError):
        EV.mix_ranks(sub, sub, ent, w, 3.0, idx)
    with pytest.raises(_lib.MrgnasError):
        EV.predict_mix([torch.from_numpy(tri)], ent, sub, w, 3.0, li, "cpu")
    with pytest.raises(ValueError):
        K.sf_mix_bce_all(ent, sub, sub[:, :4], w, 3.0, li, idx, idx)
    # the product's own scorers have no CPU form either: the literal path of loss_1n reaches them and refuses
    cell = CL.Cell_SF(3.0)
    assert not cell.cell_score._ops[0]._fused_1n(w, ent, sub, sub)
    with pytest.raises(_lib.MrgnasError):
        cell.loss_1n(ent, sub, sub, w.view(1, 2), li, idx, idx)


def fixture_labels(z, tag, N):
    return (1.0 - float(z[f"{tag}/label_smooth"])) * z[f"{tag}/label01"].float() + (1.0 / N)      # reference utils/data_set.py:21-23


class BareScoreNet(S.ScoreSearchNetwork):
    """A ScoreSearchNetwork whose embeddings after the cells are handed in: get_loss from there on."""

    def __init__(self, gamma, alpha):
        super().__init__("cpu", 4, 1, 1, 1, 1, 1, 4, 4, 2, gamma, 0.0, 0.0, sf_registry=MX.cpu_sf_registry())
        self.load_alpha(self.arch_parameters()[:4] + [alpha])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_score_search_network_dense_labels_reproduce_the_reference_cell(tag):
    torch.set_num_threads(1)
    z = load_golden("sf_mix_small")
    assert float(z[f"{tag}/unsaturated_fraction"]) > 0.5
    ent, sub, rel = (z[f"{tag}/{k}"].clone().requires_grad_(True) for k in ("ent", "sub", "rel"))
    B, N = sub.shape[0], ent.shape[0]
    net = BareScoreNet(float(z[f"{tag}/gamma"]), z[f"{tag}/alpha"])
    assert not list(net.score_func.parameters()) and not list(net.score_func.buffers())
    assert sorted(net.state_dict()) == sorted(S.SearchNetwork("cpu", 4, 1, 1, 1, 1, 1, 4, 4, 2, 1.0, 0.0, 0.0).state_dict())
    torch.testing.assert_close(net.score_weights().detach(), torch.softmax(z[f"{tag}/alpha"], dim=1), rtol=1e-6, atol=0)
    score = net.score_func(ent, sub, rel, net.score_weights())
    torch.testing.assert_close(score.detach(), z[f"{tag}/score"], rtol=1e-5, atol=1e-7)
    # get_loss gathers ent[subj] and rel[r]: hand it tables whose rows 0 .. B - 1 are the fixture's sub / rel rows behind the entities
    table = torch.cat((ent, sub))
    data = torch.stack((torch.arange(B) + N, torch.arange(B)), 1)
    dense = fixture_labels(z, tag, N)
    loss = F.binary_cross_entropy(net.score_func(ent, table[data[:, 0]], rel[data[:, 1]], net.score_weights()), dense)
    torch.testing.assert_close(loss.detach(), z[f"{tag}/loss"], rtol=1e-5, atol=0)
    loss.backward()
    alpha = net.arch_parameters()[4]
    for name, got in (("g_ent", ent.grad), ("g_sub", sub.grad), ("g_rel", rel.grad), ("g_alpha", alpha.grad)):
        ref = z[f"{tag}/{name}"]
        err = float((got - ref).abs().max())
        assert err <= 1e-5 * float(ref.abs().max()), f"{name}: err {err:.3e} against max {float(ref.abs().max()):.3e}"
    # ... and get_loss itself with dense labels is that expression: entities = the table, so the labels get B zero columns for the
    # appended rows, which changes the number: compare against the same expression, bit for bit
    alpha.grad = None
    wide = torch.cat((dense, torch.full((B, B), 1.0 / N)), 1)
    got = net.get_loss(None, table.detach(), rel.detach(), data, wide)
    want = F.binary_cross_entropy(net.score_func(table.detach(), table.detach()[data[:, 0]], rel.detach(), net.score_weights()), wide)
    assert torch.equal(got.detach(), want.detach())
    got.backward()
    assert float(alpha.grad.abs().max()) > 0


def tiny_search_case(cls, **kw):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cpu_kernels as CK
    n, R, D, B = 40, 3, 8, 12
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, n, 160), rng.integers(0, R, 160), rng.integers(0, n, 160)], 1)
    g = G.build_search_graph(n, R, tri)
    src, _, _ = g.edges(form="all")
    node_id = torch.arange(n).view(-1, 1)
    torch.manual_seed(0)

    class OnCpu(cls):
        """The forward as the reference's caller writes it (SearchNetwork._forward_reference): plain tensors, no HIP gather."""

        def forward(self, *a):
            return self._forward_reference(*a)
    net = OnCpu("cpu", n, R, 2, 1, 2, 2, D, 8, 2 * R + 1, 4.0, 0.0, 0.0, registry=CK.wrapped_registry(), **kw)
    net.train()
    return net, (g, node_id, src, g.edata["e_type"]), tri, n, R, B


ARGS = types.SimpleNamespace(momentum=0.9, weight_decay=3e-4, arch_learning_rate=3e-3, arch_weight_decay=1e-3)


def test_architect_step_reaches_all_five_alphas_and_the_genotype_names_a_score_function():
    net, graph, tri, n, R, B = tiny_search_case(S.ScoreSearchNetwork, sf_registry=MX.cpu_sf_registry())
    data = torch.from_numpy(tri[:B, :2])
    labels = torch.zeros(B, n)                                 # the multi-hot labels of (subj, rel), smoothed (utils/data_set.py:21-33)
    for i, (s, r) in enumerate(tri[:B, :2].tolist()):
        labels[i, tri[(tri[:, 0] == s) & (tri[:, 1] == r), 2]] = 1.0
    labels = 0.9 * labels + 1.0 / n
    before = [a.detach().clone() for a in net.arch_parameters()]
    architect = Architect("cpu", net, ARGS)
    architect.step(*graph, data, labels, *graph, data, labels, None, None, False)
    for i, a in enumerate(net.arch_parameters()):
        assert a.grad is not None and float(a.grad.abs().max()) > 0, i
        assert not torch.equal(a.detach(), before[i]), i
    state = architect.optimizer.state
    assert all(int(state[a]["step"]) == 1 for a in net.arch_parameters())
    genos = net.show_genotypes()
    assert genos[-1].score_func == O.SF_OPS[int(net.score_weights()[0].argmax())] and genos[-1].score_func in O.SF_OPS
    assert all(gt.score_func is None for gt in genos[:-1]) and len(genos) == 2
    with torch.no_grad():                                      # the argmax follows the alpha
        net.arch_parameters()[4].copy_(torch.tensor([[-1.0, 1.0]]))
    assert net.show_genotypes()[-1].score_func == "sf_DisMult"
    with torch.no_grad():
        net.arch_parameters()[4].copy_(torch.tensor([[1.0, -1.0]]))
    assert net.show_genotypes()[-1].score_func == "sf_TransE"
    assert net.show_genotype(1).alpha_cell == S.SearchNetwork.show_genotype(net, 1).alpha_cell


def test_a_plain_search_network_is_unchanged():
    net, graph, tri, n, R, B = tiny_search_case(S.SearchNetwork)
    gen = torch.Generator().manual_seed(1)
    triplets = torch.from_numpy(tri[:B])
    labels = (torch.rand(B, generator=gen) < 0.5).float()
    architect = Architect("cpu", net, ARGS)
    architect.step(*graph, triplets, labels, *graph, triplets, labels, None, None, False)
    alphas = net.arch_parameters()
    assert all(a.grad is not None for a in alphas[:4]) and alphas[4].grad is None
    assert all(gt.score_func is None for gt in net.show_genotypes())
    assert not hasattr(net, "score_func")
