"""The three-way score-function search leg without a GPU: the C ABI's new entry points, the literal path of MixedOp_SF over
['sf_TransE', 'sf_DisMult', 'sf_ConvE'] against the reference's own MixedOp_SF (tests/golden/make_golden_sf_mix3.py), and what the new
constructor arguments leave as it was."""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden
from mr_gnas_amd import _lib, cell_lp as CL, evaluation as EV, functional as K, operations_lp as O, supernet as S
from mr_gnas_amd.sampler import LabelIndex
import sfmix3_ref as M3

NEW = ["mrg_sfmix3_bce_workspace_bytes", "mrg_sfmix3_bce_fwd", "mrg_sfmix3_bce_grad", "mrg_sfmix3_rank_workspace_bytes", "mrg_sfmix3_rank"]


def test_the_five_entry_points_are_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(f"{ROOT}/include/mrgnas.h").read()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
        assert re.search(r"\b" + name + r"\(", header), name
    assert _lib.load().mrg_abi_version() == 23                 # additive: the ABI number stays
    # argument for argument the two-way entry points, with one more pointer (qh after qd) and, for the gradient, dl2 after dl1
    for name, extra in (("bce_workspace_bytes", 0), ("bce_fwd", 1), ("bce_grad", 2), ("rank_workspace_bytes", 0), ("rank", 1)):
        two, three = _lib.SIGNATURES["mrg_sfmix_" + name], _lib.SIGNATURES["mrg_sfmix3_" + name]
        assert three[0] is two[0] and len(three[1]) == len(two[1]) + extra, name
        assert [t for t in three[1] if t is not ctypes.c_void_p] == [t for t in two[1] if t is not ctypes.c_void_p], name
    for name in ("sf_mix3_bce_all", "sf_mix3_bce_mean", "sf_mix3_bce_grad"):
        assert hasattr(K, name)


def test_argument_errors_come_before_any_device_call():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    assert lib.mrg_sfmix3_bce_workspace_bytes(129, 449, 33) >= 129 * 8 + 3 * 8 * 24     # 3 x 8 tiles, three float64 each
    assert lib.mrg_sfmix3_bce_workspace_bytes(129, 449, 0) == -2 and lib.mrg_sfmix3_bce_workspace_bytes(129, 449, 1025) == -2
    assert lib.mrg_sfmix3_bce_workspace_bytes(1, 0, 8) == -2 and lib.mrg_sfmix3_rank_workspace_bytes(5, 65535 * 7 * 32 + 1, 8) == -2
    assert lib.mrg_sfmix3_rank_workspace_bytes(300, 449, 33) == lib.mrg_sfmix_rank_workspace_bytes(300, 449, 33)
    labels = (p, p, p, p, 3)
    fwd = lambda *a: lib.mrg_sfmix3_bce_fwd(*a)
    assert fwd(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 0, 9, 8, p, p, 1 << 20, None) == 0          # B == 0: nothing launched
    assert fwd(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 0, p, p, 1 << 20, None) == -2
    assert fwd(p, p, None, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 1 << 20, None) == -1      # qh
    assert fwd(p, p, p, p, None, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 1 << 20, None) == -1      # w
    assert fwd(p, p, p, p, p, p, None, p, p, 3, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 1 << 20, None) == -1   # a label pointer with U > 0
    assert fwd(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, p, 16, None) == -4              # workspace too small
    assert fwd(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, p, None, 1 << 20, None) == -4
    grad = lambda *a: lib.mrg_sfmix3_bce_grad(*a)
    assert grad(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 0, 9, 8, 0, 9, p, p, p, p, p, p, 1 << 20, None) == 0
    assert grad(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 3, 3, p, p, p, p, p, p, 1 << 20, None) == -2   # empty column range
    assert grad(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 10, p, p, p, p, p, p, 1 << 20, None) == -2  # c1 > N
    assert grad(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 9, p, p, p, None, p, p, 1 << 20, None) == -1  # dl2
    assert grad(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 9, p, p, p, p, None, p, 1 << 20, None) == -1  # dw
    assert grad(p, p, p, p, p, *labels, 1.0, 0.0, 1.0, 4, 9, 8, 0, 9, p, p, p, p, p, p, 16, None) == -4
    rank = lambda *a: lib.mrg_sfmix3_rank(*a)
    side = (p, p, p, p, p, p, 3)
    assert rank(p, p, p, p, p, 1.0, p, *side, 0, 9, 8, p, p, 1 << 20, None) == 0                  # Q == 0
    assert rank(p, p, p, p, p, 1.0, p, *side, 4, 9, 2000, p, p, 1 << 20, None) == -2
    assert rank(p, p, None, p, p, 1.0, p, *side, 4, 9, 8, p, p, 1 << 20, None) == -1              # qh
    assert rank(p, p, p, p, p, 1.0, None, *side, 4, 9, 8, p, p, 1 << 20, None) == -1              # t_idx
    assert rank(p, p, p, p, p, 1.0, p, p, p, p, p, p, None, 3, 4, 9, 8, p, p, 1 << 20, None) == -1   # gone_at with U > 0
    assert rank(p, p, p, p, p, 1.0, p, *side, 4, 9, 8, p, p, 16, None) == -4


def test_no_cpu_fallback():
    ent, sub = torch.zeros(9, 8), torch.zeros(4, 8)
    w, idx = torch.tensor([0.4, 0.3, 0.3]), torch.zeros(4, dtype=torch.long)
    tri = np.array([[0, 0, 1], [2, 1, 3]])
    li = LabelIndex(tri, 2, 9, "cpu")
    with pytest.raises(_lib.MrgnasError):
        K.sf_mix3_bce_all(ent, sub, sub, sub, w, 3.0, li, idx, idx)
    with pytest.raises(_lib.MrgnasError):
        EV.mix_ranks(sub, sub, ent, w, 3.0, idx, hidden=sub)
    with pytest.raises(ValueError):
        K.sf_mix3_bce_all(ent, sub, sub, sub, w[:2], 3.0, li, idx, idx)
    with pytest.raises(ValueError):
        K.sf_mix3_bce_all(ent, sub, sub, sub[:, :4], w, 3.0, li, idx, idx)
    # the product's own TransE / DistMult scorers have no CPU form: the literal path of loss_1n reaches them and refuses
    cell = CL.Cell_SF(3.0, operations=M3.THREE, sf_args=M3.conve_args(8, 2, 4, 2, 3))
    assert not cell.cell_score._ops[0]._fused_1n(w, ent, sub, sub)
    with pytest.raises(_lib.MrgnasError):
        cell.loss_1n(ent, sub, sub, w.view(1, 3), li, idx, idx)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_the_literal_three_way_mixed_op_reproduces_the_reference(tag):
    torch.set_num_threads(1)
    z = load_golden("sf_mix3_small")
    assert float(z[f"{tag}/unsaturated_fraction"]) > 0.5 and float(z[f"{tag}/unsaturated_fraction_conve"]) > 0.5
    ent, sub, rel = (z[f"{tag}/{k}"].clone().requires_grad_(True) for k in ("ent", "sub", "rel"))
    alpha = z[f"{tag}/alpha"].clone().requires_grad_(True)
    N = ent.shape[0]
    mixed = CL.MixedOp_SF(float(z[f"{tag}/gamma"]), M3.THREE, registry=M3.cpu_sf_registry(), sf_args=M3.conve_args(*z[f"{tag}/conve_shape"]))
    conve = mixed._ops[2][0]
    assert type(conve) is O.sf_ConvE_op and conve.embed_dim == ent.shape[1]
    prefix = f"{tag}/conve/"
    conve.load_state_dict({k[len(prefix):]: v for k, v in z.items() if k.startswith(prefix)})
    mixed.train()
    w = torch.softmax(alpha, dim=1)
    assert not mixed._fused_1n(w[0], ent, sub, rel)
    score = mixed(w[0], ent, sub, rel)
    torch.testing.assert_close(score.detach(), z[f"{tag}/score"], rtol=1e-5, atol=1e-7)
    labels = (1.0 - float(z[f"{tag}/label_smooth"])) * z[f"{tag}/label01"].float() + (1.0 / N)      # reference utils/data_set.py:21-23
    loss = F.binary_cross_entropy(score, labels)
    torch.testing.assert_close(loss.detach(), z[f"{tag}/loss"], rtol=1e-5, atol=0)
    loss.backward()
    grads = [("g_ent", ent.grad), ("g_sub", sub.grad), ("g_rel", rel.grad), ("g_alpha", alpha.grad)]
    grads += [("g_conve/" + k, p.grad) for k, p in conve.named_parameters()]
    assert sorted(k for k in z if k.startswith(f"{tag}/g_conve/")) == sorted(f"{tag}/g_conve/{k}" for k, _ in conve.named_parameters())
    # the same float32 operations as the reference's in the same order: 1e-5 of each gradient's largest entry; the gradients that are
    # sums cancelling to zero in exact arithmetic (a train-mode BatchNorm follows bn0, the conv bias and the fc bias) have no such
    # scale of their own and are held to the conv weight gradient's
    wscale = float(z[f"{tag}/g_conve/conv2d.weight"].abs().max())
    for name, got in grads:
        ref = z[f"{tag}/{name}"]
        scale = float(ref.abs().max())
        if name.endswith(("bn0.weight", "bn0.bias", "conv2d.bias", "fc.bias")):
            scale = max(scale, wscale)
        err = float((got - ref).abs().max())
        assert got.shape == ref.shape and err <= 1e-5 * scale, f"{name}: err {err:.3e} against scale {scale:.3e}"


def test_the_defaults_build_what_they_built_before():
    mixed = CL.MixedOp_SF(7.0, O.SF_OPS)
    assert mixed._args == {'gamma': 7.0} and [type(op[0]) for op in mixed._ops] == [O.sf_TransE_op, O.sf_DisMult_op]
    assert not list(mixed.parameters()) and not list(mixed.buffers()) and mixed._ops[0][0].gamma == 7.0
    assert O.SF_OPS == ['sf_TransE', 'sf_DisMult']
    for cell in (CL.Cell_Final(7.0), CL.Cell_SF(7.0).cell_score):
        assert list(cell._ops[0]._operations) == O.SF_OPS and not list(cell.parameters())
    # sf_args reaches the scorers, gamma included; a ConvE built without them is the reference's D = 200 one
    three = CL.MixedOp_SF(7.0, M3.THREE, sf_args=M3.conve_args(8, 2, 4, 2, 3))
    assert three._ops[0][0].gamma == 7.0 and three._ops[2][0].embed_dim == 8 and three._ops[2][0].fc.in_features == 3 * 3 * 3
    assert CL.MixedOp_SF(7.0, M3.THREE)._ops[2][0].embed_dim == 200

    def build(**kw):
        torch.manual_seed(3)
        net = S.ScoreSearchNetwork("cpu", 4, 1, 1, 1, 1, 1, 8, 8, 2, 1.0, 0.0, 0.0, sf_registry=M3.cpu_sf_registry(), **kw)
        return net, torch.rand(3)                              # the generator's state after construction
    torch.manual_seed(3)
    plain = S.SearchNetwork("cpu", 4, 1, 1, 1, 1, 1, 8, 8, 2, 1.0, 0.0, 0.0)
    after_plain = torch.rand(3)
    net, after = build()
    assert sorted(net.state_dict()) == sorted(plain.state_dict()) and torch.equal(after, after_plain)
    assert [a.shape for a in net.arch_parameters()] == [a.shape for a in plain.arch_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(net.arch_parameters(), plain.arch_parameters()))
    assert net.sf_ops == O.SF_OPS and net.arch_parameters()[4].shape == (1, 2)
    net3, _ = build(sf_ops=M3.THREE, sf_args=M3.conve_args(8, 2, 4, 2, 3))
    assert net3.arch_parameters()[4].shape == (1, 3) and net3.arch_parameters()[4].requires_grad
    assert all(torch.equal(a, b) for a, b in zip(net3.arch_parameters()[:4], plain.arch_parameters()[:4]))
    assert any(k.startswith("score_func.cell_score._ops.0._ops.2.0.fc") for k in net3.state_dict())
    for k, name in enumerate(M3.THREE):                        # the argmax follows the alpha
        with torch.no_grad():
            net3.arch_parameters()[4].copy_(torch.eye(3)[k:k + 1])
        assert net3.show_genotypes()[-1].score_func == name
