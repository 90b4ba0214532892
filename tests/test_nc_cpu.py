"""Node-classification task on CPU tensors (no GPU): the full-neighbour block builder against the fixtures' blocks, the operator and
network contracts recorded from the reference (tests/golden/make_golden_nc.py), the import hygiene of operations_nc, the row-kind
check of the genotype wiring, and the torch formulation of the operators and the network against the reference's values."""
import collections
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import load_golden

from mr_gnas_amd import graph as G, sampler as SM
from mr_gnas_amd import model_nc as MN, operations_nc as ON

Genotype = collections.namedtuple("Genotype", "alpha_cell concat_node score_func", defaults=(None,))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, what, rtol=1e-4, atol=2e-5, rms_rtol=1e-4):
    """The bounds of tests/test_ops_gpu.py's close(): the largest error against the largest entry (floored at 1), and the rms error
    against the rms."""
    a, b = a.detach().cpu(), b.detach().cpu()
    scale = float(b.abs().max()) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= atol + rtol * max(scale, 1.0), f"{what}: max err {err:.3e} (scale {scale:.3e})"
    if b.numel() and rms_rtol is not None:
        rms_b = float(b.double().square().mean().sqrt())
        rms_e = float((a.double() - b.double()).square().mean().sqrt())
        assert rms_e <= rms_rtol * rms_b + 1e-9, f"{what}: rms err {rms_e:.3e} against rms {rms_b:.3e}"


def grads_close(net, z, tag, rtol, atol=5e-6):
    """Every parameter gradient against the reference's (absent from the fixture: no gradient there, none or zero here)."""
    for n, p in net.named_parameters():
        ref = z.get(f"{tag}/gparam/{n}")
        if ref is None:
            assert p.grad is None or not p.grad.any(), n
        else:
            torch.testing.assert_close(p.grad.cpu(), ref, rtol=rtol, atol=atol, msg=lambda m: f"{tag} {n} grad: {m}")


def _n(z, prefix):
    return int(z["N"]) if prefix == "" else int(z[prefix + "args"][0])


def fixture_blocks(z, prefix):
    out = []
    for j in range(int(z[prefix + "n_blocks"])):
        p = f"{prefix}block{j}/"
        out.append(G.Block(z[p + "src_nid"], z[p + "dst_nid"], z[p + "src"], z[p + "dst"], z[p + "eid"], z[p + "etype"]))
    return out


def assert_blocks_equal(got, ref):
    assert len(got) == len(ref)
    for j, (a, b) in enumerate(zip(got, ref)):
        for what, x, y in (("src", a.edges()[0], b.edges()[0]), ("dst", a.edges()[1], b.edges()[1]),
                           ("EID", a.edata[G.EID], b.edata[G.EID]), ("ETYPE", a.edata[G.ETYPE], b.edata[G.ETYPE]),
                           ("src NID", a.srcdata[G.NID], b.srcdata[G.NID]), ("dst NID", a.dstdata[G.NID], b.dstdata[G.NID])):
            assert x.dtype == torch.int64, (j, what)
            assert torch.equal(x.cpu(), y.cpu()), f"block {j}: {what} differs"
        assert a.number_of_nodes() == a.number_of_dst_nodes() == b.number_of_dst_nodes()
        assert a.number_of_src_nodes() == b.number_of_src_nodes()


@pytest.mark.parametrize("case", ["ops", "n0", "n1", "s1"])
def test_full_neighbor_blocks_match_the_fixture(case):
    if case == "ops":
        z, prefix = load_golden("nc_ops_small"), ""
        seeds, layers = z["seeds"], int(z["layers"])
    else:
        z, prefix = load_golden("nc_fixednet_small"), case + "/"
        seeds, layers = z[prefix + "seeds"], int(z[prefix + "args"][8])
    g = G.RelGraph(_n(z, prefix), z[prefix + "gsrc"], z[prefix + "gdst"])
    g.edata[G.ETYPE] = z[prefix + "getype"].long()
    blocks = SM.full_neighbor_blocks(g, seeds, layers)
    assert_blocks_equal(blocks, fixture_blocks(z, prefix + "blocks/"))
    for j in range(layers - 1):                                     # block j's destinations are block j + 1's sources, in order
        assert torch.equal(blocks[j].dstdata[G.NID], blocks[j + 1].srcdata[G.NID])
    assert blocks[0].ndata is blocks[0].dstdata


def test_block_protocol():
    b = G.Block(torch.tensor([4, 2, 9]), torch.tensor([4, 2]), torch.tensor([2, 0, 1]), torch.tensor([0, 0, 1]), torch.tensor([7, 3, 5]),
                torch.tensor([1, 0, 1]))
    assert (G.EID, G.NID, G.ETYPE) == ("_ID", "_ID", "_TYPE")
    assert b.number_of_nodes() == b.number_of_dst_nodes() == 2 and b.number_of_src_nodes() == 3 and b.num_edges() == 3
    assert b.srcdata is not b.dstdata and b.ndata is b.dstdata
    with b.local_scope():
        b.srcdata["h"] = torch.zeros(3)
        b.edata["m"] = torch.zeros(3)
    assert "h" not in b.srcdata and "m" not in b.edata
    assert torch.equal(b.in_degrees(), torch.tensor([2, 1]))


def test_operator_contract_matches_the_reference():
    z = load_golden("nc_ops_small")
    c = json.loads(z["contract"])
    assert list(ON.MIXED_OPS) == c["MIXED_OPS"]
    assert (ON.PRE_OPS, ON.FIRST_OPS, ON.MIDDLE_OPS, ON.LAST_OPS) == (c["PRE_OPS"], c["FIRST_OPS"], c["MIDDLE_OPS"], c["LAST_OPS"])
    assert "a_std" not in ON.PRE_OPS + ON.FIRST_OPS + ON.MIDDLE_OPS + ON.LAST_OPS
    D = int(z["D"])
    for name, ctor in ON.MIXED_OPS.items():
        op = ctor({"feature_dim": D})
        assert type(op).__name__ == c["classes"][name]
        assert [[n, list(p.shape)] for n, p in op.named_parameters()] == c["params"][name], name
    assert ON.pre_corr_op.__name__ == "pre_corr_op" and "pre_corr" not in ON.MIXED_OPS


def genotypes(z, tag):
    return eval(str(z[tag + "/genotype"]), {"Genotype": Genotype})


def make_net(z, tag, device="cpu"):
    N, T, R, classes, D, D0, nbase, batch, layers, op_norm = [int(v) for v in z[tag + "/args"]]
    args = types.SimpleNamespace(feature_dim=D, op_norm=bool(op_norm))
    net = MN.Network(torch.device(device), genotypes(z, tag), N, classes, R, layers, 1, 3, D, D0, nbase, torch.nn.CrossEntropyLoss(), args)
    net.load_state_dict({k[len(tag) + 8:]: v for k, v in z.items() if k.startswith(tag + "/param0/")})
    return net.to(device)


@pytest.mark.parametrize("tag", ["n0", "n1", "s1"])
def test_network_state_dict_keys_match_the_reference(tag):
    z = load_golden("nc_fixednet_small")
    net = make_net(z, tag)
    assert list(net.state_dict().keys()) == json.loads(z[tag + "/state_keys"])


def test_import_leaves_tensor_indexing_alone():
    code = ("import sys, torch; sys.path.insert(0, %r); before = torch.Tensor.__getitem__; "
            "import mr_gnas_amd.operations_nc, mr_gnas_amd.model_nc; "
            "assert torch.Tensor.__getitem__ is before; assert 'mr_gnas_amd.operations_lp' not in sys.modules; print('ok')"
            % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


MIXED_WIRINGS = [
    # a concat over an edge-row node (2) and a destination-row node (3)
    [('pre_sub', 1, 0), ('f_identity', 2, 1), ('a_sum', 3, 2)],
    # f_dense with src_emb on destination rows and src_emb_in on edge rows
    [('pre_sub', 1, 0), ('a_mean', 2, 1), ('f_dense', 3, 2)],
    # an aggregator over destination rows
    [('pre_sub', 1, 0), ('a_max', 2, 1), ('a_std', 3, 2)],
    # a node summing edge rows and destination rows
    [('pre_sub', 1, 0), ('a_sum', 2, 1), ('f_identity', 3, 1), ('f_identity', 3, 2)],
]


@pytest.mark.parametrize("k", range(len(MIXED_WIRINGS)))
def test_row_kind_mismatch_raises(k):
    cells = MIXED_WIRINGS[k]
    concat = [2, 3] if k == 0 else [3]
    args = types.SimpleNamespace(feature_dim=8, op_norm=False)
    with pytest.raises(ValueError):
        MN.Network(torch.device("cpu"), [Genotype(cells, concat)], 20, 3, 4, 1, 1, 3, 8, 4, 3, torch.nn.CrossEntropyLoss(), args)


def test_edge_only_cell_output_raises():
    args = types.SimpleNamespace(feature_dim=8, op_norm=False)
    with pytest.raises(ValueError):
        MN.Cell(args, Genotype([('pre_sub', 1, 0), ('f_identity', 2, 1)], [1, 2]))


def test_operator_row_checks():
    b = G.Block(torch.arange(3), torch.arange(2), torch.tensor([2, 0, 1]), torch.tensor([0, 0, 1]), torch.arange(3))
    x3, x2 = torch.randn(3, 4), torch.randn(2, 4)
    with pytest.raises(ValueError):
        ON.f_dense_op({"feature_dim": 4})(b, x2, x3)
    with pytest.raises(ValueError):
        ON.a_std_op({"feature_dim": 4})(b, x2, x3)


def test_cpu_operators_match_the_reference():
    """The torch formulation the operators run on CPU operands, against the reference's values (fixture nc_ops_small)."""
    z = load_golden("nc_ops_small")
    (blk,) = fixture_blocks(z, "blocks/")
    D = int(z["D"])
    for name, ctor in ON.MIXED_OPS.items():
        op = ctor({"feature_dim": D})
        op.load_state_dict({k[len(name) + 7:]: v for k, v in z.items() if k.startswith(name + "/param/")})
        last, agg = name.endswith("_last"), name.startswith("a_")
        a = (z["xd"] if last else z["x"]).clone().requires_grad_(True)
        b = z["y"].clone().requires_grad_(True)
        out = op(blk, a, b)
        out.backward(z["gd"] if (last or agg) else z["ge"])
        close(out, z[name + "/out"], name)
        close(a.grad if a.grad is not None else torch.zeros_like(a), z[name + "/ga"], name + " ga")
        if name + "/gb" in z:
            close(b.grad, z[name + "/gb"], name + " gb")
        for n, p in op.named_parameters():
            close(p.grad, z[f"{name}/gparam/{n}"], f"{name}.{n} grad")


@pytest.mark.parametrize("tag", ["n0", "n1", "s1"])
def test_cpu_network_matches_the_reference(tag):
    z = load_golden("nc_fixednet_small")
    net = make_net(z, tag)
    blocks = fixture_blocks(z, tag + "/blocks/")
    seeds = z[tag + "/seeds"].long()
    net.train()
    logits = net(z[tag + "/trip_index"], blocks)
    loss = net._criterion(logits, z[tag + "/labels"][seeds])
    loss.backward()
    close(logits, z[tag + "/logits"], "logits")
    close(loss.reshape(1), z[tag + "/loss"].reshape(1), "loss")
    grads_close(net, z, tag, 5e-4)
    net.eval()
    with torch.no_grad():
        close(net(z[tag + "/trip_index"], blocks), z[tag + "/logits_eval"], "eval logits")
