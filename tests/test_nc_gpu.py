"""Node-classification task on the MI355X: every operator of operations_nc (reference models/operations.py) forward + backward
against the reference's fixture, a_std (csrc/segstd.hip) against a float64 restatement at random shapes (hub, empty and degree-1
destinations, equal messages, odd D), bit-reproducibility, HIP graph capture, the HIP entry points taken, the device block builder
against the CPU one, and model_nc.Network (reference models/model.py) against the reference's training step and eval forward."""
import pytest
import torch

from conftest import load_golden
from test_nc_cpu import close, fixture_blocks, grads_close, make_net

from mr_gnas_amd import _lib, graph as G, sampler as SM
from mr_gnas_amd import functional as K, operations_nc as ON

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_operators_match_the_reference():
    z = load_golden("nc_ops_small")
    (blk,) = fixture_blocks(z, "blocks/")
    blk = blk.to(DEV)
    assert int(blk.in_degrees().max()) >= 2048
    D = int(z["D"])
    for name, ctor in ON.MIXED_OPS.items():
        op = ctor({"feature_dim": D})
        op.load_state_dict({k[len(name) + 7:]: v for k, v in z.items() if k.startswith(name + "/param/")})
        op = op.to(DEV)
        last, agg = name.endswith("_last"), name.startswith("a_")
        a = (z["xd"] if last else z["x"]).to(DEV).requires_grad_(True)
        b = z["y"].to(DEV).requires_grad_(True)
        out = op(blk, a, b)
        assert out.is_cuda and out.dtype == torch.float32
        out.backward((z["gd"] if (last or agg) else z["ge"]).to(DEV))
        close(out, z[name + "/out"], name)
        close(a.grad if a.grad is not None else torch.zeros_like(a), z[name + "/ga"], name + " ga")
        if name + "/gb" in z:
            close(b.grad, z[name + "/gb"], name + " gb")
        for n, p in op.named_parameters():
            close(p.grad, z[f"{name}/gparam/{n}"], f"{name}.{n} grad")


def std_block(D, seed):
    """A block of 300 destinations: a hub of 9 000 in-edges, 40 without in-edges, 60 of in-degree 1, the rest 2..12; the edge list
    shuffled; destination 101 (in-degree 5) receives equal messages in every column, destination 102 in column 0 only."""
    gen = torch.Generator().manual_seed(seed)
    n_dst, n_src = 300, 500
    deg = torch.randint(2, 13, (n_dst,), generator=gen)
    deg[0], deg[1:41], deg[41:101], deg[101], deg[102] = 9000, 0, 1, 5, 6
    dst = torch.repeat_interleave(torch.arange(n_dst), deg)
    dst = dst[torch.randperm(dst.numel(), generator=gen)]
    E = int(dst.numel())
    src = torch.randint(0, n_src, (E,), generator=gen)
    blk = G.Block(torch.arange(n_src), torch.arange(n_dst), src, dst, torch.arange(E))
    x = torch.randn(E, D, generator=gen) * 2 + 0.5
    x[dst == 101] = 0.75
    x[dst == 102, 0] = -1.5
    return blk, x, torch.randn(n_dst, D, generator=gen)


def std_ref64(x, blk):
    """The reference's formula (models/operations.py:168-190) in float64 on the host, with its autograd gradient."""
    _, dst = blk.edges()
    dst = dst.cpu()
    x = x.detach().cpu().double().requires_grad_(True)
    n = blk.number_of_nodes()
    deg = torch.bincount(dst, minlength=n).double().view(-1, 1)
    d1 = deg.clamp(min=1)
    mean = torch.zeros(n, x.shape[1], dtype=torch.float64).index_add(0, dst, x) / d1
    msq = torch.zeros(n, x.shape[1], dtype=torch.float64).index_add(0, dst, x * x) / d1
    out = torch.where(deg > 0, torch.sqrt(torch.relu(msq - mean * mean) + 1e-5), torch.zeros_like(mean))
    return x, out


@pytest.mark.parametrize("D", [1, 7, 64, 200, 256])
def test_a_std_against_float64(D):
    blk, x, g = std_block(D, 100 + D)
    xr, ref = std_ref64(x, blk)
    ref.backward(g.double())
    b = blk.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = K.aggregate_std(xd, b)
    out.backward(g.to(DEV))
    close(out, ref.float(), f"a_std D={D}")
    close(xd.grad, xr.grad.float(), f"a_std grad D={D}")
    o = out.cpu()
    assert torch.equal(o[1:41], torch.zeros(40, D))                                     # no in-edges: 0
    eps = torch.tensor(1e-5, dtype=torch.float64).sqrt().float()
    assert torch.allclose(o[41:101], eps.expand(60, D), rtol=1e-6, atol=0)            # in-degree 1: sqrt(eps) ...
    _, dst = blk.edges()
    assert not xd.grad.cpu()[(dst >= 41) & (dst < 101)].any()                          # ... and no gradient
    assert torch.allclose(o[101], eps.expand(D), rtol=1e-6, atol=0) and not xd.grad.cpu()[dst == 101].any()   # equal messages
    assert torch.allclose(o[102, :1], eps.view(1), rtol=1e-6, atol=0) and not xd.grad.cpu()[dst == 102, 0].any()


def _std_step(x, blk, g):
    x = x.detach().requires_grad_(True)
    out = K.aggregate_std(x, blk)
    (gx,) = torch.autograd.grad(out, x, g)
    return out, gx


def test_a_std_bitwise_reproducible():
    blk, x, g = std_block(64, 7)
    blk, x, g = blk.to(DEV), x.to(DEV), g.to(DEV)
    first, second = _std_step(x, blk, g), _std_step(x, blk, g)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_a_std_capturable():
    blk, x, g = std_block(200, 8)
    blk, x, g = blk.to(DEV), x.to(DEV).requires_grad_(True), g.to(DEV)
    eager = _std_step(x, blk, g)
    blk.plan()["n_chunks"]                                  # the plan's exact sizes on the host before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _std_step(x, blk, g)                                # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, gx = K.aggregate_std(x, blk), None
        (gx,) = torch.autograd.grad(out, x, g)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(gx, eager[1])


def test_hip_path_taken(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch reduction reached: an NC aggregator fell back to torch")

    for nm in ("index_add", "index_add_", "scatter_reduce", "scatter_reduce_"):
        monkeypatch.setattr(torch.Tensor, nm, refuse)
    monkeypatch.setattr(torch, "index_add", refuse)
    monkeypatch.setattr(torch, "scatter_reduce", refuse)
    blk, x, g = std_block(64, 9)
    blk, g = blk.to(DEV), g.to(DEV)
    want = {"a_std": ["mrg_seg_std_fwd", "mrg_seg_std_bwd"], "a_sum": ["mrg_span_gcs", "mrg_seg_reduce_bwd_ordered"],
            "a_max": ["mrg_seg_reduce_fwd", "mrg_linear_bwd_weight"], "a_mean": ["mrg_span_gcs", "mrg_linear_bwd_weight"]}
    for name, fns in want.items():
        op = ON.MIXED_OPS[name]({"feature_dim": 64}).to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        _lib.meter.start()
        try:
            op(blk, xd, xd).backward(g)
        finally:
            rec = _lib.meter.stop()
        for fn in fns:
            assert fn in rec, (name, fn, sorted(rec))
        if name == "a_std":
            assert rec["mrg_seg_std_fwd"]["launches"] == 1 and rec["mrg_seg_std_bwd"]["launches"] == 1


@pytest.mark.parametrize("case", ["ops", "n1"])
def test_device_blocks_equal_cpu_blocks(case):
    if case == "ops":
        z, prefix = load_golden("nc_ops_small"), ""
        N, seeds, layers = int(z["N"]), z["seeds"], int(z["layers"])
    else:
        z, prefix = load_golden("nc_fixednet_small"), case + "/"
        N, seeds, layers = int(z[prefix + "args"][0]), z[prefix + "seeds"], int(z[prefix + "args"][8])
    g = G.RelGraph(N, z[prefix + "gsrc"], z[prefix + "gdst"])
    g.edata[G.ETYPE] = z[prefix + "getype"].long()
    cpu = SM.full_neighbor_blocks(g, seeds, layers)
    dev = SM.full_neighbor_blocks(g.to(DEV), seeds.to(DEV), layers)
    for a, b in zip(dev, cpu):
        assert a.device.type == "cuda"
        for x, y in ((a.edges()[0], b.edges()[0]), (a.edges()[1], b.edges()[1]), (a.edata[G.EID], b.edata[G.EID]),
                     (a.edata[G.ETYPE], b.edata[G.ETYPE]), (a.srcdata[G.NID], b.srcdata[G.NID]), (a.dstdata[G.NID], b.dstdata[G.NID])):
            assert torch.equal(x.cpu(), y)


@pytest.mark.parametrize("tag", ["n0", "n1", "s1"])
def test_network_matches_the_reference(tag):
    z = load_golden("nc_fixednet_small")
    net = make_net(z, tag, DEV)
    blocks = [b.to(DEV) for b in fixture_blocks(z, tag + "/blocks/")]
    trip = z[tag + "/trip_index"].to(DEV)
    seeds = z[tag + "/seeds"].long().to(DEV)
    labels = z[tag + "/labels"].to(DEV)
    net.train()
    _lib.meter.start(["mrg_linear_fwd", "mrg_mix_fwd"])
    logits = net(trip, blocks)
    rec = _lib.meter.stop()
    assert "mrg_linear_fwd" in rec and "mrg_mix_fwd" in rec               # OpModule / concat Linear on the row GEMM, BN + ReLU on the epilogue
    loss = net._criterion(logits, labels[seeds])
    loss.backward()
    close(logits, z[tag + "/logits"], f"{tag} logits", rtol=2e-4, atol=5e-5)
    close(loss.reshape(1), z[tag + "/loss"].reshape(1), f"{tag} loss")
    grads_close(net, z, tag, 2e-3)
    for n, b in net.named_buffers():
        if "running_" in n:
            torch.testing.assert_close(b.cpu(), z[f"{tag}/buffer/{n}"], rtol=1e-4, atol=1e-5, msg=lambda m: f"{tag} {n}: {m}")
    net.eval()
    with torch.no_grad():
        close(net(trip, blocks), z[tag + "/logits_eval"], f"{tag} eval logits", rtol=2e-4, atol=5e-5)
        eval_loss = net._loss(trip, blocks, labels, seeds)
    ref_eval = torch.nn.functional.cross_entropy(z[tag + "/logits_eval"], z[tag + "/labels"][z[tag + "/seeds"].long()])
    close(eval_loss.reshape(1), ref_eval.reshape(1), f"{tag} eval _loss")
