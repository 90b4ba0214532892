"""sampler.NeighborSampler on the MI355X (csrc/blocks.hip): the HIP blocks against the CPU formulation for the same uniforms (the hub
copied whole and cut to k, d == k, d == k + 1, destinations without in-edges, two layers), the scratch tables after every call, the
launch census, the full fan-out against full_neighbor_blocks on the device, and the consumers (model_nc.Network and a_mean) on
sampled blocks."""
import pytest
import torch

from conftest import load_golden
from test_nc_cpu import assert_blocks_equal, close, grads_close, make_net
from test_neighbor_sampler_cpu import FANOUTS, check_block_properties, degree_64_65_graph, fixture_graph

from mr_gnas_amd import _lib, sampler as SM
from mr_gnas_amd import operations_nc as ON

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32_MAX = 2 ** 31 - 1


def tables_at_rest(sampler):
    return bool((sampler.local == -1).all()) and bool((sampler.firstpos == I32_MAX).all())


def cpu_draws(blocks):
    return [None if b.draws is None else b.draws.cpu() for b in blocks]


@pytest.mark.parametrize("fanouts", FANOUTS + [[None], [None, None], [64, 64]], ids=str)
def test_hip_blocks_equal_the_cpu_formulation(fanouts):
    g, seeds, _ = fixture_graph("ops")
    sampler = SM.NeighborSampler(g.to(DEV), fanouts)
    gen = torch.Generator(device=DEV).manual_seed(21)
    blocks = sampler.sample(seeds.to(DEV), generator=gen)
    assert tables_at_rest(sampler)
    for b, k in zip(blocks, fanouts):
        assert b.device.type == "cuda"
        assert (b.draws is None) if k is None else (b.draws.is_cuda and tuple(b.draws.shape) == (b.number_of_dst_nodes(), k))
    ref = SM.NeighborSampler(g, fanouts).sample(seeds, draws=cpu_draws(blocks))
    assert_blocks_equal(blocks, ref)
    for b, k in zip(ref, fanouts):
        check_block_properties(g, b, k)
    # replay on the device from the same uniforms; the same generator state gives the same blocks
    assert_blocks_equal(sampler.sample(seeds.to(DEV), draws=[b.draws for b in blocks]), ref)
    assert_blocks_equal(sampler.sample(seeds.to(DEV), generator=torch.Generator(device=DEV).manual_seed(21)), ref)
    assert tables_at_rest(sampler)


def test_in_degree_64_and_65_on_the_device():
    g, seeds = degree_64_65_graph()
    sampler = SM.NeighborSampler(g.to(DEV), [64])
    (b,) = sampler.sample(seeds.to(DEV))
    assert torch.bincount(b.edges()[1]).tolist() == [64, 64]
    assert_blocks_equal([b], SM.NeighborSampler(g, [64]).sample(seeds, draws=[b.draws.cpu()]))
    assert tables_at_rest(sampler)


def test_a_second_seed_set_equals_a_fresh_sampler():
    """A missed restore of the scratch tables would leak the first call's nodes into the second."""
    g, seeds, _ = fixture_graph("ops")
    gd = g.to(DEV)
    sampler = SM.NeighborSampler(gd, [3, 2])
    sampler.sample(seeds.to(DEV))
    assert tables_at_rest(sampler)
    other = torch.tensor([29, 3, 0, 77, 41, 6, 100, 12], device=DEV)
    second = sampler.sample(other)
    assert tables_at_rest(sampler)
    fresh = SM.NeighborSampler(gd, [3, 2]).sample(other, draws=[b.draws for b in second])
    assert_blocks_equal(second, fresh)
    assert_blocks_equal(second, SM.NeighborSampler(g, [3, 2]).sample(other.cpu(), draws=cpu_draws(second)))
    # seeds without a single in-edge: an empty block, nothing launched, the tables untouched
    (empty,) = SM.NeighborSampler(gd, [4]).sample(torch.tensor([26, 27, 28, 29], device=DEV))
    assert empty.num_edges() == 0 and empty.number_of_src_nodes() == 4


def test_launch_census():
    g, seeds, _ = fixture_graph("ops")
    sampler = SM.NeighborSampler(g.to(DEV), [2, 3])
    seeds = seeds.to(DEV)
    sampler.sample(seeds)
    _lib.meter.start()
    try:
        sampler.sample(seeds)
    finally:
        rec = _lib.meter.stop()
    assert {n: r["launches"] for n, r in rec.items()} == {"mrg_block_sizes": 2, "mrg_block_emit": 2, "mrg_block_relabel": 2}, rec


@pytest.mark.parametrize("case", ["ops", "n1"])
def test_full_fanout_equals_full_neighbor_blocks_on_the_device(case):
    g, seeds, layers = fixture_graph(case)
    gd, sd = g.to(DEV), seeds.to(DEV)
    for n in sorted({layers, 2}):
        blocks = SM.NeighborSampler(gd, [None] * n).sample(sd)
        assert_blocks_equal(blocks, SM.full_neighbor_blocks(gd, sd, n))
        assert all(b.device.type == "cuda" for b in blocks)


def test_a_mean_divides_by_the_sampled_in_degree():
    g, seeds, _ = fixture_graph("ops")
    (blk,) = SM.NeighborSampler(g.to(DEV), [2]).sample(seeds.to(DEV))
    D, E, n = 16, blk.num_edges(), blk.number_of_dst_nodes()
    op = ON.a_mean_op({"feature_dim": D})
    with torch.no_grad():
        op.linear.weight.copy_(torch.eye(D))
        op.linear.bias.zero_()
    x = torch.rand(E, D, generator=torch.Generator().manual_seed(2)) + 0.5        # positive: the ReLU is the identity
    out = op.to(DEV)(blk, x.to(DEV), x.to(DEV)).cpu()
    ldst = blk.edges()[1].cpu()
    cnt = torch.bincount(ldst, minlength=n)
    assert int(cnt[0]) == 2 and int(cnt.max()) == 2                                # the hub's 2 048 in-edges cut to 2
    want = torch.zeros(n, D, dtype=torch.float64).index_add_(0, ldst, x.double()) / cnt.clamp(min=1).view(-1, 1)
    torch.testing.assert_close(out.double(), want, rtol=1e-5, atol=1e-6)


def test_network_on_sampled_blocks_matches_the_cpu_path():
    z = load_golden("nc_fixednet_small")
    tag = "n1"
    g, seeds, _ = fixture_graph(tag)
    blocks = SM.NeighborSampler(g.to(DEV), [2, 2]).sample(seeds.to(DEV), generator=torch.Generator(device=DEV).manual_seed(4))
    out = {}
    for dev in ("cpu", DEV):
        net = make_net(z, tag, dev)
        net.train()
        blk = [b.to(dev) for b in blocks]
        logits = net(z[tag + "/trip_index"].to(dev), blk)
        loss = net._criterion(logits, z[tag + "/labels"].to(dev)[seeds.to(dev)])
        loss.backward()
        out[dev] = (net, logits, loss)
    ref_net, ref_logits, ref_loss = out["cpu"]
    net, logits, loss = out[DEV]
    close(logits, ref_logits, "logits", rtol=2e-4, atol=5e-5)
    close(loss.reshape(1), ref_loss.reshape(1), "loss")
    ref = {f"{tag}/gparam/{n}": p.grad for n, p in ref_net.named_parameters() if p.grad is not None}
    assert len(ref) > 4
    grads_close(net, ref, tag, 2e-3)
