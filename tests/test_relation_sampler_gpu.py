"""sampler.NeighborSampler with per-relation fan-outs on the MI355X (csrc/blocks_rel.hip): the HIP blocks against the CPU formulation
for the same uniforms (the hub's runs copied whole, cut and dropped; a destination with more runs than a wave has lanes; runs of 64
and 65 at f = 64; mixed layers), replay, the scratch tables after every call, a second seed set, the one-type graph against the
integer fan-out's kernels, the launch census, and model_nc.Network on per-relation blocks."""
import pytest
import torch

from conftest import load_golden
from test_nc_cpu import assert_blocks_equal, close, grads_close, make_net
from test_neighbor_sampler_cpu import fixture_graph
from test_neighbor_sampler_gpu import cpu_draws, tables_at_rest
from test_relation_sampler_cpu import MIXED, OPS_SPECS, as_list, check_rel_block, runs_graph

from mr_gnas_amd import _lib, graph as G, sampler as SM

pytestmark = pytest.mark.gpu
DEV = "cuda"


def hip_against_cpu(g, seeds, layers, R, **kw):
    sampler = SM.NeighborSampler(g.to(DEV), layers, **kw)
    blocks = sampler.sample(seeds.to(DEV), generator=torch.Generator(device=DEV).manual_seed(21))
    assert tables_at_rest(sampler)
    assert all(b.device.type == "cuda" and (b.draws is None or b.draws.is_cuda) for b in blocks)
    ref = SM.NeighborSampler(g, layers, **kw).sample(seeds, draws=cpu_draws(blocks))
    assert_blocks_equal(blocks, ref)
    for b, spec in zip(ref, layers):
        if isinstance(as_list(spec), list):
            check_rel_block(g, b, spec, R)
    # replay on the device from the same uniforms; the same generator state gives the same blocks
    assert_blocks_equal(sampler.sample(seeds.to(DEV), draws=[b.draws for b in blocks]), ref)
    assert tables_at_rest(sampler)
    assert_blocks_equal(sampler.sample(seeds.to(DEV), generator=torch.Generator(device=DEV).manual_seed(21)), ref)
    assert tables_at_rest(sampler)
    return blocks


@pytest.mark.parametrize("layers", OPS_SPECS, ids=str)
def test_hip_blocks_equal_the_cpu_formulation(layers):
    g, seeds, _ = fixture_graph("ops")
    hip_against_cpu(g, seeds, layers, 7)


def test_runs_graph_on_the_device():
    g, seeds, spec, R = runs_graph()
    (b,) = hip_against_cpu(g, seeds, [spec], R, num_etypes=R)
    ldst, et = b.edges()[1], b.edata[G.ETYPE]
    assert torch.bincount(ldst * R + et, minlength=4 * R).view(4, R)[0, 70:72].tolist() == [64, 64]
    assert torch.bincount(ldst, minlength=4).tolist()[2:] == [0, 0]
    hip_against_cpu(g, seeds, [dict(enumerate(spec)), spec], R, num_etypes=R)


def test_a_second_seed_set_equals_a_fresh_sampler():
    """A missed restore of the scratch tables would leak the first call's nodes into the second."""
    g, seeds, _ = fixture_graph("ops")
    gd = g.to(DEV)
    layers = [[2] * 7, MIXED]
    sampler = SM.NeighborSampler(gd, layers)
    sampler.sample(seeds.to(DEV))
    assert tables_at_rest(sampler)
    other = torch.tensor([29, 3, 0, 77, 41, 6, 100, 12], device=DEV)
    second = sampler.sample(other)
    assert tables_at_rest(sampler)
    assert_blocks_equal(second, SM.NeighborSampler(gd, layers).sample(other, draws=[b.draws for b in second]))
    assert_blocks_equal(second, SM.NeighborSampler(g, layers).sample(other.cpu(), draws=cpu_draws(second)))
    # seeds that keep no in-edge: an empty block, nothing launched after the sizes step, the tables untouched
    lonely = torch.tensor([26, 27, 28, 29], device=DEV)
    for spec, who in (([1] * 7, lonely), ([0] * 7, seeds.to(DEV))):
        one = SM.NeighborSampler(gd, [spec])
        _lib.meter.start()
        try:
            (empty,) = one.sample(who)
        finally:
            rec = _lib.meter.stop()
        assert empty.num_edges() == 0 and empty.number_of_src_nodes() == int(who.numel())
        assert {n: r["launches"] for n, r in rec.items()} == {"mrg_block_rel_sizes": 1}, rec
        assert tables_at_rest(one)


@pytest.mark.parametrize("k", [1, 3, 64])
def test_one_type_graph_equals_the_integer_fanout_on_the_device(k):
    """Ties the per-relation kernels to the shipped ones: with one edge type a run is the whole in-list."""
    g, seeds, _ = fixture_graph("ops")
    g1 = G.RelGraph(g.number_of_nodes(), *g.edges())
    g1.edata[G.ETYPE] = torch.zeros_like(g.edata[G.ETYPE])
    gd = g1.to(DEV)
    rel_sampler = SM.NeighborSampler(gd, [[k], {0: k}])
    rel = rel_sampler.sample(seeds.to(DEV), generator=torch.Generator(device=DEV).manual_seed(2))
    assert_blocks_equal(rel, SM.NeighborSampler(gd, [k, k]).sample(seeds.to(DEV), draws=[b.draws for b in rel]))
    assert tables_at_rest(rel_sampler)


def census(sampler, seeds):
    sampler.sample(seeds)
    _lib.meter.start()
    try:
        sampler.sample(seeds)
    finally:
        rec = _lib.meter.stop()
    return {n: r["launches"] for n, r in rec.items()}


def test_launch_census():
    g, seeds, _ = fixture_graph("ops")
    gd, sd = g.to(DEV), seeds.to(DEV)
    assert census(SM.NeighborSampler(gd, [MIXED, [1] * 7]), sd) == {"mrg_block_rel_sizes": 2, "mrg_block_rel_emit": 2, "mrg_block_relabel": 2}
    assert census(SM.NeighborSampler(gd, [2], per_relation=True), sd) == {"mrg_block_rel_sizes": 1, "mrg_block_rel_emit": 1, "mrg_block_relabel": 1}
    # the integer layers keep their entry points, next to a per-relation layer and alone
    assert census(SM.NeighborSampler(gd, [2, MIXED, None]), sd) == {"mrg_block_sizes": 2, "mrg_block_emit": 2, "mrg_block_rel_sizes": 1,
                                                                    "mrg_block_rel_emit": 1, "mrg_block_relabel": 3}
    assert census(SM.NeighborSampler(gd, [2, 3]), sd) == {"mrg_block_sizes": 2, "mrg_block_emit": 2, "mrg_block_relabel": 2}
    assert census(SM.NeighborSampler(gd, [2, 3], num_etypes=7), sd) == {"mrg_block_sizes": 2, "mrg_block_emit": 2, "mrg_block_relabel": 2}


def test_network_on_per_relation_blocks_matches_the_cpu_path():
    z = load_golden("nc_fixednet_small")
    tag = "n1"
    g, seeds, _ = fixture_graph(tag)
    R = int(g.edata[G.ETYPE].max()) + 1
    blocks = SM.NeighborSampler(g.to(DEV), [[2] * R, [2] * R]).sample(seeds.to(DEV), generator=torch.Generator(device=DEV).manual_seed(4))
    full = SM.full_neighbor_blocks(g, seeds, 2)
    assert 0 < blocks[-1].num_edges() < full[-1].num_edges()            # some run of the seeds is cut
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
