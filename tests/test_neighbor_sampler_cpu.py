"""sampler.NeighborSampler on CPU tensors (no GPU): the torch formulation against full_neighbor_blocks (all fan-outs None) and against
an explicit Python loop with Floyd's pick from the block's own uniforms; the properties of a sampled block; determinism and
replay; the uniformity of the pick (a property of the algorithm: tested here once); argument errors; and the host side of the
C ABI of csrc/blocks.hip (argument validation happens before any launch)."""
import ctypes
import math

import pytest
import torch

from conftest import load_golden
from test_nc_cpu import assert_blocks_equal

from mr_gnas_amd import _lib, graph as G, sampler as SM

FANOUTS = [[1], [2], [4], [5], [64], [2, 3], [None, 2]]
NEW = ("mrg_block_sizes", "mrg_block_emit", "mrg_block_relabel", "mrg_block_sizes_workspace_bytes", "mrg_block_relabel_workspace_bytes")


def fixture_graph(case):
    """(graph, seeds, layers) of nc_ops_small ('ops': a hub of 2 048 in-edges, in-degrees 1..5, one of exactly 4, duplicated edges,
    seeds without in-edges) or of a network of nc_fixednet_small."""
    if case == "ops":
        z, prefix = load_golden("nc_ops_small"), ""
        N, seeds, layers = int(z["N"]), z["seeds"], int(z["layers"])
    else:
        z, prefix = load_golden("nc_fixednet_small"), case + "/"
        N, seeds, layers = int(z[prefix + "args"][0]), z[prefix + "seeds"], int(z[prefix + "args"][8])
    g = G.RelGraph(N, z[prefix + "gsrc"], z[prefix + "gdst"])
    g.edata[G.ETYPE] = z[prefix + "getype"].long()
    return g, seeds.long(), layers


def floyd(d, k, u):
    """The ascending k-subset of 0..d-1 that Floyd's algorithm picks from the uniforms u[0..k-1]."""
    picked = []
    for i in range(k):
        j = d - k + i
        t = min(int(math.floor(float(u[i]) * (j + 1))), j)
        picked.append(j if t in picked else t)
    return sorted(picked)


def loop_blocks(g, seeds, fanouts, draws):
    """Explicit loops over the conventions of full_neighbor_blocks (tests/golden/make_golden_nc.py), with the fan-out applied."""
    src, dst = (t.tolist() for t in g.edges())
    etype = g.edata[G.ETYPE]
    in_list = {}
    for e, v in enumerate(dst):                                          # ascending edge ids inside every list
        in_list.setdefault(v, []).append(e)
    blocks = []
    dst_nodes = [int(v) for v in seeds]
    for j in reversed(range(len(fanouts))):
        k, eids, ldst = fanouts[j], [], []
        for i, v in enumerate(dst_nodes):
            lst = in_list.get(v, [])
            if k is not None and len(lst) > k:
                lst = [lst[p] for p in floyd(len(lst), k, draws[j][i])]
            eids += lst
            ldst += [i] * len(lst)
        local = {v: i for i, v in enumerate(dst_nodes)}
        src_nodes = list(dst_nodes)
        for e in eids:
            if src[e] not in local:
                local[src[e]] = len(src_nodes)
                src_nodes.append(src[e])
        t = lambda a: torch.tensor(a, dtype=torch.long)
        blocks.append(G.Block(t(src_nodes), t(dst_nodes), t([local[src[e]] for e in eids]), t(ldst), t(eids), etype[t(eids)]))
        dst_nodes = src_nodes
    return blocks[::-1]


def check_block_properties(g, blk, k):
    """Each destination has min(d, k) distinct in-edges of its own, edge ids ascending; local indices and types lead back to the graph."""
    gsrc, gdst = g.edges()
    lsrc, ldst = blk.edges()
    eid = blk.edata[G.EID]
    assert torch.equal(blk.srcdata[G.NID][lsrc], gsrc[eid]) and torch.equal(blk.dstdata[G.NID][ldst], gdst[eid])
    assert torch.equal(blk.edata[G.ETYPE], g.edata[G.ETYPE][eid])
    assert bool((ldst[1:] >= ldst[:-1]).all())                           # grouped by destination, in destination order
    same = ldst[1:] == ldst[:-1]
    assert bool((eid[1:][same] > eid[:-1][same]).all())                  # ascending (so distinct) inside a destination
    deg = torch.bincount(gdst, minlength=g.number_of_nodes())[blk.dstdata[G.NID]]
    want = deg if k is None else deg.clamp(max=k)
    assert torch.equal(torch.bincount(ldst, minlength=blk.number_of_dst_nodes()), want)
    n_dst = blk.number_of_dst_nodes()
    assert torch.equal(blk.srcdata[G.NID][:n_dst], blk.dstdata[G.NID])
    assert blk.srcdata[G.NID].unique().numel() == blk.number_of_src_nodes()


@pytest.mark.parametrize("case", ["ops", "n0", "n1"])
def test_full_fanout_equals_full_neighbor_blocks(case):
    g, seeds, layers = fixture_graph(case)
    for layers in {layers, 2}:
        blocks = SM.NeighborSampler(g, [None] * layers).sample(seeds)
        assert_blocks_equal(blocks, SM.full_neighbor_blocks(g, seeds, layers))
        assert all(b.draws is None for b in blocks)
    assert_blocks_equal(SM.NeighborSampler(g, [-1]).sample(seeds), SM.full_neighbor_blocks(g, seeds, 1))


@pytest.mark.parametrize("fanouts", FANOUTS, ids=str)
def test_sampled_blocks_match_the_loop(fanouts):
    g, seeds, _ = fixture_graph("ops")
    sampler = SM.NeighborSampler(g, fanouts)
    blocks = sampler.sample(seeds, generator=torch.Generator().manual_seed(11))
    for j, (b, k) in enumerate(zip(blocks, fanouts)):
        if k is None:
            assert b.draws is None
        else:
            assert b.draws.dtype == torch.float64 and tuple(b.draws.shape) == (b.number_of_dst_nodes(), k)
        check_block_properties(g, b, k)
    for j in range(len(blocks) - 1):
        assert torch.equal(blocks[j].dstdata[G.NID], blocks[j + 1].srcdata[G.NID])
    assert torch.equal(blocks[-1].dstdata[G.NID], seeds)
    assert_blocks_equal(blocks, loop_blocks(g, seeds, fanouts, [b.draws for b in blocks]))
    assert bool((sampler.local == -1).all()) and bool((sampler.firstpos == 2 ** 31 - 1).all())
    if fanouts[-1] is not None:                                          # the hub (seed 0, 2 048 in-edges) is cut to the fan-out
        assert int((blocks[-1].edges()[1] == 0).sum()) == fanouts[-1]


def degree_64_65_graph():
    """Node 0 with 64 in-edges, node 1 with 65, the edge list shuffled; seeds (1, 0)."""
    gen = torch.Generator().manual_seed(3)
    dst = torch.cat((torch.zeros(64, dtype=torch.long), torch.ones(65, dtype=torch.long)))
    perm = torch.randperm(129, generator=gen)
    g = G.RelGraph(40, torch.randint(2, 40, (129,), generator=gen)[perm], dst[perm])
    g.edata[G.ETYPE] = torch.randint(0, 3, (129,), generator=gen)
    return g, torch.tensor([1, 0])


def test_in_degree_64_and_65_at_the_largest_fanout():
    g, seeds = degree_64_65_graph()
    (b,) = SM.NeighborSampler(g, [64]).sample(seeds, generator=torch.Generator().manual_seed(8))
    assert torch.bincount(b.edges()[1]).tolist() == [64, 64]            # 65 in-edges: exactly one dropped; 64: all kept
    check_block_properties(g, b, 64)
    assert_blocks_equal([b], loop_blocks(g, seeds, [64], [b.draws]))


def test_determinism_and_replay():
    g, seeds, _ = fixture_graph("ops")
    sampler = SM.NeighborSampler(g, [2, 3])
    first = sampler.sample(seeds, generator=torch.Generator().manual_seed(5))
    again = sampler.sample(seeds, generator=torch.Generator().manual_seed(5))
    assert_blocks_equal(again, first)
    assert all(torch.equal(a.draws, b.draws) for a, b in zip(again, first))
    replay = SM.NeighborSampler(g, [2, 3]).sample(seeds, draws=[b.draws for b in first])
    assert_blocks_equal(replay, first)
    other = sampler.sample(seeds, generator=torch.Generator().manual_seed(6))
    hub = lambda blocks: blocks[-1].edata[G.EID][blocks[-1].edges()[1] == 0]
    assert hub(other).numel() == 3 and not torch.equal(hub(other), hub(first))


def test_the_pick_is_uniform():
    """4 096 destinations of in-degree 5 at k = 2: Pearson's chi-square of the 10 position pairs against 409.6 each stays below the
    0.999 quantile at 9 degrees of freedom (27.88).  A correct implementation gives 11.51 for this seed."""
    n = 4096
    dst = torch.arange(n).repeat_interleave(5)                          # edge 5 v + p is position p of destination v
    g = G.RelGraph(n + 7, n + torch.arange(5 * n) % 7, dst)
    (b,) = SM.NeighborSampler(g, [2]).sample(torch.arange(n), generator=torch.Generator().manual_seed(0))
    pos = (b.edata[G.EID] - 5 * b.edges()[1]).view(n, 2)
    assert bool((pos[:, 0] < pos[:, 1]).all()) and int(pos.min()) == 0 and int(pos.max()) == 4
    counts = torch.bincount(pos[:, 0] * 5 + pos[:, 1], minlength=25).double()
    counts = counts[counts > 0]
    assert counts.numel() == 10
    chi2 = float(((counts - n / 10) ** 2 / (n / 10)).sum())
    print(f"chi-square {chi2:.2f}")
    assert chi2 < 27.88, chi2


@pytest.mark.parametrize("bad", [0, 65, -2, 2.0])
def test_bad_fanouts_raise(bad):
    g, _, _ = fixture_graph("ops")
    with pytest.raises(ValueError, match="64"):
        SM.NeighborSampler(g, [None, bad])


def test_bad_draws_raise():
    g, seeds, _ = fixture_graph("ops")
    sampler = SM.NeighborSampler(g, [None, 2])
    n = int(seeds.numel())
    with pytest.raises(ValueError):
        sampler.sample(seeds, draws=[None, torch.zeros(n, 3, dtype=torch.float64)])
    with pytest.raises(ValueError):
        sampler.sample(seeds, draws=[None, torch.zeros(n + 1, 2, dtype=torch.float64)])
    with pytest.raises(ValueError):
        sampler.sample(seeds, draws=[None, torch.zeros(n, 2)])                      # float32
    with pytest.raises(ValueError):
        sampler.sample(seeds, draws=[torch.zeros(n, 2, dtype=torch.float64)])       # one entry for two layers
    with pytest.raises(ValueError):
        sampler.sample(seeds, draws=[torch.zeros(1, 1, dtype=torch.float64), torch.zeros(n, 2, dtype=torch.float64)])
    assert bool((sampler.local == -1).all()) and bool((sampler.firstpos == 2 ** 31 - 1).all())


# ---- the host side of the C ABI ----------------------------------------------------------------------------------------------------
def test_the_library_declares_the_entry_points_at_abi_22():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 23 and lib.mrg_abi_version() == 23
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(256)                                             # never dereferenced: every call below returns before a launch
    sizes = lambda rowptr=p, dst=p, n=8, N=100, k=4, first=p, ws=p, nb=1 << 30: lib.mrg_block_sizes(rowptr, dst, n, N, k, first, ws, nb, None)
    emit = lambda rowptr=p, ie=p, isrc=p, it=p, dst=p, first=p, n=8, N=100, k=4, u=p, E=16, eid=p, et=p, ldst=p, gs=p, loc=p, fp=p: \
        lib.mrg_block_emit(rowptr, ie, isrc, it, dst, first, n, N, k, u, E, eid, et, ldst, gs, loc, fp, None)
    relabel = lambda gs=p, dst=p, n=8, N=100, E=16, loc=p, fp=p, sn=p, ls=p, nn=p, ws=p, nb=1 << 30: \
        lib.mrg_block_relabel(gs, dst, n, N, E, loc, fp, sn, ls, nn, ws, nb, None)
    # NULL pointers -> MRG_E_NULLPTR
    for kw in ("rowptr", "dst", "first"):
        assert sizes(**{kw: None}) == -1, kw
    for kw in ("rowptr", "ie", "isrc", "dst", "first", "u", "eid", "ldst", "gs", "loc", "fp"):
        assert emit(**{kw: None}) == -1, kw
    assert emit(it=None) == -1                                           # types asked for without the index's types
    for kw in ("gs", "dst", "loc", "fp", "sn", "ls", "nn"):
        assert relabel(**{kw: None}) == -1, kw
    # negative sizes, k outside 0..64 -> MRG_E_SHAPE
    for k in (-1, 65, 1000):
        assert sizes(k=k) == -2 and emit(k=k) == -2
    assert sizes(n=-1) == -2 and sizes(N=-1) == -2 and emit(n=-1) == -2 and emit(E=-1) == -2 and emit(N=-1) == -2
    assert relabel(n=-1) == -2 and relabel(E=-1) == -2 and relabel(N=-1) == -2
    assert emit(E=2 ** 31) == -2 and relabel(E=2 ** 31 - 9, n=16) == -2
    # a missing or short workspace -> MRG_E_WORKSPACE
    assert sizes(ws=None) == -4 and relabel(ws=None) == -4
    assert lib.mrg_block_sizes_workspace_bytes(8) > 0 and lib.mrg_block_relabel_workspace_bytes(16) >= 16 * 4
    assert sizes(nb=lib.mrg_block_sizes_workspace_bytes(8) - 1) == -4
    assert relabel(nb=lib.mrg_block_relabel_workspace_bytes(16) - 1) == -4
    # nothing to do -> MRG_OK, nothing launched (NULL pointers are then fine)
    assert sizes(n=0, rowptr=None, ws=None) == 0
    assert emit(n=0, rowptr=None) == 0 and emit(E=0, eid=None) == 0
    assert relabel(n=0, gs=None, ws=None) == 0 and relabel(E=0, gs=None, ws=None) == 0
    # the queries are host functions of the size
    assert lib.mrg_block_sizes_workspace_bytes(-1) == 0 and lib.mrg_block_relabel_workspace_bytes(-1) == 0
