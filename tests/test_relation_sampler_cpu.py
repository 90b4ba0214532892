"""sampler.NeighborSampler with per-relation fan-outs on CPU tensors (no GPU): the torch formulation against an explicit Python loop
(runs per destination from the edge list, Floyd's pick per run from the run's columns of the block's uniforms, a merge by edge id,
the relabelling); its equivalences with full_neighbor_blocks and with the integer fan-outs; a constructed graph with more runs on a
destination than a wave has lanes, runs of 64 and 65 at f = 64, and edge ids that interleave the types; per-type counts;
determinism, replay and the scratch tables; the uniformity of the picks (tested once); argument errors; and the host side of the
C ABI of csrc/blocks_rel.hip (argument validation happens before any launch)."""
import ctypes

import pytest
import torch

from test_nc_cpu import assert_blocks_equal
from test_neighbor_sampler_cpu import check_block_properties, fixture_graph, floyd

from mr_gnas_amd import _lib, graph as G, sampler as SM

MIXED = [2, 0, None, 64, 1, 5, 3]
OPS_SPECS = [[[1] * 7], [[None] * 7], [[0] * 7], [MIXED], [dict(enumerate(MIXED))], [3, MIXED], [MIXED, None], [[1] * 7, MIXED]]
NEW = ("mrg_block_rel_sizes", "mrg_block_rel_emit", "mrg_block_rel_sizes_workspace_bytes", "mrg_block_rel_emit_workspace_bytes")
I32_MAX = 2 ** 31 - 1


def as_list(spec):
    """A layer entry as the loop reads it: None, an integer, or the list of the per-type entries (None = every in-edge)."""
    if isinstance(spec, dict):
        spec = [spec[r] for r in range(len(spec))]
    if isinstance(spec, (list, tuple)):
        return [None if f in (None, -1) else int(f) for f in spec]
    return spec


def kept(d, f):
    return d if f is None or d <= f else f


def loop_blocks(g, seeds, layers, draws):
    """Explicit loops: the conventions of full_neighbor_blocks with every layer's fan-out applied, per run where it is per-relation."""
    src, dst = (t.tolist() for t in g.edges())
    etype = g.edata[G.ETYPE]
    types = etype.tolist()
    in_list = {}
    for e, v in enumerate(dst):                                          # ascending edge ids inside every list
        in_list.setdefault(v, []).append(e)
    blocks = []
    dst_nodes = [int(v) for v in seeds]
    for j in reversed(range(len(layers))):
        spec, eids, ldst = as_list(layers[j]), [], []
        for i, v in enumerate(dst_nodes):
            lst = in_list.get(v, [])
            if isinstance(spec, list):
                merged, off = [], 0
                for r, f in enumerate(spec):
                    run = [e for e in lst if types[e] == r]              # the run (v, r), ascending edge ids
                    if f == 0:
                        run = []
                    elif f is not None and len(run) > f:
                        run = [run[p] for p in floyd(len(run), f, draws[j][i][off:off + f])]
                    off += f or 0
                    merged += run
                lst = sorted(merged)                                     # across the types
            elif spec is not None and len(lst) > spec:
                lst = [lst[p] for p in floyd(len(lst), spec, draws[j][i])]
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


def tables_at_rest(sampler):
    return bool((sampler.local == -1).all()) and bool((sampler.firstpos == I32_MAX).all())


def check_rel_block(g, blk, spec, R):
    """The block leads back to the graph, is grouped by destination with ascending edge ids inside one, and keeps kept(d_vr, f_r)
    edges of every run."""
    spec = as_list(spec)
    gsrc, gdst = g.edges()
    lsrc, ldst = blk.edges()
    eid, n_dst = blk.edata[G.EID], blk.number_of_dst_nodes()
    assert torch.equal(blk.srcdata[G.NID][lsrc], gsrc[eid]) and torch.equal(blk.dstdata[G.NID][ldst], gdst[eid])
    assert torch.equal(blk.edata[G.ETYPE], g.edata[G.ETYPE][eid])
    assert bool((ldst[1:] >= ldst[:-1]).all())                           # grouped by destination, in destination order
    same = ldst[1:] == ldst[:-1]
    assert bool((eid[1:][same] > eid[:-1][same]).all())                  # ascending (so distinct) inside a destination, across types
    d = torch.bincount(gdst * R + g.edata[G.ETYPE], minlength=g.number_of_nodes() * R).view(-1, R)[blk.dstdata[G.NID]]
    want = torch.stack([d[:, r] if f is None else d[:, r].clamp(max=f) for r, f in enumerate(spec)], dim=1)
    assert torch.equal(torch.bincount(ldst * R + blk.edata[G.ETYPE], minlength=n_dst * R).view(n_dst, R), want)
    assert torch.equal(blk.srcdata[G.NID][:n_dst], blk.dstdata[G.NID])
    assert blk.srcdata[G.NID].unique().numel() == blk.number_of_src_nodes()


def runs_graph():
    """(graph, seeds, specification, R) with a shuffled edge list, so that edge ids interleave the types.  Node 0: 70 distinct types
    (0..69), run lengths cycling 1..5.  Node 1: a run of exactly 64 (type 70) and one of 65 (type 71), both at f = 64.  Node 2: every
    in-edge has type 72, whose f is 0.  Node 3: no in-edges.  Type 73 occurs nowhere.  Sources are the nodes 4..39."""
    gen = torch.Generator().manual_seed(17)
    dst, typ = [], []
    for r in range(70):
        dst += [0] * (1 + r % 5)
        typ += [r] * (1 + r % 5)
    dst += [1] * 129 + [2] * 5
    typ += [70] * 64 + [71] * 65 + [72] * 5
    dst, typ = torch.tensor(dst), torch.tensor(typ)
    perm = torch.randperm(int(dst.numel()), generator=gen)
    g = G.RelGraph(40, torch.randint(4, 40, (int(dst.numel()),), generator=gen), dst[perm])
    g.edata[G.ETYPE] = typ[perm]
    spec = [(1, 2, None, 4, 3, 0, 2)[r % 7] for r in range(70)] + [64, 64, 0, 5]
    return g, torch.tensor([1, 0, 3, 2]), spec, 74


def check_layers(g, seeds, layers, R, blocks, sampler):
    for j, (b, spec) in enumerate(zip(blocks, layers)):
        spec = as_list(spec)
        width = sum(f or 0 for f in spec) if isinstance(spec, list) else (spec or 0)
        if width == 0:
            assert b.draws is None
        else:
            assert b.draws.dtype == torch.float64 and tuple(b.draws.shape) == (b.number_of_dst_nodes(), width)
        if isinstance(spec, list):
            check_rel_block(g, b, spec, R)
        else:
            check_block_properties(g, b, spec)
    for j in range(len(blocks) - 1):
        assert torch.equal(blocks[j].dstdata[G.NID], blocks[j + 1].srcdata[G.NID])
    assert torch.equal(blocks[-1].dstdata[G.NID], seeds)
    assert_blocks_equal(blocks, loop_blocks(g, seeds, layers, [b.draws for b in blocks]))
    assert tables_at_rest(sampler)


@pytest.mark.parametrize("layers", OPS_SPECS, ids=str)
def test_per_relation_blocks_match_the_loop(layers):
    g, seeds, _ = fixture_graph("ops")
    assert int(g.edata[G.ETYPE].max()) == 6                              # 7 types
    sampler = SM.NeighborSampler(g, layers)
    blocks = sampler.sample(seeds, generator=torch.Generator().manual_seed(11))
    check_layers(g, seeds, layers, 7, blocks, sampler)
    last = as_list(layers[-1])
    if isinstance(last, list):                                           # the hub (seed 0): 2 048 in-edges over all 7 types
        hub_types = g.edata[G.ETYPE][g.edges()[1] == 0]
        d = torch.bincount(hub_types, minlength=7).tolist()
        assert min(d) > 64
        assert int((blocks[-1].edges()[1] == 0).sum()) == sum(kept(d[r], f) for r, f in enumerate(last))


def test_all_none_gives_the_full_blocks():
    g, seeds, _ = fixture_graph("ops")
    for layers in ([[None] * 7], [[-1] * 7, None], [{r: None for r in range(7)}, [None] * 7]):
        blocks = SM.NeighborSampler(g, layers).sample(seeds)
        assert_blocks_equal(blocks, SM.full_neighbor_blocks(g, seeds, len(layers)))
        assert all(b.draws is None for b in blocks)


@pytest.mark.parametrize("case", ["n0", "n1"])
def test_entries_as_large_as_the_longest_run_give_the_full_blocks(case):
    g, seeds, _ = fixture_graph(case)
    R = int(g.edata[G.ETYPE].max()) + 1
    longest = int(torch.bincount(g.edges()[1] * R + g.edata[G.ETYPE]).max())
    assert 1 < longest <= 64
    blocks = SM.NeighborSampler(g, [[longest] * R, [64] * R]).sample(seeds)
    assert_blocks_equal(blocks, SM.full_neighbor_blocks(g, seeds, 2))
    assert tuple(blocks[0].draws.shape)[1] == longest * R                # drawn and ignored: the stream depends on shapes only


@pytest.mark.parametrize("k", [1, 3, 64])
def test_one_type_graph_equals_the_integer_fanout(k):
    g, seeds, _ = fixture_graph("ops")
    g1 = G.RelGraph(g.number_of_nodes(), *g.edges())
    g1.edata[G.ETYPE] = torch.zeros_like(g.edata[G.ETYPE])
    rel = SM.NeighborSampler(g1, [[k], {0: k}]).sample(seeds, generator=torch.Generator().manual_seed(2))
    assert_blocks_equal(rel, SM.NeighborSampler(g1, [k, k]).sample(seeds, draws=[b.draws for b in rel]))


def test_per_relation_flag_reads_an_integer_as_one_per_type():
    g, seeds, _ = fixture_graph("ops")
    flag = SM.NeighborSampler(g, [2, None, 3], per_relation=True)
    assert flag.num_etypes == 7
    blocks = flag.sample(seeds, generator=torch.Generator().manual_seed(4))
    assert [None if b.draws is None else tuple(b.draws.shape)[1] for b in blocks] == [14, None, 21]
    same = SM.NeighborSampler(g, [[2] * 7, None, torch.full((7,), 3)]).sample(seeds, draws=[b.draws for b in blocks])
    assert_blocks_equal(blocks, same)
    # without the flag an integer keeps its meaning, and num_etypes pads the specification with types that do not occur
    wide = SM.NeighborSampler(g, [MIXED + [7, 7]], num_etypes=9).sample(seeds, generator=torch.Generator().manual_seed(4))
    assert tuple(wide[0].draws.shape)[1] == sum(f or 0 for f in MIXED) + 14
    narrow = SM.NeighborSampler(g, [MIXED]).sample(seeds, draws=[wide[0].draws[:, :-14].contiguous()])
    assert_blocks_equal(wide, narrow)


def test_runs_graph():
    g, seeds, spec, R = runs_graph()
    assert sorted(set(range(R)) - set(g.edata[G.ETYPE].tolist())) == [73]
    sampler = SM.NeighborSampler(g, [spec], num_etypes=R)
    (b,) = sampler.sample(seeds, generator=torch.Generator().manual_seed(8))
    check_layers(g, seeds, [spec], R, [b], sampler)
    ldst, eid, et = b.edges()[1], b.edata[G.EID], b.edata[G.ETYPE]
    assert torch.bincount(ldst * R + et, minlength=4 * R).view(4, R)[0, 70:72].tolist() == [64, 64]   # 64 kept whole, 65 cut to 64
    counts = torch.bincount(ldst, minlength=4).tolist()
    assert counts[0] == 128 and counts[2] == 0 and counts[3] == 0      # node 3 has no in-edges, node 2 only edges of a type with f = 0
    assert counts[1] == sum(kept(1 + r % 5, spec[r]) for r in range(70))
    assert b.dstdata[G.NID].tolist() == [1, 0, 3, 2]
    for i in range(4):                                                   # ascending edge ids inside each destination ...
        ids = eid[ldst == i].tolist()
        assert ids == sorted(ids) and len(set(ids)) == len(ids)
    for i in (0, 1):                                                     # ... which is NOT the order type by type
        t = et[ldst == i].tolist()
        assert t != sorted(t)
    again = SM.NeighborSampler(g, [dict(enumerate(spec)), spec], num_etypes=R)
    check_layers(g, seeds, [spec, spec], R, again.sample(seeds, generator=torch.Generator().manual_seed(9)), again)


def test_determinism_replay_and_the_tables():
    g, seeds, _ = fixture_graph("ops")
    layers = [[2] * 7, MIXED]
    sampler = SM.NeighborSampler(g, layers)
    first = sampler.sample(seeds, generator=torch.Generator().manual_seed(5))
    assert tables_at_rest(sampler)
    again = sampler.sample(seeds, generator=torch.Generator().manual_seed(5))
    assert_blocks_equal(again, first)
    assert all(torch.equal(a.draws, b.draws) for a, b in zip(again, first))
    replay = SM.NeighborSampler(g, layers).sample(seeds, draws=[b.draws for b in first])
    assert_blocks_equal(replay, first)
    other = sampler.sample(seeds, generator=torch.Generator().manual_seed(6))
    assert tables_at_rest(sampler)
    hub = lambda blocks: blocks[-1].edata[G.EID][blocks[-1].edges()[1] == 0]
    assert hub(other).numel() == hub(first).numel() and not torch.equal(hub(other), hub(first))
    # a raised error leaves the tables at rest as well
    n, K = int(seeds.numel()), sum(f or 0 for f in MIXED)
    for bad in ([None, torch.zeros(n, K + 1, dtype=torch.float64)], [None, torch.zeros(n + 1, K, dtype=torch.float64)],
                [None, torch.zeros(n, K)], [torch.zeros(n, K, dtype=torch.float64)], [None, None]):
        with pytest.raises(ValueError):
            sampler.sample(seeds, draws=bad)
        assert tables_at_rest(sampler)
    with pytest.raises(ValueError):
        SM.NeighborSampler(g, [[0] * 7]).sample(seeds, draws=[torch.zeros(n, 0, dtype=torch.float64)])   # K = 0 draws nothing
    with pytest.raises(ValueError):
        sampler.sample(torch.tensor([0, g.number_of_nodes()]))           # a seed outside the graph
    assert tables_at_rest(sampler)
    assert_blocks_equal(sampler.sample(seeds, draws=[b.draws for b in first]), first)


def test_the_picks_are_uniform_and_independent_across_types():
    """4 096 destinations with 5 in-edges of type 0 and 3 of type 1 at [2, 1]: Pearson's chi-square of the 10 x 3 joint table (pair
    of type-0 positions, type-1 position) against 136.53 each stays below the 0.999 quantile at 29 degrees of freedom (58.30); it
    tests both marginals and their independence.  A correct implementation gives 47.46 for this seed (seeds 0..19 give 14.0 to
    47.5, 26.4 on average against the expected 29)."""
    n = 4096
    dst = torch.arange(n).repeat_interleave(8)                          # edge 8 v + p: p < 5 is position p of type 0, else p - 5 of type 1
    g = G.RelGraph(n + 7, n + torch.arange(8 * n) % 7, dst)
    g.edata[G.ETYPE] = (torch.arange(8 * n) % 8 >= 5).long()
    (b,) = SM.NeighborSampler(g, [[2, 1]]).sample(torch.arange(n), generator=torch.Generator().manual_seed(0))
    assert tuple(b.draws.shape) == (n, 3)
    pos = (b.edata[G.EID] - 8 * b.edges()[1]).view(n, 3)
    assert bool((pos[:, 0] < pos[:, 1]).all()) and bool((pos[:, 1] < 5).all()) and bool((pos[:, 2] >= 5).all())
    counts = torch.bincount((pos[:, 0] * 5 + pos[:, 1]) * 3 + pos[:, 2] - 5, minlength=75).double()
    counts = counts[counts > 0]
    assert counts.numel() == 30
    chi2 = float(((counts - n / 30) ** 2 / (n / 30)).sum())
    print(f"chi-square {chi2:.2f}")
    assert chi2 < 58.30, chi2


def test_bad_specifications_raise():
    g, _, _ = fixture_graph("ops")
    ok = [1] * 7
    bad = [ok[:6], ok + [1],                                             # a wrong length
           {r: 1 for r in range(6)}, {**{r: 1 for r in range(7)}, 7: 1}, {**{r: 1 for r in range(7)}, -1: 1},   # a missing type, keys outside [0, R)
           {**{r: 1 for r in range(6)}, "6": 1},
           ok[:6] + [65], ok[:6] + [-2], ok[:6] + [2.0], ok[:6] + [True], ok[:6] + ["1"],                   # values outside the allowed set
           {**{r: 1 for r in range(6)}, 6: 65},
           torch.ones(7), torch.ones(7, 1, dtype=torch.long), torch.ones(6, dtype=torch.long), torch.full((7,), 65)]
    for spec in bad:
        with pytest.raises(ValueError):
            SM.NeighborSampler(g, [None, spec])
    with pytest.raises(ValueError):
        SM.NeighborSampler(g, [ok], num_etypes=6)                        # the graph has a type 6
    with pytest.raises(ValueError):
        SM.NeighborSampler(g, [ok + [1]], num_etypes=7)
    for bad_k in (0, 65, -2, 2.0):
        with pytest.raises(ValueError, match="64"):
            SM.NeighborSampler(g, [None, bad_k], per_relation=True)
    plain = G.RelGraph(g.number_of_nodes(), *g.edges())                  # no edge types
    for layers, kw in (([[1]], {}), ([{0: 1}], {}), ([1], {"per_relation": True}), ([[1] * 7], {"num_etypes": 7})):
        with pytest.raises(ValueError, match="edge types"):
            SM.NeighborSampler(plain, layers, **kw)
    SM.NeighborSampler(plain, [None, 2], num_etypes=7)                   # integer layers need none


# ---- the host side of the C ABI ----------------------------------------------------------------------------------------------------
def test_the_library_declares_the_new_entry_points_at_abi_23():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 23 and lib.mrg_abi_version() == 23
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(256)                                             # never dereferenced: every call below returns before a launch
    fan = lambda *f: (ctypes.c_int32 * len(f))(*f)                       # the HOST copy of the specification is read by the checks
    good = fan(2, 0, -1, 64)                                             # K = 66

    def sizes(rp=p, rs=p, rt=p, dst=p, n=8, N=100, fh=good, spec=p, R=4, first=p, ws=p, nb=1 << 30):
        return lib.mrg_block_rel_sizes(rp, rs, rt, dst, n, N, fh, spec, R, first, ws, nb, None)

    def emit(rp=p, rs=p, rt=p, re=p, so=p, to=p, EG=1000, dst=p, first=p, n=8, N=100, fh=good, spec=p, R=4, u=p, K=66, E=16, eid=p, et=p,
             ldst=p, gs=p, loc=p, fp=p, ws=p, nb=1 << 30):
        return lib.mrg_block_rel_emit(rp, rs, rt, re, so, to, EG, dst, first, n, N, fh, spec, R, u, K, E, eid, et, ldst, gs, loc, fp, ws, nb, None)

    # NULL pointers -> MRG_E_NULLPTR
    for kw in ("rp", "rs", "rt", "dst", "fh", "spec", "first"):
        assert sizes(**{kw: None}) == -1, kw
    for kw in ("rp", "rs", "rt", "re", "so", "dst", "first", "fh", "spec", "u", "eid", "ldst", "gs", "loc", "fp"):
        assert emit(**{kw: None}) == -1, kw
    assert emit(to=None) == -1                                           # types asked for without the graph's types
    # negative sizes, no type at all, an entry outside -1..64, a K that is not the sum of the entries >= 1 -> MRG_E_SHAPE
    assert sizes(n=-1) == -2 and sizes(N=-1) == -2 and sizes(R=0) == -2 and sizes(R=-1) == -2
    assert emit(n=-1) == -2 and emit(N=-1) == -2 and emit(R=0) == -2 and emit(E=-1) == -2 and emit(EG=-1) == -2
    assert emit(E=2 ** 31) == -2 and emit(EG=2 ** 31) == -2
    for f in (65, -2, 1000):
        assert sizes(fh=fan(2, 0, f, 64)) == -2 and emit(fh=fan(2, 0, f, 64)) == -2, f
        assert sizes(fh=fan(f), R=1, n=0) == -2 and emit(fh=fan(f), R=1, K=0, E=0) == -2, f     # checked even with nothing to do
    assert emit(K=65) == -2 and emit(K=0) == -2 and emit(K=-1) == -2
    # a missing or short workspace -> MRG_E_WORKSPACE
    assert sizes(ws=None) == -4 and emit(ws=None) == -4
    assert lib.mrg_block_rel_sizes_workspace_bytes(8) > 0 and lib.mrg_block_rel_emit_workspace_bytes(16) >= 2 * 16 * 8
    assert sizes(nb=lib.mrg_block_rel_sizes_workspace_bytes(8) - 1) == -4
    assert emit(nb=lib.mrg_block_rel_emit_workspace_bytes(16) - 1) == -4
    # nothing to do -> MRG_OK, nothing launched (NULL pointers are then fine)
    assert sizes(n=0, rp=None, spec=None, ws=None) == 0
    assert emit(n=0, rp=None, ws=None) == 0 and emit(E=0, eid=None, ws=None) == 0
    assert emit(fh=fan(0, -1), R=2, K=0, u=None, E=0) == 0
    # the queries are host functions of the size
    assert lib.mrg_block_rel_sizes_workspace_bytes(-1) == 0 and lib.mrg_block_rel_emit_workspace_bytes(-1) == 0
    assert lib.mrg_block_rel_emit_workspace_bytes(2 ** 31) == 0
    assert lib.mrg_block_rel_emit_workspace_bytes(1 << 20) > lib.mrg_block_rel_emit_workspace_bytes(1 << 10)
