"""Search-step sampling, negative sampling and label construction on the device -- the data preparation around the
hot path that the reference does in numpy on the host for every step:

* ``generate_sampled_graph_and_labels`` / ``sample_edge_uniform`` / ``negative_sampling``
  (reference utils/utils_rgcn.py:73-118, 191-204): same names, same return values, tensors instead of numpy arrays;
* ``LabelIndex`` (reference utils/process_data.py:4-31 + utils/data_set.py:6-59): the ``sr2o`` dictionaries as a
  sorted key / CSR pair in HBM and the dense (label-smoothed) ``[B, num_ent]`` targets of a batch.

Everything integer runs in the HIP kernels of ``csrc/sampling.hip`` / ``csrc/plans.hip`` behind the C ABI.  Random
draws come from torch's device generator (the reference uses numpy's global generator; bit-equal streams are not
possible across generators), but every function takes the draws as optional arguments and is bit-exact with the
reference for the same draws -- that is what the tests replay.  The neighbourhood-expansion sampler
(``sample_edge_neighborhood``, utils_rgcn.py:30-71, ``--edge_sampler neighbor``) is ``sample_size`` dependent picks: one
launch of one persistent workgroup (``mrg_sample_edge_neighborhood``) over an adjacency CSR in the reference's append order.

Node classification: ``full_neighbor_blocks`` (torch ops, every in-edge) and ``NeighborSampler`` (per-layer fan-outs over a resident
in-edge index, over all in-edges or per edge type; the kernels of ``csrc/blocks.hip`` and ``csrc/blocks_rel.hip``) build the blocks of
a minibatch.
"""
import ctypes

import numpy as np
import torch

from . import graph as G
from ._lib import call, load, ptr, require_hip, stream_of


def sample_edge_uniform(n_triplets, sample_size, device, generator=None):
    """`np.random.choice(n_triplets, sample_size, replace=False)` (reference utils/utils_rgcn.py:73-76)."""
    return torch.randperm(int(n_triplets), device=device, generator=generator)[: int(sample_size)]


class AdjIndex:
    """``get_adj_and_degrees`` (reference utils/utils_rgcn.py:18-28) resident in HBM: the adjacency lists in the reference's
    append order (for triple i: ``[i, o]`` joins s's list, then ``[i, s]`` joins o's) as a CSR, plus the degrees."""

    def __init__(self, num_nodes, triplets):
        t = triplets.long()
        T, dev = int(t.shape[0]), t.device
        self.N, self.T = int(num_nodes), T
        vert = torch.stack((t[:, 0], t[:, 2]), dim=1).reshape(-1)            # entry 2i: s's list, entry 2i + 1: o's list
        other = torch.stack((t[:, 2], t[:, 0]), dim=1).reshape(-1)
        eid = torch.arange(T, device=dev).repeat_interleave(2)
        order = torch.sort(vert, stable=True).indices                        # stable: append order inside every list
        self.adj_edge = eid[order].to(torch.int32).contiguous()
        self.adj_other = other[order].to(torch.int32).contiguous()
        deg = torch.bincount(vert, minlength=self.N)
        self.degrees = deg.to(torch.int32).contiguous()
        rowptr = torch.zeros(self.N + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(deg, 0)
        self.rowptr = rowptr.to(torch.int32).contiguous()
        G.settle(dev)


def sample_edge_neighborhood(adj, sample_size, draws=None, generator=None):
    """Reference utils/utils_rgcn.py:30-71: `sample_size` edges by neighbourhood expansion (the sampled edges form a connected
    graph).  `adj`: AdjIndex.  `draws`: dict(u_vertex=float64 [sample_size], tries=int64 [n]) replays the reference's own draws
    (the uniform behind every `np.random.choice(..., p=...)` and the sequence of adjacency slots it tried, rejected ones
    included): bit-exact.  Without draws the uniforms come from torch's device generator and the edge of a vertex is ONE draw
    among its unpicked entries (the reference's distribution without its rejection loop).  Returns int64 edge ids."""
    dev = adj.rowptr.device
    S = int(sample_size)
    draws = draws or {}
    u_vertex = draws.get("u_vertex")
    u_vertex = (torch.rand(S, dtype=torch.float64, device=dev, generator=generator) if u_vertex is None
                else torch.as_tensor(u_vertex).to(dev).double().contiguous())
    tries = draws.get("tries")
    u_edge = None
    if tries is None:
        u_edge = torch.rand(S, dtype=torch.float64, device=dev, generator=generator)
    else:
        tries = torch.as_tensor(tries).to(dev).long().contiguous()
    if u_vertex.numel() != S:
        raise ValueError(f"sample_edge_neighborhood needs {S} vertex draws, got {u_vertex.numel()}")
    require_hip(adj.rowptr, u_vertex, tries, u_edge)
    edges = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.zeros(3, dtype=torch.int64, device=dev)
    nb = load().mrg_sample_neighborhood_workspace_bytes(adj.N, adj.T)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    call("mrg_sample_edge_neighborhood", (ptr(adj.rowptr), ptr(adj.adj_edge), ptr(adj.adj_other), ptr(adj.degrees), adj.N, adj.T, S, ptr(u_vertex),
                                          ptr(tries), int(tries.numel()) if tries is not None else 0, ptr(u_edge), ptr(edges), ptr(status),
                                          ptr(ws), nb, stream_of(edges)))
    made, used, code = (int(v) for v in status.tolist())
    if code != 0 or made != S:
        raise RuntimeError({1: "sample_edge_neighborhood: the graph has fewer incident edges than sample_size",
                            2: "sample_edge_neighborhood: a replayed adjacency slot is out of range",
                            3: "sample_edge_neighborhood: the replayed tries ran out"}.get(code, f"sample_edge_neighborhood failed (code {code})")
                           + f" after {made} of {S} picks")
    return edges.long()


def negative_sampling(pos_samples, num_entity, negative_rate, values=None, choices=None, generator=None):
    """Reference utils/utils_rgcn.py:191-204.  pos_samples [B, 3] int64 on the device; returns (samples
    [(rate+1) B, 3] int64, labels float32).  `values` (int64 [B * rate] in [0, num_entity)) and `choices` (float64
    [B * rate] in [0, 1)) are the reference's two random draws; drawn on the device when absent.  `num_entity` may be a DEVICE
    tensor (the node count of a static step graph, static_step below): the bound of the drawn entity ids then never visits the host."""
    pos = pos_samples.long().contiguous()
    require_hip(pos)
    B, n = int(pos.shape[0]), int(pos.shape[0]) * int(negative_rate)
    dev = pos.device
    if values is None and torch.is_tensor(num_entity):
        ne = num_entity.to(torch.float64).reshape(())
        values = torch.minimum((torch.rand(n, device=dev, dtype=torch.float64, generator=generator) * ne).floor(), ne - 1).clamp_(min=0).long()
    elif values is None:
        values = torch.randint(0, int(num_entity), (n,), device=dev, generator=generator)
    if choices is None:
        choices = torch.rand(n, device=dev, dtype=torch.float64, generator=generator)
    values, choices = values.to(dev).long().contiguous(), choices.to(dev).double().contiguous()
    if values.numel() != n or choices.numel() != n:
        raise ValueError(f"negative_sampling needs {n} draws, got {values.numel()} / {choices.numel()}")
    samples = torch.empty(B * (negative_rate + 1), 3, dtype=torch.int64, device=dev)
    labels = torch.empty(B * (negative_rate + 1), dtype=torch.float32, device=dev)
    call("mrg_negative_sampling", (ptr(pos), B, int(negative_rate), ptr(values), ptr(choices), ptr(samples), ptr(labels), stream_of(pos)))
    return samples, labels


def relabel_nodes(src, dst, num_nodes, static=False):
    """`uniq_v, edges = np.unique((src, dst), return_inverse=True)` (reference utils/utils_rgcn.py:97-101):
    returns (uniq_v ascending, new_src, new_dst).  static: no host read -- returns (uniq_v padded with node 0 to its host-known
    capacity min(2 n, num_nodes), new_src, new_dst, count [1] int32 on the device)."""
    src, dst = src.long().contiguous(), dst.long().contiguous()
    require_hip(src, dst)
    dev, n = src.device, int(src.numel())
    cap = max(min(2 * n, int(num_nodes)), 1)
    uniq = torch.zeros(cap, dtype=torch.int64, device=dev) if static else torch.empty(cap, dtype=torch.int64, device=dev)
    ns, nd = torch.empty_like(src), torch.empty_like(dst)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = load().mrg_relabel_workspace_bytes(int(num_nodes))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    call("mrg_relabel_nodes", (ptr(src), ptr(dst), n, int(num_nodes), ptr(uniq), ptr(ns), ptr(nd), ptr(count), ptr(ws), nb, stream_of(src)))
    if static:
        return uniq, ns, nd, count
    return uniq[: int(count.item())], ns, nd


def static_step(triplets, sample_size, split_size, num_rels, negative_rate, num_nodes, generator=None):
    """generate_sampled_graph_and_labels (uniform sampler) WITHOUT a host read and with host-known shapes, so that a whole search step
    -- this function included -- can be captured into one HIP graph and replayed with a new draw every time (reference
    search/mr_lp_search.py:187-245: a new step graph per step; utils/utils_rgcn.py:79-118).  The number of distinct nodes of a draw
    stays in device memory: the step graph has `cap = min(2 * sample_size, num_nodes)` nodes, of which the first *n_nodes are the
    draw's (relabelled 0 .. n - 1 as the reference does) and the rest are isolated padding nodes (uniq_v entry 0; no edge touches
    them; the MixedOp kernels keep their rows zero and out of every statistic: the graph carries the counts as g.valid_rows, which
    cell_lp.fused_candidates hands to the epilogues, and supernet.SearchNetwork.static_rows switches the padded step on).
    Draws come from torch's default device generator unless `generator` is registered with the capturing graph.
    Returns dict(g, node_id [cap, 1], src, rel, samples, labels, n_nodes [1] int32, n_rows [1] int32 = E + n_nodes, cap)."""
    dev = triplets.device
    T = int(triplets.shape[0])
    pick = sample_edge_uniform(T, sample_size, dev, generator)
    edges = triplets[pick].long()
    uniq_v, src, dst, count = relabel_nodes(edges[:, 0], edges[:, 2], num_nodes, static=True)
    rel = edges[:, 1].contiguous()
    relabeled = torch.stack((src, rel, dst), dim=1)
    samples, labels = negative_sampling(relabeled, count, negative_rate, generator=generator)
    n_split = int(sample_size * split_size)
    split = torch.randperm(int(sample_size), device=dev, generator=generator)[:n_split]
    cap = int(uniq_v.numel())
    graph_triples = relabeled[split]
    g = G.build_search_graph(cap, num_rels, graph_triples, device=dev)
    src_o, _, _ = g.edges(form="all")
    n_rows = (count + int(g.num_edges())).to(torch.int32)
    g.valid_rows = {int(g.num_edges()) + cap: n_rows, cap: count}
    return dict(g=g, node_id=uniq_v.view(-1, 1), src=src_o, rel=g.edata["e_type"], samples=samples, labels=labels,
                n_nodes=count, n_rows=n_rows, cap=cap, graph_triples=graph_triples)


def generate_sampled_graph_and_labels(triplets, sample_size, split_size, num_rels, negative_rate, num_nodes, sampler="uniform",
                                      draws=None, generator=None, adj=None):
    """One search-step sample (reference utils/utils_rgcn.py:79-118).  `triplets` [T, 3] int64 on the device.
    Returns ``(g, uniq_v, src, rel, node_norm, samples, labels)`` like the reference, with ``g`` a RelGraph that
    already carries ``edata['e_type']`` and the edge norm ``edata['norm']`` [E, 1] (what the search driver computes
    next with node_norm_to_edge_norm, search/mr_lp_search.py:30-36,214), everything resident in HBM.
    `draws`: optional dict(edges, values, choices, split) replaying the reference's four random draws; with
    sampler="neighbor" (reference :92-93) the edge draw is dict(u_vertex, tries) instead of `edges` (sample_edge_neighborhood)
    and `adj` may carry a prebuilt AdjIndex of `triplets` (the reference builds its adjacency lists once per run)."""
    if sampler not in ("uniform", "neighbor"):
        raise ValueError("Sampler type must be either 'uniform' or 'neighbor'.")
    draws = draws or {}
    dev = triplets.device
    T = int(triplets.shape[0])
    pick = draws.get("edges")
    if pick is not None:
        pick = torch.as_tensor(pick).to(dev).long()
    elif sampler == "uniform":
        pick = sample_edge_uniform(T, sample_size, dev, generator)
    else:
        adj = adj if adj is not None else AdjIndex(num_nodes, triplets)
        pick = sample_edge_neighborhood(adj, sample_size, {k: draws[k] for k in ("u_vertex", "tries") if k in draws} or None, generator)
    edges = triplets[pick].long()
    uniq_v, src, dst = relabel_nodes(edges[:, 0], edges[:, 2], num_nodes)
    rel = edges[:, 1].contiguous()
    relabeled = torch.stack((src, rel, dst), dim=1)
    samples, labels = negative_sampling(relabeled, int(uniq_v.numel()), negative_rate, draws.get("values"), draws.get("choices"), generator)
    n_split = int(sample_size * split_size)
    split = draws.get("split")
    split = torch.randperm(int(sample_size), device=dev, generator=generator)[:n_split] if split is None else torch.as_tensor(split).to(dev).long()
    g = G.build_search_graph(int(uniq_v.numel()), num_rels, relabeled[split], device=dev)
    src_o, _, _ = g.edges(form="all")
    deg = g._in_degree32.long()
    node_norm = G._deg_norm_table(dev, int(g.num_edges()) + 1)[deg]
    return g, uniq_v, src_o, g.edata["e_type"], node_norm, samples, labels


class LabelIndex:
    """``sr2o`` of process() (reference utils/process_data.py:4-31) resident in HBM: for every (subject, relation) pair
    -- relations r and r + num_rel for the inverse direction -- the set of known objects, as ascending keys
    ``subject * 2R + relation`` with a CSR of object ids.  ``labels(subj, rel)`` is TrainDataset / TestDataset.get_label
    for a batch (reference utils/data_set.py:21-33), optionally label-smoothed like TrainDataset.__getitem__ (:21-23)."""

    def __init__(self, triples, num_rel, num_ent, device):
        t = torch.as_tensor(np.asarray(triples) if not torch.is_tensor(triples) else triples).to(device).long()
        s, r, o = t[:, 0], t[:, 1], t[:, 2]
        self.num_rel, self.num_ent = int(num_rel), int(num_ent)
        key = torch.cat((s * (2 * num_rel) + r, o * (2 * num_rel) + r + num_rel))
        obj = torch.cat((o, s))
        pair = torch.unique(key * num_ent + obj)                          # the sets of sr2o: duplicates collapse; ascending
        key_s, obj_s = pair // num_ent, pair % num_ent
        self.keys, counts = torch.unique_consecutive(key_s, return_counts=True)
        rowptr = torch.zeros(self.keys.numel() + 1, dtype=torch.int64, device=t.device)
        rowptr[1:] = torch.cumsum(counts, 0)
        self.rowptr, self.objs = rowptr.to(torch.int32).contiguous(), obj_s.to(torch.int32).contiguous()
        G.settle(t.device)

    def label_values(self, label_smooth=0.0):
        """(v_zero, v_one): the two values a label takes, as Python floats that are exact float32."""
        v = torch.tensor([0.0, 1.0])
        if label_smooth != 0.0:                                             # the reference's own float32 expression (data_set.py:23)
            v = (1.0 - label_smooth) * v + (1.0 / self.num_ent)
        return float(v[0]), float(v[1])

    def labels(self, subj, rel, label_smooth=0.0):
        subj, rel = subj.long(), rel.long()
        q = (subj * (2 * self.num_rel) + rel).contiguous()
        require_hip(q)
        B = int(q.numel())
        out = torch.empty(B, self.num_ent, dtype=torch.float32, device=q.device)
        v = self.label_values(label_smooth)
        call("mrg_multi_hot_labels", (ptr(self.keys), ptr(self.rowptr), ptr(self.objs), ptr(q), B, int(self.keys.numel()), self.num_ent,
                                      float(v[0]), float(v[1]), ptr(out), stream_of(q)))
        return out


def _edge_types(graph):
    for key in (G.ETYPE, "e_type", "etype"):
        if key in graph.edata:
            return graph.edata[key]
    return None


def full_neighbor_blocks(graph, seeds, num_layers):
    """The blocks of DGL's ``MultiLayerFullNeighborSampler(num_layers, return_eids=True)`` for the destination nodes ``seeds``
    (reference search/mr_nc_search.py:43, train/mr_nc_train.py:42), outermost first, as graph.Block objects:

    * the last block's destination nodes are ``seeds`` (unique ids), in the given order;
    * block j's destination nodes are block j + 1's source nodes, in the same order;
    * a block's source nodes are its destination nodes first, then the new sources in order of first appearance over its edge list;
    * a block's edges are every in-edge of its destination nodes, grouped by destination in destination order, edge ids ascending
      within a destination; ``edata[EID]`` holds their ids in ``graph``, ``edata[ETYPE]`` their types (graph.edata[ETYPE], or
      'e_type' / 'etype').

    Torch ops on the tensors' device (CPU included); two host reads of sizes per layer."""
    dev = graph.device
    N = graph.number_of_nodes()
    gsrc, gdst = graph.edges()
    gsrc, gdst = gsrc.long(), gdst.long()
    etype = _edge_types(graph)
    order = torch.argsort(gdst, stable=True)                         # edge ids by destination, ascending within one
    deg = torch.zeros(N, dtype=torch.long, device=dev).scatter_add_(0, gdst, torch.ones_like(gdst))
    rowptr = torch.cumsum(deg, 0) - deg
    dst_nodes = torch.as_tensor(seeds, device=dev).long().reshape(-1)
    blocks = []
    for _ in range(int(num_layers)):
        n_dst = int(dst_nodes.numel())
        d = deg[dst_nodes]
        E = int(d.sum())                                             # host read 1
        ldst = torch.repeat_interleave(torch.arange(n_dst, device=dev), d, output_size=E)
        first = torch.cumsum(d, 0) - d
        pos = torch.arange(E, device=dev) - first[ldst] + rowptr[dst_nodes][ldst]
        eid = order[pos]
        s = gsrc[eid]
        local = torch.full((N,), -1, dtype=torch.long, device=dev)
        local[dst_nodes] = torch.arange(n_dst, device=dev)
        firstpos = torch.full((N,), E, dtype=torch.long, device=dev)
        firstpos.scatter_reduce_(0, s, torch.arange(E, device=dev), reduce="amin")
        fresh = (local[s] < 0) & (firstpos[s] == torch.arange(E, device=dev))
        new = s[fresh]                                               # new sources in order of first appearance (host read 2)
        local[new] = torch.arange(n_dst, n_dst + int(new.numel()), device=dev)
        src_nodes = torch.cat((dst_nodes, new))
        blocks.append(G.Block(src_nodes, dst_nodes, local[s], ldst, eid, etype[eid].long() if etype is not None else None))
        dst_nodes = src_nodes
    return blocks[::-1]


MAX_FANOUT = 64          # csrc/blocks.hip: one lane of a wave per pick
_I32_MAX = 2 ** 31 - 1


def _check_fanout(f):
    """None (every in-edge; -1 says the same) or the integer fan-out 1..MAX_FANOUT."""
    if f is None:
        return None
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)):
        raise ValueError(f"a fan-out is None, -1 or an integer in 1..{MAX_FANOUT}, got {f!r}")
    f = int(f)
    if f == -1:
        return None
    if not 1 <= f <= MAX_FANOUT:
        raise ValueError(f"a fan-out is None, -1 or an integer in 1..{MAX_FANOUT} (the limit is {MAX_FANOUT}), got {f}")
    return f



def _check_rel_fanout(f):
    """An entry of a per-relation specification: None (every in-edge of the type; -1 says the same), 0 (none) or 1..MAX_FANOUT."""
    if f is None:
        return None
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)):
        raise ValueError(f"a per-relation fan-out is None, -1, 0 or an integer in 1..{MAX_FANOUT}, got {f!r}")
    f = int(f)
    if f == -1:
        return None
    if not 0 <= f <= MAX_FANOUT:
        raise ValueError(f"a per-relation fan-out is None, -1, 0 or an integer in 1..{MAX_FANOUT} (the limit is {MAX_FANOUT}), got {f}")
    return f


class _RelSpec:
    """One per-relation layer: ``f[r]`` per edge type (None = every in-edge of the type), ``K`` = the width of its uniforms (the sum
    of the integer entries >= 1; type r reads the columns ``[off_r, off_r + f_r)``, off_r = the sum over the lower types), and the two
    copies csrc/blocks_rel.hip takes: ``fan_host`` (a host int32 array, -1 for None) and ``spec`` (int32 [2 R] on the sampler's
    device: the same entries, then the offsets)."""

    def __init__(self, f, device):
        self.f = tuple(f)
        self.R = len(self.f)
        fan = [-1 if x is None else x for x in self.f]
        off = [sum(max(x, 0) for x in fan[:r]) for r in range(self.R)]
        self.K = sum(max(x, 0) for x in fan)
        self.fan_host = (ctypes.c_int32 * self.R)(*fan)
        self.spec = torch.tensor(fan + off, dtype=torch.int32, device=device)

    def __repr__(self):
        return f"per-relation{list(self.f)}"


def _rel_entries(f, R):
    """The R entries of a per-relation layer given as a dict {etype: f} or a 1-D sequence / integer tensor of length R."""
    if isinstance(f, dict):
        for key in f:
            if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < R:
                raise ValueError(f"a per-relation fan-out names the edge types 0..{R - 1}, got the key {key!r}")
        given = {int(key): v for key, v in f.items()}
        missing = [r for r in range(R) if r not in given]
        if missing:
            raise ValueError(f"a per-relation fan-out names every edge type 0..{R - 1}; missing {missing[:8]}")
        return [_check_rel_fanout(given[r]) for r in range(R)]
    if torch.is_tensor(f) or isinstance(f, np.ndarray):
        if f.ndim != 1 or (f.dtype.is_floating_point or f.dtype == torch.bool if torch.is_tensor(f) else f.dtype.kind not in "iu"):
            raise ValueError(f"a per-relation fan-out tensor is 1-D and integer, got {f.dtype} with {f.ndim} dimensions")
        f = [int(x) for x in f.tolist()]
    f = list(f)
    if len(f) != R:
        raise ValueError(f"a per-relation fan-out has one entry per edge type ({R}), got {len(f)}")
    return [_check_rel_fanout(x) for x in f]


class NeighborSampler:
    """DGL's ``MultiLayerNeighborSampler(fanouts, return_eids=True)`` (reference search/mr_nc_search.py:39-44, 231: ``--fanout``)
    over a resident in-edge index of ``graph``: ``sample(seeds)`` returns the blocks of a minibatch, outermost first, with the
    conventions of ``full_neighbor_blocks`` (destinations of the last block = ``seeds`` in order; block j's destinations = block
    j + 1's sources; sources = destinations first, then new sources in order of first appearance over the edge list; edges grouped
    by destination in destination order, edge ids ascending within one; ``EID`` / ``ETYPE`` / ``NID`` filled).

    ``fanouts[j]`` belongs to ``blocks[j]`` (DGL's order: the last entry is the seeds' block).  ``None`` / ``-1``: every in-edge.
    An integer k in 1..64: a destination of in-degree d <= k keeps all its in-edges, one with d > k a uniformly random k-subset
    of the positions 0..d-1 of its in-list (ascending edge id), chosen by Floyd's algorithm from its row of uniforms ``u[v, 0..k-1]``
    (float64 in [0, 1)): for i = 0..k-1, j = d - k + i, t = min(floor(u_i (j + 1)), j); pick j when t is already picked, else t.
    Layers are processed from the seeds outwards and every integer layer draws ONE ``torch.rand((n_dst, k), dtype=float64)`` from
    ``generator`` (rows of destinations with d <= k are drawn and ignored: the stream depends on shapes only); the tensor stays on
    the block as ``block.draws``.  ``draws=[...]`` (aligned with ``fanouts``; None for a full layer) replays a run.

    The index (rowptr over destinations; edge ids, sources and types in stable destination order) and two [N] int32 scratch tables
    are built once, on ``graph.device``.  On a HIP graph a layer is three entry points of csrc/blocks.hip (mrg_block_sizes,
    mrg_block_emit, mrg_block_relabel) and two host reads of sizes; nothing per call grows with the graph.  CPU graphs run the torch
    formulation of the same function.  Preconditions: ``seeds`` are unique node ids.  The scratch tables are shared by all calls:
    a sampler object is used from ONE stream at a time.

    Per-relation layers (DGL's fan-out per edge type; ``sample_etype_neighbors`` on a homogenised graph).  With R edge types
    (``num_etypes``, else 1 + the largest type of the graph, read once here) ``fanouts[j]`` may also be a dict ``{etype: f}`` naming
    every type or a 1-D sequence / integer tensor of length R; every ``f`` is None / -1 (every in-edge of the type), 0 (none) or an
    integer 1..64.  ``per_relation=True`` reads an integer entry k as ``[k] * R`` (None keeps its meaning).  A run (v, r) is the
    in-edges of destination v with type r in ascending edge id, d_vr its length: v keeps nothing of it when f_r = 0, all of it when
    f_r is None or d_vr <= f_r, else the f_r positions of the run that Floyd's recurrence above picks with d = d_vr, k = f_r.  The
    block keeps every convention above; edge ids ascend inside a destination ACROSS the types.  Such a layer draws ONE
    ``torch.rand((n_dst, K), dtype=float64)``, K = the sum of its integer entries >= 1, of which type r reads the columns
    ``[off_r, off_r + f_r)``, off_r = the sum of the integer entries of the lower types (columns of absent or short runs are drawn
    and ignored); K = 0 draws nothing.  Its index -- the in-edges in stable (destination, type, edge id) order and the table of
    runs -- is built here only when some layer is per-relation; on a HIP graph the layer is mrg_block_rel_sizes, mrg_block_rel_emit
    (csrc/blocks_rel.hip) and mrg_block_relabel, again with two host reads."""

    def __init__(self, graph, fanouts, num_etypes=None, per_relation=False):
        dev = self.device = graph.device
        etype = _edge_types(graph)
        fanouts = list(fanouts)
        scalar = lambda f: f is None or (isinstance(f, (int, np.integer)) and not isinstance(f, bool)) or isinstance(f, (float, str, bytes))
        rel = [not scalar(f) or (per_relation and _check_fanout(f) is not None) for f in fanouts]
        R = self.num_etypes = None
        if any(rel):
            if etype is None:
                raise ValueError("a per-relation fan-out needs a graph with edge types")
            R = int(num_etypes) if num_etypes is not None else (int(etype.max()) + 1 if etype.numel() else 1)
            if R < 1 or (etype.numel() and not (0 <= int(etype.min()) and int(etype.max()) < R)):
                raise ValueError(f"NeighborSampler: an edge type lies outside [0, {R})")
            self.num_etypes = R
        self.fanouts = [(_RelSpec(_rel_entries([f] * R if scalar(f) else f, R), dev) if is_rel else _check_fanout(f))
                        for f, is_rel in zip(fanouts, rel)]
        N = self.N = graph.number_of_nodes()
        gsrc, gdst = graph.edges()
        gsrc, gdst = gsrc.long(), gdst.long()
        E = int(gsrc.numel())
        if E > _I32_MAX - 1 or N > _I32_MAX - 1:
            raise ValueError("NeighborSampler indexes nodes and edges with int32")
        if E and not (0 <= int(torch.minimum(gsrc.min(), gdst.min())) and int(torch.maximum(gsrc.max(), gdst.max())) < N):
            raise ValueError("NeighborSampler: an edge endpoint lies outside [0, number_of_nodes())")
        etype = _edge_types(graph)
        order = torch.argsort(gdst, stable=True)                         # edge ids by destination, ascending within one
        deg = torch.zeros(N, dtype=torch.long, device=dev).scatter_add_(0, gdst, torch.ones_like(gdst))
        rowptr = torch.zeros(N + 1, dtype=torch.long, device=dev)
        rowptr[1:] = torch.cumsum(deg, 0)
        i32 = lambda t: t.to(torch.int32).contiguous()
        self.rowptr, self.in_eid, self.in_src = i32(rowptr), i32(order), i32(gsrc[order])
        self.in_type = i32(etype[order]) if etype is not None else None
        self.local = torch.full((N,), -1, dtype=torch.int32, device=dev)            # -1 everywhere between calls
        self.firstpos = torch.full((N,), _I32_MAX, dtype=torch.int32, device=dev)   # INT32_MAX everywhere between calls
        if any(rel):                                                     # the runs (destination, type), edge ids ascending inside one
            by_type = torch.argsort(etype.long(), stable=True)
            order = by_type[torch.argsort(gdst[by_type], stable=True)]
            d_s, t_s = gdst[order], etype.long()[order]
            head = torch.ones(E, dtype=torch.bool, device=dev)
            head[1:] = (d_s[1:] != d_s[:-1]) | (t_s[1:] != t_s[:-1])
            start = torch.nonzero(head).reshape(-1)
            run_ptr = torch.zeros(N + 1, dtype=torch.long, device=dev)
            run_ptr[1:] = torch.cumsum(torch.bincount(d_s[start], minlength=N), 0)
            self.rel_eid, self.run_ptr, self.run_type = i32(order), i32(run_ptr), i32(t_s[start])
            self.run_start = i32(torch.cat((start, torch.tensor([E], device=dev))))
            self.src_of, self.type_of = i32(gsrc), i32(etype)
        self._hip = G._hip_ready(gsrc)
        G.settle(dev)

    def sample(self, seeds, generator=None, draws=None):
        dev, L = self.device, len(self.fanouts)
        if draws is not None and len(draws) != L:
            raise ValueError(f"draws needs one entry per fan-out ({L}), got {len(draws)}")
        dst_nodes = torch.as_tensor(seeds, device=dev).long().reshape(-1).contiguous()
        layer = self._layer_hip if self._hip else self._layer_torch
        rel_layer = self._layer_rel_hip if self._hip else self._layer_rel_torch
        blocks = []
        for j in reversed(range(L)):
            k, n_dst, u = self.fanouts[j], int(dst_nodes.numel()), None
            rel = isinstance(k, _RelSpec)
            width = k.K if rel else (k or 0)                                  # the uniforms of a row; 0: the layer draws nothing
            if width and draws is None:
                u = torch.rand((n_dst, width), dtype=torch.float64, device=dev, generator=generator)
            elif width:
                u = draws[j]
                if not torch.is_tensor(u) or u.dtype != torch.float64 or tuple(u.shape) != (n_dst, width):
                    raise ValueError(f"draws[{j}] must be a float64 tensor of shape ({n_dst}, {width}), got "
                                     + (f"{u.dtype} {tuple(u.shape)}" if torch.is_tensor(u) else repr(type(u))))
                u = u.to(dev).contiguous()
            elif draws is not None and draws[j] is not None:
                raise ValueError(f"draws[{j}] must be None: layer {j} draws no uniforms")
            try:
                blk = (rel_layer if rel else layer)(dst_nodes, k, u)
            except Exception:
                self.local.fill_(-1)                                          # a failed layer may have left its entries behind
                self.firstpos.fill_(_I32_MAX)
                raise
            blk.draws = u
            blocks.append(blk)
            dst_nodes = blk.srcdata[G.NID]
        return blocks[::-1]

    def _layer_hip(self, dst_nodes, k, u):
        dev, N, n_dst, k = self.device, self.N, int(dst_nodes.numel()), int(k or 0)
        lib, st = load(), stream_of(dst_nodes)
        i64 = lambda n: torch.empty(int(n), dtype=torch.int64, device=dev)
        E = 0
        if n_dst:
            first = torch.empty(n_dst + 1, dtype=torch.int32, device=dev)
            nb = lib.mrg_block_sizes_workspace_bytes(n_dst)
            ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
            call("mrg_block_sizes", (ptr(self.rowptr), ptr(dst_nodes), n_dst, N, k, ptr(first), ptr(ws), nb, st))
            E = int(first[n_dst])                                             # host read 1
            if E < 0:
                raise ValueError("NeighborSampler: the block has more than 2^31 - 1 edges (are the seeds unique?)")
        eid, ldst, lsrc = i64(E), i64(E), i64(E)
        etype = i64(E) if self.in_type is not None else None
        if E == 0:
            return G.Block(dst_nodes, dst_nodes, lsrc, ldst, eid, etype)
        gsrc = torch.empty(E, dtype=torch.int32, device=dev)
        src_nodes = i64(n_dst + E)
        n_new = torch.empty(1, dtype=torch.int32, device=dev)
        nb = lib.mrg_block_relabel_workspace_bytes(E)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        call("mrg_block_emit", (ptr(self.rowptr), ptr(self.in_eid), ptr(self.in_src), ptr(self.in_type), ptr(dst_nodes), ptr(first), n_dst, N, k,
                                ptr(u), E, ptr(eid), ptr(etype), ptr(ldst), ptr(gsrc), ptr(self.local), ptr(self.firstpos), st))
        call("mrg_block_relabel", (ptr(gsrc), ptr(dst_nodes), n_dst, N, E, ptr(self.local), ptr(self.firstpos), ptr(src_nodes), ptr(lsrc),
                                   ptr(n_new), ptr(ws), nb, st))
        src_nodes = src_nodes[: n_dst + int(n_new)]                            # host read 2
        return G.Block(src_nodes, dst_nodes, lsrc, ldst, eid, etype)

    def _layer_torch(self, dst_nodes, k, u):
        """The same function in torch ops; like the kernels it touches the two tables at the block's nodes only."""
        dev, n_dst = self.device, int(dst_nodes.numel())
        if n_dst and not (0 <= int(dst_nodes.min()) and int(dst_nodes.max()) < self.N):
            raise ValueError("NeighborSampler: a seed lies outside [0, number_of_nodes())")
        r0 = self.rowptr[dst_nodes].long()
        d = self.rowptr[dst_nodes + 1].long() - r0
        if k is None:
            E = int(d.sum())
            ldst = torch.repeat_interleave(torch.arange(n_dst, device=dev), d, output_size=E)
            pos = torch.arange(E, device=dev) - (torch.cumsum(d, 0) - d)[ldst] + r0[ldst]
        else:
            pick = torch.arange(k, device=dev).repeat(n_dst, 1)              # d <= k: positions 0..d-1
            big = d > k
            if bool(big.any()):                                                # Floyd's k picks, every large destination at once
                db, ub = d[big], u[big]
                P = torch.empty(int(db.numel()), k, dtype=torch.long, device=dev)
                for i in range(k):
                    j = db - k + i
                    t = torch.minimum(torch.floor(ub[:, i] * (j + 1).double()).long(), j)
                    P[:, i] = torch.where((P[:, :i] == t[:, None]).any(1), j, t)
                pick[big] = P.sort(1).values
            keep = torch.arange(k, device=dev)[None, :] < d.clamp(max=k)[:, None]
            ldst = torch.arange(n_dst, device=dev)[:, None].expand(n_dst, k)[keep]
            pos = (r0[:, None] + pick)[keep]
        etype = self.in_type[pos].long() if self.in_type is not None else None
        return self._relabel_torch(dst_nodes, ldst, self.in_eid[pos].long(), self.in_src[pos].long(), etype)

    def _layer_rel_hip(self, dst_nodes, spec, u):
        dev, N, n_dst, R = self.device, self.N, int(dst_nodes.numel()), spec.R
        lib, st = load(), stream_of(dst_nodes)
        i64 = lambda n: torch.empty(int(n), dtype=torch.int64, device=dev)
        runs = (ptr(self.run_ptr), ptr(self.run_start), ptr(self.run_type))
        E = 0
        if n_dst:
            first = torch.empty(n_dst + 1, dtype=torch.int32, device=dev)
            nb = lib.mrg_block_rel_sizes_workspace_bytes(n_dst)
            ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
            call("mrg_block_rel_sizes", runs + (ptr(dst_nodes), n_dst, N, spec.fan_host, ptr(spec.spec), R, ptr(first), ptr(ws), nb, st))
            E = int(first[n_dst])                                             # host read 1
            if E < 0:
                raise ValueError("NeighborSampler: the block has more than 2^31 - 1 edges (are the seeds unique?)")
        eid, ldst, lsrc, etype = i64(E), i64(E), i64(E), i64(E)
        if E == 0:
            return G.Block(dst_nodes, dst_nodes, lsrc, ldst, eid, etype)
        gsrc = torch.empty(E, dtype=torch.int32, device=dev)
        src_nodes = i64(n_dst + E)
        n_new = torch.empty(1, dtype=torch.int32, device=dev)
        nb = lib.mrg_block_rel_emit_workspace_bytes(E)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        call("mrg_block_rel_emit", runs + (ptr(self.rel_eid), ptr(self.src_of), ptr(self.type_of), int(self.rel_eid.numel()), ptr(dst_nodes),
                                           ptr(first), n_dst, N, spec.fan_host, ptr(spec.spec), R, ptr(u), spec.K, E, ptr(eid), ptr(etype),
                                           ptr(ldst), ptr(gsrc), ptr(self.local), ptr(self.firstpos), ptr(ws), nb, st))
        nb = lib.mrg_block_relabel_workspace_bytes(E)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        call("mrg_block_relabel", (ptr(gsrc), ptr(dst_nodes), n_dst, N, E, ptr(self.local), ptr(self.firstpos), ptr(src_nodes), ptr(lsrc),
                                   ptr(n_new), ptr(ws), nb, st))
        src_nodes = src_nodes[: n_dst + int(n_new)]                            # host read 2
        return G.Block(src_nodes, dst_nodes, lsrc, ldst, eid, etype)

    def _layer_rel_torch(self, dst_nodes, spec, u):
        """A per-relation layer in torch ops: the runs of every destination, Floyd's picks of all cut runs at once, then the block's
        edges sorted by (destination, edge id)."""
        dev, n_dst, R = self.device, int(dst_nodes.numel()), spec.R
        if n_dst and not (0 <= int(dst_nodes.min()) and int(dst_nodes.max()) < self.N):
            raise ValueError("NeighborSampler: a seed lies outside [0, number_of_nodes())")
        ar = lambda n: torch.arange(n, device=dev)
        fan, col = spec.spec[:R].long(), spec.spec[R:].long()
        q0 = self.run_ptr[dst_nodes].long()
        nr = self.run_ptr[dst_nodes + 1].long() - q0
        n_runs = int(nr.sum())
        rdst = torch.repeat_interleave(ar(n_dst), nr, output_size=n_runs)       # the destination of every run of the layer
        q = ar(n_runs) - (torch.cumsum(nr, 0) - nr)[rdst] + q0[rdst]
        s0 = self.run_start[q].long()
        d, r = self.run_start[q + 1].long() - s0, self.run_type[q].long()
        f = fan[r]
        kept = torch.where((f < 0) | (d <= f), d, f)
        E = int(kept.sum())
        run = torch.repeat_interleave(ar(n_runs), kept, output_size=E)          # the run of every kept edge, type by type
        within = ar(E) - (torch.cumsum(kept, 0) - kept)[run]                    # kept whole: positions 0..d-1 of the run
        big = (f >= 1) & (d > f)
        if bool(big.any()):                                                     # Floyd's f picks, every cut run at once
            db, fb, row, cb = d[big], f[big], rdst[big], col[r[big]]
            P = torch.full((int(db.numel()), int(fb.max())), _I32_MAX, dtype=torch.long, device=dev)
            for i in range(P.shape[1]):
                j = db - fb + i
                ui = u[row, (cb + i).clamp(max=spec.K - 1)]
                t = torch.minimum(torch.floor(ui * (j + 1).double()).long(), j)
                P[:, i] = torch.where(i < fb, torch.where((P[:, :i] == t[:, None]).any(1), j, t), P[:, i])
            P = P.sort(1).values                                                # a run's picks ascending, then the unused columns
            slot = torch.zeros(n_runs, dtype=torch.long, device=dev)
            slot[big] = ar(int(db.numel()))
            cut = big[run]
            within[cut] = P[slot[run[cut]], within[cut]]
        eid, ldst = self.rel_eid[s0[run] + within].long(), rdst[run]
        order = torch.argsort(ldst * max(int(self.rel_eid.numel()), 1) + eid)   # edge ids ascending inside a destination, across types
        eid, ldst = eid[order], ldst[order]
        return self._relabel_torch(dst_nodes, ldst, eid, self.src_of[eid].long(), self.type_of[eid].long())

    def _relabel_torch(self, dst_nodes, ldst, eid, s, etype):
        """Local source indices and the source list of a layer's edges; touches the two tables at the block's nodes only."""
        dev, n_dst, E = self.device, int(dst_nodes.numel()), int(eid.numel())
        ar = torch.arange(E, dtype=torch.int32, device=dev)
        self.local[dst_nodes] = torch.arange(n_dst, dtype=torch.int32, device=dev)
        self.firstpos.scatter_reduce_(0, s, ar, reduce="amin")
        ls, fp = self.local[s].long(), self.firstpos[s]
        fresh = (ls < 0) & (fp == ar)
        rank = torch.cumsum(fresh, 0) - fresh.long()
        lsrc = torch.where(ls >= 0, ls, n_dst + rank[fp.long()])
        src_nodes = torch.cat((dst_nodes, s[fresh]))
        self.firstpos[s] = _I32_MAX
        self.local[dst_nodes] = -1
        return G.Block(src_nodes, dst_nodes, lsrc, ldst, eid, etype)
