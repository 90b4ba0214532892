#!/usr/bin/env python3
"""Generate the node-classification fixtures under tests/golden/ by RUNNING THE REFERENCE (see make_golden.py for the stand-ins and
the rules).

    python tests/golden/make_golden_nc.py

The reference's ``models/operations.py`` and ``models/model.py`` run as they are.  What DGL would supply is stood in below, on top
of make_golden.py's stand-in package, following DGL's documented conventions (unpinned against real DGL, as the other DGL semantics):
  * blocks: ``srcdata`` / ``dstdata`` frames with the global node ids under ``dgl.NID``, ``ndata`` = ``dstdata``,
    ``edata[dgl.EID]`` (global edge ids) and ``edata[dgl.ETYPE]``;
  * UDF reducers: ``update_all(fn.copy_edge, reduce_fn)`` calls ``reduce_fn`` once per in-degree bucket with a mailbox
    [n, deg, D] whose messages are in edge-id order; destinations without in-edges get zero rows;
  * the full-neighbour block builder of ``MultiLayerFullNeighborSampler(layers, return_eids=True)``: the last block's destination
    nodes are the seeds in order; block j's destination nodes are block j + 1's source nodes; a block's source nodes are its
    destination nodes, then new sources in order of first appearance over its edges; edges grouped by destination in destination
    order, edge ids ascending within a destination.

Cases:
  nc_ops_small        every MIXED_OPS entry forward + backward on one block with a hub of >= 2 048 in-edges, destinations without
                      in-edges and of in-degree 1, duplicate edges, and a destination whose messages are equal in column 0
  nc_fixednet_small   models.model.Network with the training driver's default two-cell genotype, two layers, op_norm off (case n0)
                      and on (case n1): one training step (cross-entropy on random labels, backward), then one eval-mode forward
  (in nc_fixednet_small, case s1) a small genotype with a_std, op_norm on
"""
import collections
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins, npify  # noqa: E402

EID = NID = "_ID"
ETYPE = "_TYPE"
Genotype = collections.namedtuple("Genotype", "alpha_cell concat_node score_func", defaults=(None,))

TRAIN_GENOTYPE = ("[Genotype(alpha_cell=[('pre_sub', 1, 0), ('f_dense', 2, 1), ('f_sparse', 3, 2), ('f_identity', 4, 3), ('a_sum', 5, 2), "
                  "('a_sum', 6, 3), ('a_mean', 7, 4), ('f_dense_last', 8, 7), ('f_sparse_last', 9, 7), ('f_sparse_last', 10, 5)], "
                  "concat_node=[5, 6, 7, 8, 9, 10]), Genotype(alpha_cell=[('pre_sub', 1, 0), ('f_sparse', 2, 1), ('f_identity', 3, 2), "
                  "('f_identity', 4, 1), ('a_max', 5, 2), ('a_mean', 6, 3), ('a_mean', 7, 4), ('f_sparse_last', 8, 7), "
                  "('f_sparse_last', 9, 8), ('f_identity', 10, 9)], concat_node=[5, 6, 7, 8, 9, 10])]")
STD_GENOTYPE = ("[Genotype(alpha_cell=[('pre_add', 1, 0), ('f_dense', 2, 1), ('a_std', 3, 2), ('a_max', 4, 1), ('f_sparse_last', 5, 3)], "
                "concat_node=[3, 4, 5])] * 2")


class _NodeBatch:
    def __init__(self, mailbox):
        self.mailbox = mailbox


class FakeBlock:
    """The slice of DGL's block protocol that models/operations.py and models/model.py touch."""

    def __init__(self, src_nodes, dst_nodes, src, dst, eid, etype):
        self._src, self._dst = src, dst
        self.srcdata = {NID: src_nodes}
        self.dstdata = {NID: dst_nodes}
        self.ndata = self.dstdata
        self.edata = {EID: eid, ETYPE: etype}

    def number_of_dst_nodes(self):
        return int(self.dstdata[NID].numel())

    def update_all(self, msg, reduce_fn):
        _, ef, mname = msg
        m = self.edata[ef]
        n, D = self.number_of_dst_nodes(), m.shape[1]
        deg = torch.bincount(self._dst, minlength=n)
        h = torch.zeros(n, D, dtype=m.dtype)
        for d in sorted(set(deg.tolist()) - {0}):
            nodes = torch.nonzero(deg == d).view(-1)
            # the in-edges of every node of the bucket, edge ids ascending
            rows = torch.stack([torch.nonzero(self._dst == v).view(-1) for v in nodes.tolist()])
            out = reduce_fn(_NodeBatch({mname: m[rows]}))
            (key, val), = out.items()
            h = h.index_copy(0, nodes, val)
        self.dstdata[key] = h


def full_neighbor_blocks(src, dst, etype, seeds, layers):
    """Explicit loops over the conventions in the module docstring."""
    blocks = []
    dst_nodes = [int(v) for v in seeds]
    for _ in range(layers):
        eids = [e for v in dst_nodes for e in range(len(dst)) if dst[e] == v]
        local = {v: i for i, v in enumerate(dst_nodes)}
        src_nodes = list(dst_nodes)
        for e in eids:
            if int(src[e]) not in local:
                local[int(src[e])] = len(src_nodes)
                src_nodes.append(int(src[e]))
        lsrc = [local[int(src[e])] for e in eids]
        ldst = [dst_nodes.index(int(dst[e])) for e in eids]
        t = lambda a: torch.tensor(a, dtype=torch.long)
        blocks.append(FakeBlock(t(src_nodes), t(dst_nodes), t(lsrc), t(ldst), t(eids), torch.as_tensor(etype)[t(eids)]))
        dst_nodes = src_nodes
    return blocks[::-1]


def _install_nc_standins():
    _install_standins()
    dgl = sys.modules["dgl"]
    dgl.EID, dgl.NID, dgl.ETYPE = EID, NID, ETYPE
    import configs.genotypes as CG
    CG.Genotype = Genotype           # the NC genotypes carry no score_func


def _store_blocks(st, prefix, blocks):
    st[f"{prefix}/n_blocks"] = np.array(len(blocks))
    for j, b in enumerate(blocks):
        st[f"{prefix}/block{j}/src"], st[f"{prefix}/block{j}/dst"] = b._src, b._dst
        st[f"{prefix}/block{j}/eid"], st[f"{prefix}/block{j}/etype"] = b.edata[EID], b.edata[ETYPE]
        st[f"{prefix}/block{j}/src_nid"], st[f"{prefix}/block{j}/dst_nid"] = b.srcdata[NID], b.dstdata[NID]


def ops_graph(rng):
    """Graph of nc_ops_small: seeds 0..29; node 0 a hub of 2 048 in-edges, nodes 1..5 in-degree 1, node 6 in-degree 4 (its messages
    are made equal in column 0), nodes 7..25 in-degree 1..5 with one duplicated edge, nodes 26..29 without in-edges; more edges
    into non-seed nodes; the edge list shuffled."""
    N = 120
    s, d = [], []
    add = lambda u, v: (s.append(int(u)), d.append(int(v)))
    for u in rng.integers(0, N, 2048):
        add(u, 0)
    for v in range(1, 6):
        add(rng.integers(0, N), v)
    for u in rng.integers(0, N, 4):
        add(u, 6)
    for v in range(7, 26):
        for u in rng.integers(0, N, rng.integers(1, 6)):
            add(u, v)
    add(40, 9); add(40, 9)                                           # a duplicated edge
    for u, v in zip(rng.integers(0, N, 200), rng.integers(30, N, 200)):
        add(u, v)
    perm = rng.permutation(len(s))
    src, dst = np.asarray(s)[perm], np.asarray(d)[perm]
    etype = rng.integers(0, 7, len(src))
    return N, src, dst, etype


def case_ops(D=4, seed=5):
    import models.operations as OP
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    N, src, dst, etype = ops_graph(rng)
    seeds = np.arange(30)
    (blk,) = full_neighbor_blocks(src, dst, etype, seeds, 1)
    E, n_dst = blk._src.numel(), blk.number_of_dst_nodes()
    st = {"N": np.array(N), "D": np.array(D), "gsrc": src, "gdst": dst, "getype": etype, "seeds": seeds, "layers": np.array(1)}
    _store_blocks(st, "blocks", [blk])
    x = torch.randn(E, D, generator=gen)
    x[blk._dst == 6, 0] = 0.5                                        # node 6: equal messages in column 0
    y = torch.randn(E, D, generator=gen)
    xd = torch.randn(n_dst, D, generator=gen)
    ge, gd = torch.randn(E, D, generator=gen), torch.randn(n_dst, D, generator=gen)
    st.update({"x": x, "y": y, "xd": xd, "ge": ge, "gd": gd})
    contract = {"MIXED_OPS": list(OP.MIXED_OPS), "PRE_OPS": OP.PRE_OPS, "FIRST_OPS": OP.FIRST_OPS, "MIDDLE_OPS": OP.MIDDLE_OPS,
                "LAST_OPS": OP.LAST_OPS, "classes": {}, "params": {}}
    for name, ctor in OP.MIXED_OPS.items():
        op = ctor({"feature_dim": D})
        contract["classes"][name] = type(op).__name__
        contract["params"][name] = [[n, list(p.shape)] for n, p in op.named_parameters()]
        for n, p in op.named_parameters():                           # biases away from 0 so their gradients are exercised
            if p.dim() == 1:
                with torch.no_grad():
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
        last = name in ("f_dense_last", "f_sparse_last")
        agg = name.startswith("a_")
        a = (xd if last else x).clone().requires_grad_(True)
        b = y.clone().requires_grad_(True)
        out = op(blk, a, b)
        out.backward(gd if (last or agg) else ge)
        st[f"{name}/out"] = out
        st[f"{name}/ga"] = a.grad if a.grad is not None else torch.zeros_like(a)
        if b.grad is not None:
            st[f"{name}/gb"] = b.grad
        for n, p in op.named_parameters():
            st[f"{name}/param/{n}"] = p
            st[f"{name}/gparam/{n}"] = p.grad
    st["contract"] = np.array(json.dumps(contract))
    np.savez_compressed(os.path.join(OUT, "nc_ops_small.npz"), **npify(st))
    print(f"wrote nc_ops_small: E={E} n_dst={n_dst} hub in-degree={int((blk._dst == 0).sum())}")


def fixed_net_case(st, tag, genotype_str, op_norm, seed, N=160, T=700, R=6, classes=4, D=16, D0=8, nbase=5, batch=12, layers=2):
    import models.model as MM
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    src, dst = rng.integers(0, N, T), rng.integers(0, N, T)
    src[:3], dst[:3] = 5, 7                                          # a duplicated edge
    etype = rng.integers(0, R, T)
    trip_index = torch.stack([torch.arange(T), torch.as_tensor(src), torch.as_tensor(dst)], dim=1)
    seeds = rng.choice(N, batch, replace=False)
    blocks = full_neighbor_blocks(src, dst, etype, seeds, layers)
    genotype = eval(genotype_str)
    args = types.SimpleNamespace(feature_dim=D, op_norm=op_norm)
    net = MM.Network(torch.device("cpu"), genotype, N, classes, R, layers, 1, 3, D, D0, nbase, torch.nn.CrossEntropyLoss(), args)
    for n, p in net.named_parameters():                              # BatchNorm gains / biases away from 1 / 0
        if p.dim() == 1:
            with torch.no_grad():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1 + (1.0 if n.endswith("weight") and "batchnorm" in n else 0.0))
    labels = torch.as_tensor(rng.integers(0, classes, N))
    st.update({f"{tag}/args": np.array([N, T, R, classes, D, D0, nbase, batch, layers, int(op_norm)]), f"{tag}/genotype": np.array(genotype_str),
               f"{tag}/gsrc": src, f"{tag}/gdst": dst, f"{tag}/getype": etype, f"{tag}/seeds": seeds, f"{tag}/trip_index": trip_index,
               f"{tag}/labels": labels, f"{tag}/state_keys": np.array(json.dumps(list(net.state_dict().keys())))})
    _store_blocks(st, f"{tag}/blocks", blocks)
    for n, p in net.state_dict().items():
        st[f"{tag}/param0/{n}"] = p.clone()
    net.train()
    logits = net(trip_index, blocks)                                 # the training driver's step (train/mr_nc_train.py:155-160)
    loss = net._criterion(logits, labels[torch.as_tensor(seeds)])
    loss.backward()
    st.update({f"{tag}/logits": logits, f"{tag}/loss": loss})
    for n, p in net.named_parameters():
        if p.grad is not None:
            st[f"{tag}/gparam/{n}"] = p.grad
    for n, b in net.named_buffers():
        st[f"{tag}/buffer/{n}"] = b
    net.eval()
    with torch.no_grad():
        st[f"{tag}/logits_eval"] = net(trip_index, blocks)
    print(f"  {tag}: E per block {[int(b._src.numel()) for b in blocks]} loss={float(loss):.6f}")


def case_fixed_net():
    st = {}
    fixed_net_case(st, "n0", TRAIN_GENOTYPE, False, 31)
    fixed_net_case(st, "n1", TRAIN_GENOTYPE, True, 32)
    fixed_net_case(st, "s1", STD_GENOTYPE, True, 33)
    np.savez_compressed(os.path.join(OUT, "nc_fixednet_small.npz"), **npify(st))
    print("wrote nc_fixednet_small")


def main():
    _install_nc_standins()
    case_ops()
    case_fixed_net()


if __name__ == "__main__":
    main()
