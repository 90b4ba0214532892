#!/usr/bin/env python3
"""Time one forward + backward of the node-classification search supernet (model_search_nc.Network) on a synthetic block pair, with
the candidate Linears of every MixedOp as one grouped launch (functional.switches.CAND_LINEAR_GROUP, the default) and as one row-GEMM
launch per candidate (the switch off: the kernels the library had before ABI 22) -- in the same process, in alternating rounds, with
HIP events, after warm-up.

    python tools/nc_search_bench.py [--edges 200000 --edges2 20000 --dim 64 --layers 2 --rounds 30 --warmup 5]

Prints one JSON line: per setting the median and the p10 / p90 of the step time, the launch counts of the entry points the switch
moves, and for the grouped forward its summed device time against its algorithmic traffic 4 * rows * D * 2n + 4 * n * D^2 bytes
(achieved bytes/s; the partial column sums it also writes are not counted), over all its launches and over those on the large block alone.  Needs a HIP device: there is no CPU form of a timing.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import _lib, graph as G, model_search_nc as MS      # noqa: E402
from mr_gnas_amd.functional import switches as SW                    # noqa: E402

MOVED = ["mrg_cand_linear_fwd", "mrg_cand_linear_bwd_input", "mrg_linear_fwd", "mrg_linear_bwd_input", "mrg_linear_bwd_weight",
         "mrg_mix_stats_coef"]


def synthetic_blocks(edges, edges2, n_nodes, n_rel, gen, dev):
    """Two blocks: `edges` edge rows into ~edges / 10 destinations, whose outputs feed `edges2` edge rows into ~edges2 / 10 seeds.
    Block 0's destination nodes are block 1's source nodes, in order (the sampler's convention)."""
    n_dst1 = max(2, edges2 // 10)
    n_src1 = max(n_dst1, edges // 10)                       # = block 0's destinations
    n_src0 = n_src1 + n_nodes // 2

    def block(n_src, n_dst, E, eid0):
        dst, _ = torch.sort(torch.randint(0, n_dst, (E,), generator=gen))
        src = torch.randint(0, n_src, (E,), generator=gen)
        etype = torch.randint(0, n_rel, (E,), generator=gen)
        return G.Block(torch.arange(n_src), torch.arange(n_dst), src, dst, torch.arange(eid0, eid0 + E), etype)

    b0, b1 = block(n_src0, n_src1, edges, 0), block(n_src1, n_dst1, edges2, edges)
    T = edges + edges2
    trip = torch.stack([torch.arange(T), torch.randint(0, n_nodes, (T,), generator=gen), torch.randint(0, n_nodes, (T,), generator=gen)], 1)
    return [b0.to(dev), b1.to(dev)], trip.to(dev), n_dst1


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=200000)
    ap.add_argument("--edges2", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nc_search_bench needs a HIP device")
    if a.layers != 2:
        raise SystemExit("the synthetic block pair serves two layers")
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    n_nodes, n_rel, classes = 50000, 20, 8
    blocks, trip, n_seeds = synthetic_blocks(a.edges, a.edges2, n_nodes, n_rel, gen, dev)
    for b in blocks:
        b.plan()["n_chunks"]
    net = MS.Network(torch.device(dev), n_nodes, classes, n_rel, a.layers, 1, a.nodes, a.dim, 32, 10).to(dev).train()
    labels = torch.randint(0, classes, (n_seeds,), generator=gen).to(dev)

    def step():
        for p in net.parameters():
            p.grad = None
        for al in net.arch_parameters():
            al.grad = None
        loss = net._criterion(net(trip, blocks), labels)
        loss.backward()
        return loss

    def timed(on):
        SW.CAND_LINEAR_GROUP = on
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        step()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    for _ in range(a.warmup):
        timed(True), timed(False)
    times = {True: [], False: []}
    for r in range(a.rounds):                                # alternating rounds: drift of the machine hits both settings alike
        for on in ((True, False) if r % 2 == 0 else (False, True)):
            times[on].append(timed(on))
    out = {"edges": [a.edges, a.edges2], "dim": a.dim, "layers": a.layers, "nodes": a.nodes, "rounds": a.rounds}
    losses = {}
    for on, tag in ((True, "grouped"), (False, "per_member")):
        SW.CAND_LINEAR_GROUP = on
        _lib.meter.start(MOVED)
        losses[tag] = float(step())
        torch.cuda.synchronize()
        per_launch = [(ev0.elapsed_time(ev1), nb) for ev0, ev1, nb, _ in _lib.meter.records.get("mrg_cand_linear_fwd", [])]
        rec = _lib.meter.stop()
        out[tag] = {"ms_median": round(pct(times[on], 0.5), 4), "ms_p10": round(pct(times[on], 0.1), 4), "ms_p90": round(pct(times[on], 0.9), 4),
                    "launches": {k: v["launches"] for k, v in sorted(rec.items())},
                    "kernel_ms": {k: round(v["ms"], 4) for k, v in sorted(rec.items())}}
        if on:
            f = rec["mrg_cand_linear_fwd"]
            out[tag]["cand_linear_fwd_bytes"] = f["bytes"]
            out[tag]["cand_linear_fwd_TBps"] = round(f["bytes"] / (f["ms"] * 1e-3) / 1e12, 3)
            # the launches on the large block alone (the sum above is mostly launch gaps of the few-row launches)
            big = max(nb for _, nb in per_launch)
            ms_big = [ms for ms, nb in per_launch if nb == big]
            out[tag]["cand_linear_fwd_largest"] = {"launches": len(ms_big), "bytes_each": big, "ms_median": round(pct(ms_big, 0.5), 4),
                                                   "TBps": round(big / (pct(ms_big, 0.5) * 1e-3) / 1e12, 3)}
    SW.CAND_LINEAR_GROUP = True
    out["loss"] = losses                                     # the two settings compute the same step within rounding
    print(json.dumps(out))


if __name__ == "__main__":
    main()
