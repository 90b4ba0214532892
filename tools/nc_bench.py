#!/usr/bin/env python3
"""Node-classification timings on the GPU:

  a_std        forward and backward of a_std on HIP (csrc/segstd.hip) against a torch restatement (index_add of x and x^2, autograd)
               and against the no-self a_mean reduction (functional.seg_reduce, span kernel) on the same block; three blocks: cache
               resident (E 200 k, D 64), beyond the caches (E 4 M, D 64: 1 GB of messages) and D 200 (E 2 M).  Bandwidth of the
               forward from its algorithmic bytes 4 E D + 8 n_dst D, against the ~6.3 TB/s achievable HBM rate.
  train_step   one node-classification training step (model_nc.Network, the training driver's default two-cell genotype, batch 64,
               D 64, init 16, 50 bases, 2 layers, SGD with momentum): forward, backward and the optimizer step on blocks already
               built, and the block build (sampler.full_neighbor_blocks) on its own; synthetic graphs of the size of AIFB (8 285
               entities, 29 043 triples, 45 relations, 4 classes) and AM (1 666 764 entities, 5 988 321 triples, 133 relations, 11
               classes), built with synth.py.  A new batch of seeds every repeat (its blocks are built outside the step's timing).
               Next to it the same step on blocks of sampler.NeighborSampler with fan-outs [4, 4], and the block-build leg
               (DESIGN.md section 9.9): full_neighbor_blocks against NeighborSampler with [None, None] and with [4, 4], the three
               builders alternating on the same seeds in one process.  With them the per-relation sampler,
               NeighborSampler with [1] * R per layer: its build in the same alternation, the step on its blocks, and per builder
               the number of distinct edge types that reach the seeds' block.

HIP events, a warm-up, the median of the repeats.  Prints one JSON line at the end.
Usage on the GPU box:  python tools/nc_bench.py [--reps 20] [--only a_std|train_step]"""
import argparse
import collections
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import graph as G, model_nc as MN, sampler as SM, synth  # noqa: E402
from mr_gnas_amd import functional as K  # noqa: E402

HBM_TBPS = 6.3
STD_SHAPES = {"cache_e200k_d64": (200_000, 20_000, 64), "hbm_e4m_d64": (4_000_000, 262_144, 64), "hbm_e2m_d200": (2_000_000, 131_072, 200)}
GRAPHS = {"aifb": (8_285, 45, 29_043, 4), "am": (1_666_764, 133, 5_988_321, 11)}
Genotype = collections.namedtuple("Genotype", "alpha_cell concat_node score_func", defaults=(None,))
DEFAULT_GENOTYPE = [
    Genotype([('pre_sub', 1, 0), ('f_dense', 2, 1), ('f_sparse', 3, 2), ('f_identity', 4, 3), ('a_sum', 5, 2), ('a_sum', 6, 3),
              ('a_mean', 7, 4), ('f_dense_last', 8, 7), ('f_sparse_last', 9, 7), ('f_sparse_last', 10, 5)], [5, 6, 7, 8, 9, 10]),
    Genotype([('pre_sub', 1, 0), ('f_sparse', 2, 1), ('f_identity', 3, 2), ('f_identity', 4, 1), ('a_max', 5, 2), ('a_mean', 6, 3),
              ('a_mean', 7, 4), ('f_sparse_last', 8, 7), ('f_sparse_last', 9, 8), ('f_identity', 10, 9)], [5, 6, 7, 8, 9, 10]),
]


def timeit(fn, reps, warm=3, before=None):
    for _ in range(warm):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def bench_std(reps):
    out = {}
    for name, (E, n_dst, D) in STD_SHAPES.items():
        gen = torch.Generator(device="cuda").manual_seed(1)
        dst = torch.randint(0, n_dst, (E,), device="cuda", generator=gen)
        dst[: E // 100] = 0                                        # one hub of 1 % of the edges
        blk = G.Block(torch.arange(n_dst, device="cuda"), torch.arange(n_dst, device="cuda"), torch.randint(0, n_dst, (E,), device="cuda",
                      generator=gen), dst, torch.arange(E, device="cuda"))
        x = torch.randn(E, D, device="cuda", generator=gen).requires_grad_(True)
        g = torch.randn(n_dst, D, device="cuda", generator=gen)
        d1 = blk.in_degrees().clamp(min=1).float().view(-1, 1)

        def torch_std(x):
            s = torch.zeros(n_dst, D, device="cuda").index_add_(0, dst, x)
            q = torch.zeros(n_dst, D, device="cuda").index_add_(0, dst, x * x)
            m = s / d1
            return torch.sqrt(torch.relu(q / d1 - m * m) + 1e-5) * (d1 > 0)

        forms = {"hip": lambda x: K.aggregate_std(x, blk), "torch": torch_std, "a_mean_noself": lambda x: K.seg_reduce("mean", x, None, blk)}
        res = {}
        for form, f in forms.items():
            with torch.no_grad():
                fwd = timeit(lambda: f(x), reps)
            y = f(x)
            bwd = timeit(lambda: torch.autograd.grad(y, x, g, retain_graph=True), reps)
            res[form] = {"fwd_ms": round(fwd, 4), "bwd_ms": round(bwd, 4)}
            del y
        nb = 4 * E * D + 8 * n_dst * D
        res["hip"]["fwd_TBps"] = round(nb / (res["hip"]["fwd_ms"] * 1e-3) / 1e12, 3)
        res["hip"]["fwd_frac_of_6.3TBps"] = round(res["hip"]["fwd_TBps"] / HBM_TBPS, 3)
        res["hip_fwd_vs_a_mean"] = round(res["hip"]["fwd_ms"] / res["a_mean_noself"]["fwd_ms"], 3)
        res["shape"] = {"E": E, "n_dst": n_dst, "D": D, "fwd_bytes": nb}
        out[name] = res
        print(name, json.dumps(res), flush=True)
        del x, g, blk
        torch.cuda.empty_cache()
    return out


def bench_train(reps):
    out = {}
    for name, (N, R, T, C) in GRAPHS.items():
        tri = torch.from_numpy(synth.synth_kg(N, R, T, seed=3)).cuda()
        g = G.RelGraph(N, tri[:, 0], tri[:, 2], device="cuda")
        g.edata[G.ETYPE] = tri[:, 1].contiguous()
        trip_index = torch.stack((torch.arange(T, device="cuda"), tri[:, 0], tri[:, 2]), dim=1)
        labels = torch.randint(0, C, (N,), device="cuda")
        args = types.SimpleNamespace(feature_dim=64, op_norm=False)
        torch.manual_seed(0)
        net = MN.Network(torch.device("cuda"), DEFAULT_GENOTYPE, N, C, R, 2, 1, 3, 64, 16, 50, torch.nn.CrossEntropyLoss(), args).cuda()
        opt = torch.optim.SGD(net.parameters(), lr=0.0005, momentum=0.9)
        gen = torch.Generator().manual_seed(5)
        batches = [torch.randperm(N, generator=gen)[:64].cuda() for _ in range(reps + 3)]
        state = {"i": 0}
        edges = []

        def build():
            seeds = batches[state["i"] % len(batches)]
            state["i"] += 1
            state["blocks"] = SM.full_neighbor_blocks(g, seeds, 2)
            state["seeds"] = seeds
            edges.append([b.num_edges() for b in state["blocks"]])

        def step():
            opt.zero_grad(set_to_none=True)
            loss = net._loss(trip_index, state["blocks"], labels, state["seeds"])
            loss.backward()
            opt.step()

        t_step = timeit(step, reps, before=build)
        state["i"] = 0
        t_blocks = timeit(build, reps)
        e = np.array(edges[3:reps + 3])
        res = {"step_ms": round(t_step, 3), "blocks_ms": round(t_blocks, 3), "edges_per_block_median": [int(v) for v in np.median(e, 0)],
               "graph": {"N": N, "T": T, "R": R, "classes": C}}

        # the same step on sampled blocks, fan-outs [4, 4]
        sampled = SM.NeighborSampler(g, [4, 4])
        gen44 = torch.Generator(device="cuda").manual_seed(9)
        edges44 = []

        def build44():
            seeds = batches[state["i"] % len(batches)]
            state["i"] += 1
            state["blocks"] = sampled.sample(seeds, generator=gen44)
            state["seeds"] = seeds
            edges44.append([b.num_edges() for b in state["blocks"]])

        state["i"] = 0
        res["step_4_4_ms"] = round(timeit(step, reps, before=build44), 3)
        res["edges_per_block_4_4_median"] = [int(v) for v in np.median(np.array(edges44[3:reps + 3]), 0)]

        # the same step on per-relation blocks, one in-edge of every type per destination
        per_rel = SM.NeighborSampler(g, [1, 1], num_etypes=R, per_relation=True)
        edges_rel = []

        def build_rel():
            seeds = batches[state["i"] % len(batches)]
            state["i"] += 1
            state["blocks"] = per_rel.sample(seeds, generator=gen44)
            state["seeds"] = seeds
            edges_rel.append([b.num_edges() for b in state["blocks"]])

        state["i"] = 0
        res["step_rel_1_ms"] = round(timeit(step, reps, before=build_rel), 3)
        res["edges_per_block_rel_1_median"] = [int(v) for v in np.median(np.array(edges_rel[3:reps + 3]), 0)]

        # the block-build leg: the four builders alternate on the same seeds; next to the time, how many distinct edge types reach the
        # seeds' block (counted outside the timing)
        full = SM.NeighborSampler(g, [None, None])
        builders = {"full_neighbor_blocks": lambda sd: SM.full_neighbor_blocks(g, sd, 2), "sampler_none_none": full.sample,
                    "sampler_4_4": lambda sd: sampled.sample(sd, generator=gen44), "sampler_rel_1": lambda sd: per_rel.sample(sd, generator=gen44)}
        times, reached = {k: [] for k in builders}, {k: [] for k in builders}
        for r in range(reps + 3):
            for k, f in builders.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                blocks = f(batches[r])
                b.record()
                torch.cuda.synchronize()
                if r >= 3:
                    times[k].append(a.elapsed_time(b))
                    reached[k].append(int(blocks[-1].edata[G.ETYPE].unique().numel()))
        res["blocks_build_ms"] = {k: round(float(np.median(v)), 3) for k, v in times.items()}
        res["blocks_build_quartiles_ms"] = {k: [round(float(q), 3) for q in np.percentile(v, [25, 75])] for k, v in times.items()}
        res["seed_block_edge_types_median"] = {k: int(np.median(v)) for k, v in reached.items()}
        out[name] = res
        print(name, json.dumps(res), flush=True)
        del net, opt, g, tri, trip_index
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["a_std", "train_step"])
    a = ap.parse_args()
    res = {}
    if a.only in (None, "a_std"):
        res["a_std"] = bench_std(a.reps)
    if a.only in (None, "train_step"):
        res["train_step"] = bench_train(a.reps)
    print(json.dumps({"nc_bench": res, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
