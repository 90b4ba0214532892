#!/usr/bin/env python3
"""The "dot" sweeps under a per-entity score bias next to their unbiased twins, and CompGCN_ConvE's training step with loss_1n next to
its dense forward + BCE, at FB15k-237's shape (N = 14 541, D = 200, B = 1024), in one process:

  sweeps   the forward loss sweep (mrg_rows_bias_bce_fwd / mrg_distmult_bce_fwd), the logit-gradient sweep over all N columns
           (mrg_rows_bias_bce_dlogit / mrg_distmult_bce_dlogit), the filtered rank sweep (mrg_rows_bias_rank / mrg_rows_rank) and the
           filtered top-10 sweep (mrg_rows_bias_topk / mrg_rows_topk) on the same operands.  The legs of a pair alternate (plain, biased,
           plain, ...) after --warmup rounds; a leg's time is the device time between two events around the call (which includes the
           call's small kernels: list lookup, finish, target scores), reported as median and min..max over --rounds.
  chunk    one backward of functional.rows_bce_all(bias=) under the library's per-entry-point meter: the column-sum kernel
           (mrg_cols_sum) next to the chunk's logit-gradient sweep and its two gradient GEMMs.
  step     one CompGCN_ConvE training step (forward, loss, backward; dropout as constructed) with loss_1n and with forward +
           F.binary_cross_entropy on LabelIndex.labels: time as above, memory as the peak of torch.cuda.max_memory_allocated over the
           step minus the allocation before it.

Prints one JSON line per part.  Needs a HIP device: there is no fallback.

    python tools/bias_1n_bench.py [--rounds 15] [--warmup 3] [--parts sweeps,chunk,step]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import _lib, compgcn as CG, evaluation as EV, functional as K, graph as G  # noqa: E402
from mr_gnas_amd.sampler import LabelIndex  # noqa: E402

N, R, T, D, B = 14541, 237, 272115, 200, 1024
DEV = "cuda"


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def alternate(legs, rounds, warmup):
    """{name: stats} of the device time of each leg, the legs taking turns within every round."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: stats(v) for k, v in ts.items()}


def data():
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)], 1)
    li = LabelIndex(tri, R, N, DEV)
    subj, rel = torch.from_numpy(tri[:B, 0]).to(DEV), torch.from_numpy(tri[:B, 1]).to(DEV)
    gen = torch.Generator().manual_seed(0)
    ent, q = ((0.15 * torch.randn(n, D, generator=gen)).to(DEV) for n in (N, B))
    bias = (2.0 * torch.rand(N, generator=gen) - 1.0).to(DEV)
    return tri, li, subj, rel, torch.from_numpy(tri[:B, 2]).to(DEV), ent, q, bias


def part_sweeps(args, tri, li, subj, rel, obj, ent, q, bias):
    side = EV._LabelSide(li)
    when = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    qkey = (subj.long() * side.num_rels + rel.long()).contiguous()
    v0, v1 = li.label_values(0.1)
    gscale = torch.full((1,), 1.0 / (B * N), device=DEV)
    dl = torch.empty(B * N, device=DEV)
    out = {"part": "sweeps", "B": B, "N": N, "D": D, "rounds": args.rounds}
    with torch.no_grad():
        for name, fn in (("bce_fwd", lambda b: K.distmult_bce_mean(q, ent, li, qkey, v0, v1, bias=b)),
                         ("bce_dlogit", lambda b: K.distmult_bce_dlogit(q, ent, li, qkey, v0, v1, 0, N, gscale, dl, bias=b)),
                         ("rank", lambda b: EV.query_ranks(q, ent, obj, side, when, qkey, bias=b)),
                         ("topk10", lambda b: EV.query_topk(q, ent, 10, side, when, qkey, bias=b))):
            # the plain leg twice: the spread between two legs of the same code is what a difference has to exceed
            out[name] = alternate({"plain": lambda: fn(None), "biased": lambda: fn(bias), "plain_again": lambda: fn(None)},
                                  args.rounds, args.warmup)
    print(json.dumps(out), flush=True)


def part_chunk(args, tri, li, subj, rel, obj, ent, q, bias):
    names = ["mrg_cols_sum", "mrg_rows_bias_bce_dlogit", "mrg_linear_fwd", "mrg_linear_bwd_input", "mrg_linear_bwd_weight",
             "mrg_rows_bias_bce_fwd"]
    rec = {}
    for i in range(args.warmup + args.rounds):
        e, s, b = (t.detach().clone().requires_grad_(True) for t in (ent, q, bias))
        _lib.meter.start(names)
        K.rows_bce_all("dot", None, e, s, li, subj, rel, 0.1, bias=b).backward()
        got = _lib.meter.stop()
        if i >= args.warmup:
            for k, v in got.items():
                rec.setdefault(k, []).append((v["ms"], v["launches"]))
    out = {"part": "chunk", "B": B, "N": N, "D": D, "col_chunk": min(K.bce_default_col_chunk(B), N),
           "entry_ms_per_step": {k: dict(stats([m for m, _ in v]), launches=v[0][1]) for k, v in rec.items()}}
    print(json.dumps(out), flush=True)


def part_step(args, tri, li, subj, rel, obj, ent, q, bias):
    g = G.build_train_graph(N, R, tri).to(DEV)
    E = g.num_edges()
    m = torch.zeros(E, dtype=torch.bool, device=DEV)
    m[: E // 2] = True
    key = "e_type" if "e_type" in g.edata else "etype"
    g.edata["etype"], g.edata["in_edges_mask"], g.edata["out_edges_mask"] = g.edata[key], m, ~m
    torch.manual_seed(0)
    net = CG.CompGCN_ConvE(-1, 2 * R, N, 100, [D], comp_fn="sub", num_filt=200, ker_sz=7, k_w=10, k_h=20).to(DEV).train()

    def step(fused):
        net.zero_grad(set_to_none=True)
        if fused:
            loss = net.loss_1n(g, subj, rel, li, 0.1)
        else:
            loss = F.binary_cross_entropy(net(g, subj, rel), li.labels(subj, rel, 0.1))
        loss.backward()
        return loss

    legs = {"dense": lambda: step(False), "loss_1n": lambda: step(True), "dense_again": lambda: step(False)}
    out = {"part": "step", "B": B, "N": N, "D": D, "E": int(E), "rounds": args.rounds, "time": alternate(legs, args.rounds, args.warmup)}
    mem = {}
    for k, fn in legs.items():
        net.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn()
        torch.cuda.synchronize()
        mem[k] = {"peak_mib": round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1), "loss": round(float(loss.detach()), 6)}
    out["memory"], out["batch_by_entity_mib"] = mem, round(B * N * 4 / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="sweeps,chunk,step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bias_1n_bench needs a HIP device")
    d = data()
    for part in args.parts.split(","):
        {"sweeps": part_sweeps, "chunk": part_chunk, "step": part_step}[part](args, *d)


if __name__ == "__main__":
    main()
