#!/usr/bin/env python3
"""Top-k link prediction -- "which k objects complete (s, r, ?)" for a batch of queries -- two ways, in one process:

  dense  the scorer's forward ([B, N] probabilities: functional.distmult_scores_all / transe_scores_all) -> torch.topk; the filtered
         form first overwrites the known objects (LabelIndex.labels, a second [B, N] tensor) with -1
  fused  no [B, N] tensor: evaluation.query_topk on the query rows (--kind dot: mrg_rows_topk, csrc/topk.hip; --kind l1: mrg_transe_topk,
         csrc/transe_1n.hip) -> sigmoid of the k values

at FB15k-237's shape (N = 14 541, B = 256, D = 64 and 200) and at the project's largest configuration (N = 1 000 000, B = 256,
D = 256), k = 10 (--k).  The legs alternate (dense, fused, dense filtered, fused filtered, dense, ...) after --warmup rounds each; a
leg's time is the device time between two events around it, reported as median and min..max; its memory is the peak of
torch.cuda.max_memory_allocated over the leg minus the allocation before it.  "agree": the fraction of (query, position) pairs at which
the fused and the dense list of the last round name the same entity (the dense path ranks float32 sigmoids, which tie where the
logits differ, and torch.topk leaves ties in unspecified order).  After the timed rounds every fused leg runs once more under the
library's per-entry-point meter.  Prints one JSON line per shape.  Needs a HIP device: there is no fallback.

    python tools/topk_bench.py [--kind dot|l1] [--k 10] [--rounds 7] [--warmup 2] [--shapes fb64,fb200,c5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import _lib, evaluation as EV, functional as K  # noqa: E402
from mr_gnas_amd.sampler import LabelIndex  # noqa: E402

SHAPES = {"fb64": (14541, 237, 256, 64, 272115), "fb200": (14541, 237, 256, 200, 272115), "c5": (1_000_000, 64, 256, 256, 4_000_000)}


def leg(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ids, prob = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - before, ids


def spread(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--shapes", default="fb64,fb200,c5")
    ap.add_argument("--kind", default="dot", choices=("dot", "l1"))
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("topk_bench: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs a HIP device")
    dev, k = "cuda", args.k
    for name in args.shapes.split(","):
        N, R, B, D, T = SHAPES[name]
        g = torch.Generator().manual_seed(0)
        tri = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, R, (T,), generator=g), torch.randint(0, N, (T,), generator=g)), 1)
        index = LabelIndex(tri.to(dev), R, N, dev)
        subj, rel = tri[:B, 0].to(dev), tri[:B, 1].to(dev)
        scale = 0.3 if D <= 64 else 0.15
        ent, sub, relb = ((scale * torch.randn(n, D, generator=g)).to(dev) for n in (N, B, B))
        side = EV._LabelSide(index)
        when = torch.full((B,), -1, dtype=torch.int32, device=dev)
        qkey = (subj.long() * side.num_rels + rel.long()).contiguous()
        extra = {}
        with torch.no_grad():
            if args.kind == "dot":
                score = lambda: K.distmult_scores_all(ent, sub, relb)
                query, prob_of = (lambda: sub * relb), torch.sigmoid
            else:
                gamma = float(torch.round(((sub + relb).unsqueeze(1) - ent[:1024].unsqueeze(0)).abs().sum(-1).median()))
                extra = {"gamma": gamma}
                score = lambda: K.transe_scores_all(ent, sub, relb, gamma)
                query, prob_of = (lambda: sub + relb), (lambda d: torch.sigmoid(gamma - d))

            def dense(filtered):
                p = score()
                if filtered:
                    p = p.masked_fill(index.labels(subj, rel, 0.0) > 0, -1.0)
                v, i = torch.topk(p, k, dim=1)
                return i, v

            def fused(filtered):
                ids, vals = EV.query_topk(query(), ent, k, *((side, when, qkey) if filtered else ()), kind=args.kind)
                return ids, prob_of(vals)

            legs = {"dense_raw": lambda: dense(False), "fused_raw": lambda: fused(False),
                    "dense_filtered": lambda: dense(True), "fused_filtered": lambda: fused(True)}
            times, peaks, last = {n: [] for n in legs}, {n: 0 for n in legs}, {}
            for rnd in range(args.warmup + args.rounds):
                for n, fn in legs.items():                      # alternating: one leg of each kind per round
                    ms, peak, ids = leg(fn)
                    if rnd >= args.warmup:
                        times[n].append(ms)
                        peaks[n] = max(peaks[n], peak)
                        last[n] = ids
            entry_ms = {}
            for n in ("fused_raw", "fused_filtered"):           # one more round per fused leg under the per-entry-point meter
                _lib.meter.start()
                leg(legs[n])
                entry_ms[n] = {s: round(r["ms"], 4) for s, r in sorted(_lib.meter.stop().items())}
            agree = {w: float((last["fused_" + w] == last["dense_" + w]).float().mean()) for w in ("raw", "filtered")}
        print(json.dumps({"shape": {"name": name, "kind": args.kind, "N": N, "B": B, "D": D, "k": k, "matrix_MiB": B * N * 4 / 2 ** 20, **extra},
                          "agree": agree,
                          "legs": {n: {**spread(times[n]), "peak_MiB": peaks[n] / 2 ** 20, **({"entry_ms": entry_ms[n]} if n in entry_ms else {})}
                                   for n in legs}}), flush=True)
        del index, side, ent, sub, relb, legs, last
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
