#!/usr/bin/env python3
"""The fixed-genotype driver's 1-N loss alone -- forward plus backward down to the gradients of the entity table, the subject rows and
the relation rows -- two ways, in one process:

  dense  LabelIndex.labels ([B, N] targets) -> distmult_scores_all ([B, N] probabilities) -> F.binary_cross_entropy
  fused  functional.distmult_bce_all: mrg_distmult_bce_fwd / mrg_distmult_bce_dlogit (csrc/bce.hip), no [B, N] tensor

at FB15k-237's shape (N = 14 541, B = 256, D = 64 and 200) and at the project's largest configuration (N = 1 000 000, B = 256,
D = 256).  The legs alternate (dense, fused, dense, ...) after --warmup rounds each; a leg's time is the device time between two
events around it, reported as median and min..max; its memory is the peak of torch.cuda.max_memory_allocated over the leg minus the
allocation before it and minus the gradients it leaves.  --col-chunk takes a list: every value is one more fused leg (0 = the default,
functional.bce_default_col_chunk).  Prints one JSON line per shape.  Needs a HIP device: there is no fallback.

    python tools/fused_loss_bench.py [--rounds 7] [--warmup 2] [--col-chunk 0,14560] [--shapes fb64,fb200,c5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import functional as K  # noqa: E402
from mr_gnas_amd.sampler import LabelIndex  # noqa: E402

SHAPES = {"fb64": (14541, 237, 256, 64, 272115), "fb200": (14541, 237, 256, 200, 272115), "c5": (1_000_000, 64, 256, 256, 4_000_000)}
SMOOTH = 0.1


def leg(fn, ent, sub, relb):
    e, s, r = (t.detach().requires_grad_(True) for t in (ent, sub, relb))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = fn(e, s, r)
    loss.backward()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before - sum(t.grad.numel() * 4 for t in (e, s, r))
    return a.elapsed_time(b), peak, float(loss.detach())


def spread(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--col-chunk", default="0")
    ap.add_argument("--shapes", default="fb64,fb200,c5")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("fused_loss_bench: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("fused_loss_bench needs a HIP device")
    dev = "cuda"
    chunks = [int(c) for c in args.col_chunk.split(",")]
    for name in args.shapes.split(","):
        N, R, B, D, T = SHAPES[name]
        g = torch.Generator().manual_seed(0)
        tri = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, R, (T,), generator=g), torch.randint(0, N, (T,), generator=g)), 1)
        index = LabelIndex(tri.to(dev), R, N, dev)
        subj, rel = tri[:B, 0].to(dev), tri[:B, 1].to(dev)
        scale = 0.3 if D <= 64 else 0.15
        ent, sub, relb = ((scale * torch.randn(n, D, generator=g)).to(dev) for n in (N, B, B))
        legs = {"dense": lambda e, s, r: F.binary_cross_entropy(K.distmult_scores_all(e, s, r), index.labels(subj, rel, SMOOTH))}
        for c in chunks:
            cc = c or K.bce_default_col_chunk(B)
            legs[f"fused_col_chunk_{cc}"] = (lambda e, s, r, cc=cc: K.distmult_bce_all(e, s, r, index, subj, rel, SMOOTH, cc))
        times, peaks, losses = {k: [] for k in legs}, {k: 0 for k in legs}, {}
        for rnd in range(args.warmup + args.rounds):
            for k, fn in legs.items():                          # alternating: one leg of each kind per round
                ms, peak, loss = leg(fn, ent, sub, relb)
                if rnd >= args.warmup:
                    times[k].append(ms)
                    peaks[k] = max(peaks[k], peak)
                    losses[k] = loss
        print(json.dumps({"shape": {"name": name, "N": N, "B": B, "D": D, "label_smooth": SMOOTH, "matrix_MiB": B * N * 4 / 2 ** 20},
                          "legs": {k: {**spread(times[k]), "peak_MiB": peaks[k] / 2 ** 20, "loss": losses[k]} for k in legs}}), flush=True)
        del index, ent, sub, relb, legs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
