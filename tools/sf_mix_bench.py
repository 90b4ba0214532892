#!/usr/bin/env python3
"""The score-function search loss alone -- forward plus backward down to the gradients of the entity table, the subject rows, the
relation rows and the two mixing weights -- three ways, in one process:

  dense  the literal formulation: cell_lp.MixedOp_SF.forward (two [B, N] score matrices and their weighted sum) + LabelIndex.labels
         ([B, N] targets) + F.binary_cross_entropy
  fused  functional.sf_mix_bce_all (csrc/sf_mix_1n.hip): no [B, N] tensor
  fixed  functional.transe_bce_all + functional.distmult_bce_all, the two fixed-genotype losses one after the other.  NOT the same
         number (BCE of a mixture is not a mixture of BCEs): the price of the two sweeps the mixed one replaces, for scale.

at FB15k-237's shape (N = 14 541, B = 256 and 1024, D = 64 and 200) and WN18RR's entity count (N = 40 943, B = 256, D = 200).  gamma is
the rounded median distance of the batch.  The legs alternate (dense, fused, fixed, dense, ...) after --warmup rounds each; a leg's
time is the device time between two events around it, reported as median and min..max; its memory is the peak of
torch.cuda.max_memory_allocated over the leg minus the allocation before it and minus the gradients it leaves.  After the timed
rounds the fused leg runs once more under the library's per-entry-point meter.  Prints one JSON line per shape.  Needs a HIP device:
there is no fallback.

    python tools/sf_mix_bench.py [--rounds 7] [--warmup 2] [--shapes fb64,fb200,fb200b,wn200] [--col-chunk 0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import _lib, cell_lp as CL, functional as K, operations_lp as O  # noqa: E402
from mr_gnas_amd.sampler import LabelIndex  # noqa: E402

SHAPES = {"fb64": (14541, 237, 256, 64, 272115), "fb200": (14541, 237, 256, 200, 272115), "fb200b": (14541, 237, 1024, 200, 272115),
          "wn200": (40943, 11, 256, 200, 86835)}
SMOOTH = 0.1
WEIGHTS = (0.55, 0.45)


def leg(fn, ent, sub, relb, w):
    e, s, r, ww = (t.detach().requires_grad_(True) for t in (ent, sub, relb, w))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = fn(e, s, r, ww)
    loss.backward()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before - sum(t.grad.numel() * 4 for t in (e, s, r, ww) if t.grad is not None)
    return a.elapsed_time(b), peak, float(loss.detach())


def spread(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--col-chunk", type=int, default=0)
    ap.add_argument("--shapes", default="fb64,fb200,fb200b,wn200")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("sf_mix_bench: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("sf_mix_bench needs a HIP device")
    dev = "cuda"
    for name in args.shapes.split(","):
        N, R, B, D, T = SHAPES[name]
        g = torch.Generator().manual_seed(0)
        tri = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, R, (T,), generator=g), torch.randint(0, N, (T,), generator=g)), 1)
        index = LabelIndex(tri.to(dev), R, N, dev)
        subj, rel = tri[:B, 0].to(dev), tri[:B, 1].to(dev)
        scale = 0.3 if D <= 64 else 0.15
        ent, sub, relb = ((scale * torch.randn(n, D, generator=g)).to(dev) for n in (N, B, B))
        w = torch.tensor(WEIGHTS, dtype=torch.float32, device=dev)
        with torch.no_grad():
            o = sub + relb
            gamma = float(torch.round((o.unsqueeze(1) - ent[:1024].unsqueeze(0)).abs().sum(-1).median()))   # over the first 1024 entities
        mixed = CL.MixedOp_SF(gamma, O.SF_OPS).to(dev)
        cc = args.col_chunk or None
        legs = {"dense": lambda e, s, r, ww: F.binary_cross_entropy(mixed(ww, e, s, r), index.labels(subj, rel, SMOOTH)),
                "fused": lambda e, s, r, ww: K.sf_mix_bce_all(e, s, r, ww, gamma, index, subj, rel, SMOOTH, cc),
                "fixed": lambda e, s, r, ww: (K.transe_bce_all(e, s, r, gamma, index, subj, rel, SMOOTH)
                                              + K.distmult_bce_all(e, s, r, index, subj, rel, SMOOTH))}
        times, peaks, losses = {k: [] for k in legs}, {k: 0 for k in legs}, {}
        for rnd in range(args.warmup + args.rounds):
            for k, fn in legs.items():                          # alternating: one leg of each kind per round
                ms, peak, loss = leg(fn, ent, sub, relb, w)
                if rnd >= args.warmup:
                    times[k].append(ms)
                    peaks[k] = max(peaks[k], peak)
                    losses[k] = loss
        _lib.meter.start()
        leg(legs["fused"], ent, sub, relb, w)
        entry_ms = {n: round(r["ms"], 4) for n, r in sorted(_lib.meter.stop().items())}
        print(json.dumps({"shape": {"name": name, "N": N, "B": B, "D": D, "label_smooth": SMOOTH, "gamma": gamma, "weights": WEIGHTS,
                                    "matrix_MiB": B * N * 4 / 2 ** 20},
                          "legs": {k: {**spread(times[k]), "peak_MiB": peaks[k] / 2 ** 20, "loss": losses[k]} for k in legs},
                          "fused_entry_ms": entry_ms}), flush=True)
        del index, ent, sub, relb, legs, mixed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
