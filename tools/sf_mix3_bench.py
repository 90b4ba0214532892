#!/usr/bin/env python3
"""The three-way score-function search loss alone -- forward plus backward down to the gradients of the entity table, the subject rows,
the relation rows, the mixing weights and the ConvE parameters -- in one process:

  dense3  the literal formulation: cell_lp.MixedOp_SF(['sf_TransE', 'sf_DisMult', 'sf_ConvE']).forward (three [B, N] score matrices
          and their weighted sum) + LabelIndex.labels ([B, N] targets) + F.binary_cross_entropy
  fused3  the same module's loss_1n: one sf_ConvE_op.query + functional.sf_mix3_bce_all (csrc/sf_mix_1n.hip): no [B, N] tensor
  fused2  functional.sf_mix_bce_all (csrc/sf_mix_1n.hip), the two-way leg over SF_OPS.  NOT the same number: for scale.

at FB15k-237's shape (N = 14 541, B = 256, D = 200; sf_ConvE_op's default 20 x 10 image, 200 filters of 7 x 7, train mode with its
default dropouts).  The legs alternate after --warmup rounds each; a leg's time is the device time between two events around it,
reported as median and min..max; its memory is the peak of torch.cuda.max_memory_allocated over the leg minus the allocation before
it and minus the gradients it leaves.  After the timed rounds the fused3 leg runs once more under the library's per-entry-point meter.
Prints one JSON line per shape.  Needs a HIP device: there is no fallback.

    python tools/sf_mix3_bench.py [--rounds 9] [--warmup 3] [--shapes fb200] [--col-chunk 0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import _lib, cell_lp as CL, functional as K  # noqa: E402
from mr_gnas_amd.sampler import LabelIndex  # noqa: E402

SHAPES = {"fb200": (14541, 237, 256, 200, 272115, (20, 10, 7, 200)), "fb200b": (14541, 237, 1024, 200, 272115, (20, 10, 7, 200)),
          "fb64": (14541, 237, 256, 64, 272115, (8, 8, 3, 32))}
SMOOTH = 0.1
WEIGHTS = (0.4, 0.35, 0.25)
THREE = ['sf_TransE', 'sf_DisMult', 'sf_ConvE']


def leg(fn, leaves, params):
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    for p in params:
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = fn(*leaves)
    loss.backward()
    b.record()
    torch.cuda.synchronize()
    left = sum(t.grad.numel() * 4 for t in [*leaves, *params] if t.grad is not None)
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - before - left, float(loss.detach())


def spread(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--col-chunk", type=int, default=0)
    ap.add_argument("--shapes", default="fb200")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("sf_mix3_bench: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("sf_mix3_bench needs a HIP device")
    dev = "cuda"
    for name in args.shapes.split(","):
        N, R, B, D, T, (k_h, k_w, ker, filt) = SHAPES[name]
        g = torch.Generator().manual_seed(0)
        tri = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, R, (T,), generator=g), torch.randint(0, N, (T,), generator=g)), 1)
        index = LabelIndex(tri.to(dev), R, N, dev)
        subj, rel = tri[:B, 0].to(dev), tri[:B, 1].to(dev)
        scale = 0.3 if D <= 64 else 0.15
        ent, sub, relb = ((scale * torch.randn(n, D, generator=g)).to(dev) for n in (N, B, B))
        w3 = torch.tensor(WEIGHTS, dtype=torch.float32, device=dev)
        w2 = torch.tensor((0.55, 0.45), dtype=torch.float32, device=dev)
        with torch.no_grad():
            o = sub + relb
            gamma = float(torch.round((o.unsqueeze(1) - ent[:1024].unsqueeze(0)).abs().sum(-1).median()))   # over the first 1024 entities
        torch.manual_seed(0)
        mixed = CL.MixedOp_SF(gamma, THREE, sf_args={'embed_dim': D, 'k_h': k_h, 'k_w': k_w, 'ker_sz': ker, 'num_filt': filt}).to(dev).train()
        params = list(mixed.parameters())
        assert mixed._fused_1n(w3, ent, sub, relb)
        cc = args.col_chunk or None
        legs = {"dense3": (lambda e, s, r, ww: F.binary_cross_entropy(mixed(ww, e, s, r), index.labels(subj, rel, SMOOTH)), w3),
                "fused3": (lambda e, s, r, ww: mixed.loss_1n(ww, e, s, r, index, subj, rel, SMOOTH, cc), w3),
                "fused2": (lambda e, s, r, ww: K.sf_mix_bce_all(e, s, r, ww, gamma, index, subj, rel, SMOOTH, cc), w2)}
        times, peaks, losses = {k: [] for k in legs}, {k: 0 for k in legs}, {}
        for rnd in range(args.warmup + args.rounds):
            for k, (fn, w) in legs.items():                     # alternating: one leg of each kind per round
                ms, peak, loss = leg(fn, (ent, sub, relb, w), params)
                if rnd >= args.warmup:
                    times[k].append(ms)
                    peaks[k] = max(peaks[k], peak)
                    losses[k] = loss
        _lib.meter.start()
        leg(legs["fused3"][0], (ent, sub, relb, w3), params)
        entry_ms = {n: round(r["ms"], 4) for n, r in sorted(_lib.meter.stop().items())}
        print(json.dumps({"shape": {"name": name, "N": N, "B": B, "D": D, "conve": [k_h, k_w, ker, filt], "label_smooth": SMOOTH, "gamma": gamma,
                                    "weights": WEIGHTS, "matrix_MiB": B * N * 4 / 2 ** 20},
                          "legs": {k: {**spread(times[k]), "peak_MiB": peaks[k] / 2 ** 20, "loss": losses[k]} for k in legs},
                          "fused3_entry_ms": entry_ms}), flush=True)
        del index, ent, sub, relb, legs, mixed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
