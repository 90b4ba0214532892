#!/usr/bin/env python3
"""One filtered link-prediction evaluation at FB15k-237's shape (N = 14 541 entities, R = 237, D = 200, T = 20 466 test triples, a
synthetic known set of 310 116 triples: 272 115 train + 17 535 valid + the test triples), two ways, in one process:

  fused        evaluation.calc_mrr: mrg_distmult_rank, the row GEMM with the counting epilogue; no [Q, N] tensor
  composition  the entry points that existed before it, in batches of 1000 queries: compose (mult) -> mrg_linear_fwd with the sigmoid
               epilogue ([B, N] scores) -> mrg_multi_hot_labels ([B, N] labels) -> mrg_rank_filtered, both passes

The legs alternate (fused, composition, fused, ...) after one warm-up each; times are host clocks around work that ends in a device
synchronise, reported as median and min..max.  `fused_rank_ms` is the device time of the mrg_distmult_rank calls alone (HIP events
around the calls, from a separate round), and `bf16_pipe_share` is the bf16 matrix work those calls issue -- six 32 x 32 x 16 MFMA
terms per product over the padded shape -- over that time and the 2.5 PFLOP/s dense bf16 peak.  The composition filters every known
triple but the query's own, i.e. calc_mrr's protocol="standard"; `ranks_equal_share` compares the two legs' ranks under that protocol
(they differ where float32 sigmoid rounds two scores together).  Prints one JSON line.

    python tools/mrr_bench.py [--reps 5] [--batch 1000] [--eval-bz 40932]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import _lib, evaluation as EV, functional as K  # noqa: E402
from mr_gnas_amd.sampler import LabelIndex  # noqa: E402

N, R, D = 14541, 237, 200
N_TRAIN, N_VALID, N_TEST = 272115, 17535, 20466
BF16_PEAK = 2.5e15


def composition_ranks(emb, w, index, test, batch):
    """cat(ranks_s, ranks_o) through [B, N] scores and labels.  index: LabelIndex of the known triples (relation r + R = inverse)."""
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    out = []
    for fixed, rel, tgt in ((o, r + R, s), (s, r, o)):
        for b in range(0, test.shape[0], batch):
            f, rl, t = fixed[b:b + batch], rel[b:b + batch], tgt[b:b + batch]
            pred = K.linear(K.compose("mult", emb[f], w[rl % R]), emb, None, "sigmoid")
            out.append(EV.filtered_ranks(pred, index.labels(f, rl), t))
    return torch.cat(out)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--eval-bz", type=int, default=2 * N_TEST)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mrr_bench needs a HIP device")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    tri = lambda n: torch.stack((torch.randint(0, N, (n,), generator=g), torch.randint(0, R, (n,), generator=g),
                                 torch.randint(0, N, (n,), generator=g)), 1)
    train, valid, test = tri(N_TRAIN).to(dev), tri(N_VALID).to(dev), tri(N_TEST).to(dev)
    emb, w = torch.randn(N, D, generator=g).mul_(0.4).to(dev), torch.randn(R, D, generator=g).to(dev)
    index = LabelIndex(torch.cat((train, valid, test)), R, N, dev)

    fused = lambda protocol="reference": EV.calc_mrr(emb, w, train, valid, test, hits=[1, 3, 10], eval_bz=args.eval_bz, protocol=protocol)
    comp = lambda: composition_ranks(emb, w, index, test, args.batch)
    fused(), comp()                                                       # warm-up: code objects, allocator
    t_f, t_c = [], []
    for _ in range(args.reps):
        t_f.append(timed(fused))
        t_c.append(timed(comp))
    _lib.meter.start(["mrg_distmult_rank"])
    for _ in range(args.reps):
        fused()
    rec = _lib.meter.stop()["mrg_distmult_rank"]
    rank_ms = rec["ms"] / args.reps
    pad = lambda x, m: -(-x // m) * m
    bf16_flop = 6 * 2 * pad(2 * N_TEST, 128) * pad(N, 224) * pad(D, 16)

    known = EV.KnownTriples(train, valid, test, N, R)
    std = EV._both_passes(emb, w, test, args.eval_bz, known, "standard")
    same = float((std == comp()).double().mean())
    mrr, hits = fused()
    print(json.dumps({"shape": {"N": N, "R": R, "D": D, "T": N_TEST, "known": N_TRAIN + N_VALID + N_TEST, "queries": 2 * N_TEST},
                      "fused": spread(t_f), "composition": spread(t_c), "composition_batch": args.batch, "eval_bz": args.eval_bz,
                      "speedup_median": float(np.median(t_c) / np.median(t_f)),
                      "fused_rank_ms": rank_ms, "fused_rank_launches": rec["launches"] // args.reps,
                      "bf16_pipe_share": bf16_flop / (rank_ms * 1e-3) / BF16_PEAK, "algorithmic_tflops": 2 * 2 * N_TEST * N * D / (rank_ms * 1e-3) / 1e12,
                      "ranks_equal_share": same, "mrr": mrr, "hits": hits}))


if __name__ == "__main__":
    main()
