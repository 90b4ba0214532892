#!/usr/bin/env python3
"""Forward timing of the standalone ccorr(a, b) (csrc/ccorr.hip, functional/ccorr.py) with a shared row b [1, D] against a [N, D]:
  rows     the per-row kernel (mrg_ccorr_rows) on the pair with b expanded to [N, D] beforehand (the kernel alone);
  matrix   the shared-row path: circulant build + the split-core row GEMM (``functional.linear``);
  linear   ``functional.linear`` alone at [N, D] x [D, D] (what the matrix path costs without its builder);
  gcs      the existing compose_aggregate("ccorr", ...) in its self-loop form (one element per segment, CompGCN's loop plan).
HIP events, median of the repeats; fraction = 2 N D^2 flop / time / the 157.3 TF f32 vector peak.  `sweep` times the two paths at
D = 200 over row counts: where the matrix path starts to win is functional/ccorr.py's MATRIX_MIN_ROWS.
Prints one JSON line.  Usage on the GPU box:  python tools/ccorr_bench.py [--reps 20]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import functional as K  # noqa: E402

C = importlib.import_module("mr_gnas_amd.functional.ccorr")
PEAK_TF = 157.3
SHAPES = [(200, 300), (200, 14_541), (200, 544_230), (256, 1_000_000)]
SWEEP = [256, 512, 1024, 2048, 4096, 8192, 16_384, 32_768, 65_536]


def timeit(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def forms(D, N, gen):
    a = torch.randn(N, D, device="cuda", generator=gen)
    b = torch.randn(1, D, device="cuda", generator=gen)
    bx = b.expand(N, D).contiguous()

    def matrix():
        K.switches.CCORR_PATH = "matrix"
        try:
            return K.ccorr(a, b)
        finally:
            K.switches.CCORR_PATH = None

    return a, b, bx, {"rows": lambda: C._rows(C.CORR, a, bx), "matrix": matrix}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    with torch.no_grad():
        for D, N in SHAPES:
            a, b, bx, fns = forms(D, N, gen)
            W = torch.randn(D, D, device="cuda", generator=gen)
            ar = torch.arange(N, device="cuda")
            plan = K.ComposePlan(ar, torch.zeros(N, dtype=torch.long, device="cuda"), ar, None, N, 1, N)
            fns["linear"] = lambda: K.linear(a, W)
            fns["gcs"] = lambda: K.compose_aggregate("ccorr", a, b, plan)
            ref = fns["rows"]()
            for name in ("matrix", "gcs"):
                err = float((fns[name]() - ref).abs().max() / ref.abs().max())
                assert err < 1e-5, (name, D, N, err)
            flops = 2.0 * N * D * D
            rec = {"D": D, "N": N, "auto_path": "matrix" if C._use_matrix(N, D) else "rows"}
            for name, fn in fns.items():
                ms = timeit(fn, args.reps)
                rec[name] = {"ms": round(ms, 4), "gflops": round(flops / ms / 1e6, 1), "frac_peak": round(flops / ms / 1e9 / PEAK_TF, 4)}
            rows.append(rec)
            del a, b, bx, W, plan, fns, ref
            torch.cuda.empty_cache()
        sweep = []
        for N in SWEEP:
            _, _, _, fns = forms(200, N, gen)
            sweep.append({"N": N, "rows_ms": round(timeit(fns["rows"], args.reps), 4), "matrix_ms": round(timeit(fns["matrix"], args.reps), 4)})
    print(json.dumps({"tool": "ccorr_bench", "peak_tf": PEAK_TF, "matrix_min_rows": C.MATRIX_MIN_ROWS, "shapes": rows, "sweep": sweep}))


if __name__ == "__main__":
    main()
