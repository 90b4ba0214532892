#!/usr/bin/env python3
"""Forward + backward timing of the ConvE scorers (csrc/conve.hip, functional/conve.py) against torch's formulation on the GPU:
  train_default  sf_ConvE_op at the training driver's defaults (B 256, D 128, 32 x 8 image, ks 8, F 128)
  sf_defaults    sf_ConvE_op at its own defaults (B 256, D 200, 40 x 10 image, ks 7, F 200)
  compgcn_d200   CompGCN_ConvE's scorer part (interleaved 20 x 20 image, ks 7, F 200, score bias) on given rows
N = 14 541 entities, dropout at the modules' defaults (0.3 / 0.3; the masks are drawn in both forms), training mode.  HIP events,
a warm-up, the median of the repeats; launches per call are the library calls the meter saw in one step (the torch form makes none).
Figures from the shapes: conv and fc GFLOP of the forward, the z and Wfc bytes.  Prints one JSON line.
Usage on the GPU box:  python tools/conve_bench.py [--reps 20]"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mr_gnas_amd import _lib, compgcn as CG, operations_lp as O  # noqa: E402
from mr_gnas_amd import functional as K  # noqa: E402

B, N = 256, 14_541
SHAPES = {  # name: (kind, D, k_h, k_w, ks, F)
    "train_default": ("sf", 128, 16, 8, 8, 128),
    "sf_defaults": ("sf", 200, 20, 10, 7, 200),
    "compgcn_d200": ("compgcn", 200, 20, 10, 7, 200),
}


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


def scorer(kind, D, k_h, k_w, ks, F):
    if kind == "sf":
        op = O.sf_ConvE_op({"embed_dim": D, "num_filt": F, "ker_sz": ks, "k_w": k_w, "k_h": k_h}).cuda()
        return op, lambda ent, s, r, hip: op(ent, s, r)
    net = CG.CompGCN_ConvE(0, 2, 2, 4, [D], num_filt=F, ker_sz=ks, k_w=k_w, k_h=k_h)
    del net.compGCN_Model
    net.bias = torch.nn.Parameter(torch.zeros(N))
    net = net.cuda()

    def run(ent, s, r, hip):
        if hip:
            return K.conve_scores(s, r, K.conve.INTERLEAVED, (2 * k_w, k_h), net.bn0, net.m_conv1, net.bn1, net.feature_drop, net.fc,
                                  net.hidden_drop, net.bn2, net._one, ent, net.bias)
        x = net.bn0(net.concat(s, r))
        x = net.feature_drop(torch.relu(net.bn1(net.m_conv1(x))))
        x = torch.relu(net.bn2(net.hidden_drop(net.fc(x.view(-1, net.flat_sz)))))
        return torch.sigmoid(x @ ent.t() + net.bias)
    return net, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name, (kind, D, k_h, k_w, ks, F) in SHAPES.items():
        mod, run = scorer(kind, D, k_h, k_w, ks, F)
        mod.train()
        Hi, Wi = (2 * k_h, k_w) if kind == "sf" else (2 * k_w, k_h)
        P = (Hi - ks + 1) * (Wi - ks + 1)
        Kfc = F * P
        ent = torch.randn(N, D, device="cuda", generator=gen).requires_grad_(True)
        s = torch.randn(B, D, device="cuda", generator=gen).requires_grad_(True)
        r = torch.randn(B, D, device="cuda", generator=gen).requires_grad_(True)
        gout = torch.randn(B, N, device="cuda", generator=gen)
        ref = copy.deepcopy(mod)
        if kind == "sf":
            ref.conv2d.register_forward_hook(lambda *a: None)       # a hooked submodule: torch's formulation

        def step(m, hip):
            for t in (ent, s, r):
                t.grad = None
            m.zero_grad(set_to_none=True)
            if kind == "sf":
                y = m(ent, s, r)
            else:
                y = run(ent, s, r, hip)
            y.backward(gout)

        hip_run = lambda: step(mod, True)
        if kind == "sf":
            torch_run = lambda: step(ref, False)
        else:
            torch_run = lambda: step(mod, False)
        _lib.meter.start()
        hip_run()
        rec_m = _lib.meter.stop()
        conve_calls = {k: v["launches"] for k, v in rec_m.items() if k.startswith("mrg_conve")}
        rec = {"shape": name, "B": B, "N": N, "D": D, "image": [Hi, Wi], "ks": ks, "F": F, "fc_K": Kfc,
               "conv_gflop": round(2.0 * B * Kfc * ks * ks / 1e9, 3), "fc_gflop": round(2.0 * B * Kfc * D / 1e9, 3),
               "z_mb": round(4.0 * B * Kfc / 1e6, 1), "wfc_mb": round(4.0 * D * Kfc / 1e6, 1),
               "library_calls_per_step": sum(v["launches"] for v in rec_m.values()), "conve_calls_per_step": conve_calls,
               "conve_kernel_launches_per_step": {"forward": 5, "backward": 6},
               "hip_ms": round(timeit(hip_run, args.reps), 4), "torch_ms": round(timeit(torch_run, args.reps), 4)}
        rec["speedup"] = round(rec["torch_ms"] / rec["hip_ms"], 3)
        rows.append(rec)
        del mod, ref, ent, s, r, gout
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "conve_bench", "shapes": rows}))


if __name__ == "__main__":
    main()
