#!/usr/bin/env python3
"""What optim.FusedAdam and the architect step cost on the GPU, against torch's own.

  adam       device-event time, host time and launch count of one optimiser step over (a) the parameter list of bench.py's FixedStep
             model (fb15k237_fixed_d64) and (b) the supernet's five architecture parameters: optim.FusedAdam, torch.optim.Adam with its
             defaults, torch.optim.Adam(capturable=True).  Every optimiser steps its own copy of the parameters on the same fixed
             gradients; the three are timed ALTERNATELY, rep by rep, after a warm-up.
  architect  architect.Architect.step with weight_grads True (the reference's behaviour: the baseline) and False, alternately, at the
             fb15k237_supernet_300 and fb15k237_supernet_30k shapes of bench.py (the step's own sample serves as the validation sample).

  unrolled   the second-order architect step (architect_unrolled.SecondOrderArchitect.step(unrolled=True), eta = 0.01, the step's
             ClippedSGD for the momentum buffers) against the first-order step of the same object, alternately, on the D = 200 supernet
             of fb15k237_supernet_300; and its parameter passes alone -- virtual step, radius, two shifts, restore: five mrg_unrolled_*
             calls -- against the same arithmetic written with torch._foreach_* (eta a host float, R a 0-dim device tensor), on that
             model's parameter list with fixed random g, v and momentum buffers.

Times: HIP events around the call (they span the launch gaps of a launch-bound sequence) and a host clock around call + synchronise;
median and the 10th / 90th percentile over the reps.  Launches: device events of a torch.profiler run of its own (kernels and copies
counted apart), per step.  Prints one JSON line.  Usage on the GPU box:  python tools/optim_bench.py [--reps 50]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mr_gnas_amd.architect import Architect  # noqa: E402
from mr_gnas_amd.optim import FusedAdam  # noqa: E402


def stats(ts):
    return {"median": round(float(np.median(ts)), 4), "p10": round(float(np.percentile(ts, 10)), 4), "p90": round(float(np.percentile(ts, 90)), 4)}


def time_alternately(fns, reps, warm=5, between=None):
    """{name: fn} timed in turn, rep by rep: device-event ms and host ms (call + synchronise) per call."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
            if between:
                between()
    torch.cuda.synchronize()
    dev = {k: [] for k in fns}
    host = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            host[name].append((time.perf_counter() - t0) * 1e3)
            dev[name].append(a.elapsed_time(b))
            if between:
                between()
    return {k: {"device_ms": stats(dev[k]), "host_ms": stats(host[k])} for k in fns}


def count_launches(fn, n=5):
    """Device activities per call: kernels, copies / fills, and the kernels' names."""
    import collections
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    names = collections.Counter()
    for ev in prof.events():
        if ev.device_type != DeviceType.CUDA or ev.name.startswith("Optimizer.step#"):      # (the optimiser's profiler span shows up as a device activity)
            continue
        if "memcpy" in ev.name.lower() or "memset" in ev.name.lower() or "copy" in ev.name.lower() and "kernel" not in ev.name.lower():
            copies += 1
        else:
            kernels += 1
            names[ev.name.split("(")[0].split("<")[0][-48:]] += 1
    top = {k: round(v / n, 2) for k, v in names.most_common(4)}
    return {"kernels_per_step": kernels / n, "copies_per_step": copies / n, "most_launched": top}


def adam_case(params, reps, gen, no_grad=()):
    sets = {k: [p.detach().clone().requires_grad_(True) for p in params] for k in ("fused", "torch", "torch_capturable")}
    grads = [torch.randn(p.shape, device=p.device, generator=gen) * 1e-2 for p in params]
    for ps in sets.values():
        for i, (p, g) in enumerate(zip(ps, grads)):
            p.grad = None if i in no_grad else g.clone()
    opts = {"fused": FusedAdam(sets["fused"], 1e-3), "torch": torch.optim.Adam(sets["torch"], 1e-3),
            "torch_capturable": torch.optim.Adam(sets["torch_capturable"], 1e-3, capturable=True)}
    fns = {k: o.step for k, o in opts.items()}
    out = time_alternately(fns, reps)
    for k, fn in fns.items():
        out[k].update(count_launches(fn))
    out["tensors"], out["elements"] = len(params), int(sum(p.numel() for p in params))
    return out


def architect_case(workload, reps):
    saved = sys.argv
    sys.argv = ["bench.py", "--workload", workload]
    try:
        args = bench.parse()
    finally:
        sys.argv = saved
    dev = torch.device("cuda", 0)
    step = bench.Step(args, dev, bench.build_step_inputs(args.workload, args.negative, args.seed))
    a_args = types.SimpleNamespace(momentum=0.9, weight_decay=3e-4, arch_learning_rate=3e-4, arch_weight_decay=1e-3)
    sample = (step.g, step.node_id, step.src_in, step.edge_type, step.samples, step.labels)
    archs = {"weight_grads": Architect(dev, step.model, a_args), "alpha_grads_only": Architect(dev, step.model, a_args, weight_grads=False)}
    fns = {k: (lambda a=a: a.step(*sample, *sample, None, None, False)) for k, a in archs.items()}

    def between():                                            # the driver's optimizer.zero_grad(), outside the timed calls
        for p in step.params:
            p.grad = None

    out = time_alternately(fns, reps, warm=3, between=between)
    for k, fn in fns.items():
        out[k].update(count_launches(fn, 2))
        between()
    out["edges"], out["nodes"] = int(step.E), int(step.g.number_of_nodes())
    return out


def unrolled_case(workload, reps, gen):
    from mr_gnas_amd.architect_unrolled import SecondOrderArchitect, UnrolledEngine
    saved = sys.argv
    sys.argv = ["bench.py", "--workload", workload]
    try:
        args = bench.parse()
    finally:
        sys.argv = saved
    dev = torch.device("cuda", 0)
    step = bench.Step(args, dev, bench.build_step_inputs(args.workload, args.negative, args.seed))
    a_args = types.SimpleNamespace(momentum=0.9, weight_decay=3e-4, arch_learning_rate=3e-4, arch_weight_decay=1e-3)
    sample = (step.g, step.node_id, step.src_in, step.edge_type, step.samples, step.labels)
    arch = SecondOrderArchitect(dev, step.model, a_args)
    fns = {"first_order": lambda: arch.step(*sample, *sample, None, None, False),
           "second_order": lambda: arch.step(*sample, *sample, 0.01, step.opt, True)}

    def between():
        for p in step.params:
            p.grad = None

    out = {"step": time_alternately(fns, reps, warm=3, between=between)}
    for k, fn in fns.items():
        out["step"][k].update(count_launches(fn, 2))
        between()
    # the parameter passes alone, on copies of the parameter list
    eta, mom, wd, r = 0.01, 0.9, 3e-4, 1e-2
    mine = [p.detach().clone() for p in step.params]
    theirs = [p.detach().clone() for p in step.params]
    g = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in mine]
    v = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in mine]
    bufs = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in mine]
    holder = types.SimpleNamespace(parameters=lambda: mine, arch_parameters=lambda: step.arch)
    eng = UnrolledEngine(holder, mom, wd)
    opt = types.SimpleNamespace(state={p: {"momentum_buffer": b} for p, b in zip(mine, bufs)})
    eta_dev = eng._eta(eta)
    backup = [torch.empty_like(p) for p in theirs]

    def hip_passes():
        eng._virtual(g, opt, eta_dev)
        staged = eng._radius(v)
        eng._shift(staged, +1)
        eng._shift(staged, -1)
        eng._shift(None, 0)

    def foreach_passes():
        torch._foreach_copy_(backup, theirs)
        d = torch._foreach_add(g, theirs, alpha=wd)
        m = torch._foreach_mul(bufs, mom)
        torch._foreach_add_(m, d)
        torch._foreach_add_(theirs, m, alpha=-eta)
        R = r / torch.linalg.vector_norm(torch.stack(torch._foreach_norm(v)))
        rv = torch._foreach_mul(v, R)
        torch._foreach_copy_(theirs, backup)
        torch._foreach_add_(theirs, rv)
        torch._foreach_copy_(theirs, backup)
        torch._foreach_sub_(theirs, rv)
        torch._foreach_copy_(theirs, backup)

    fns = {"hip": hip_passes, "foreach": foreach_passes}
    out["passes"] = time_alternately(fns, reps)
    for k, fn in fns.items():
        out["passes"][k].update(count_launches(fn))
    out["tensors"], out["elements"] = len(mine), int(sum(p.numel() for p in mine))
    out["edges"], out["nodes"] = int(step.E), int(step.g.number_of_nodes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-architect", action="store_true")
    ap.add_argument("--only-unrolled", action="store_true", help="the unrolled leg alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs a HIP device: nothing here can be measured without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"tool": "optim_bench", "reps": a.reps}
    if a.only_unrolled:
        res["unrolled_fb15k237_supernet_300"] = unrolled_case("fb15k237_supernet_300", max(10, a.reps // 2), gen)
        print(json.dumps(res))
        return
    fixed = bench.FixedStep(types.SimpleNamespace(seed=0, hip_graph=False), dev)
    res["adam_fixedstep_params"] = adam_case(list(fixed.model.parameters()), a.reps, gen)
    del fixed
    from mr_gnas_amd import supernet as S
    net = S.SearchNetwork(dev, 14541, 237, 2, 1, 2, 2, 200, 100, 475, 40.0, 0.3, 0.1).to(dev)
    res["adam_supernet_alphas"] = adam_case(list(net.arch_parameters()), a.reps, gen, no_grad=(4,))      # the score-function alpha never has a gradient
    del net
    if not a.skip_architect:
        for w in ("fb15k237_supernet_300", "fb15k237_supernet_30k"):
            res["architect_" + w] = architect_case(w, max(10, a.reps // 2))
            torch.cuda.empty_cache()
        res["unrolled_fb15k237_supernet_300"] = unrolled_case("fb15k237_supernet_300", max(10, a.reps // 2), gen)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
