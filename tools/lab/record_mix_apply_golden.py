#!/usr/bin/env python3
"""Lab: record what mrg_mix_bwd_apply writes, bit for bit, as fixtures of tests/test_mix_apply_gpu.py.

Run ONCE on the GPU against the build whose bits are to be pinned (the by-index kernels, before the role kernels replaced them):
    python tools/lab/record_mix_apply_golden.py [OUT_DIR]           (default: tests/golden)
writes OUT_DIR/mix_apply_<case>.npz for every case of test_mix_apply_gpu.GOLDEN_CASES: the seed and the output tensors only --
the inputs are rebuilt from the seed by a CPU generator (test_mix_apply_gpu.make_case).  A later build must reproduce them with
torch.equal; recording again from a build under test would pin nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_mix_apply_gpu as T  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
os.makedirs(out_dir, exist_ok=True)
total = 0
for name, case in T.GOLDEN_CASES.items():
    tensors = {k: v.numpy() for k, v in T.golden_tensors(name).items()}
    path = os.path.join(out_dir, f"mix_apply_{name}.npz")
    np.savez(path, seed=np.int64(case[6]), **tensors)
    total += os.path.getsize(path)
    print(f"{path}: {len(tensors)} tensors, {os.path.getsize(path)} bytes")
print(f"{total} bytes in all")
