#!/usr/bin/env python3
"""Lab: record what the register-tiled 1-N sweeps (csrc/transe_1n.hip, csrc/sf_mix_1n.hip) write, bit for bit, as the fixture of
tests/test_sweep_bits_gpu.py.

Run ONCE on the GPU against the build whose bits are to be pinned (the one with a kernel file per scorer count, before they became one
template; MRG_LIB_PATH selects a library of the same ABI):
    python tools/lab/record_sweep_bits.py [OUT_DIR]           (default: tests/golden)
writes OUT_DIR/sweep_1n_bits.npz: for every case of tests/sweep_bits_case.CASES the outputs only -- the inputs are rebuilt from the
case's seed by a CPU generator (sweep_bits_case.make_inputs).  A later build must reproduce them with torch.equal; recording again
from a build under test would pin nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mr_gnas_amd  # noqa: E402,F401
import sweep_bits_case as C  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
os.makedirs(out_dir, exist_ok=True)
store = {}
for name in C.CASES:
    tensors = C.outputs(name)
    for k, v in tensors.items():
        assert not (v.is_floating_point() and bool(v.isnan().any())), f"{name} {k}: a NaN would not compare equal to itself"
    packed = C.pack(tensors)
    store.update({f"{name}/{k}": v for k, v in packed.items()})
    print(f"{name}: {len(tensors)} outputs, {len(packed['#names'])} of them as digests")
path = os.path.join(out_dir, "sweep_1n_bits.npz")
np.savez_compressed(path, **store)
print(f"{path}: {os.path.getsize(path)} bytes")
