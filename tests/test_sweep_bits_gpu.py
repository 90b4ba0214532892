"""The register-tiled [queries, entities] sweeps -- the L1 sweep of csrc/transe_1n.hip and the mixed-score sweeps of csrc/sf_mix_1n.hip
at two and three scorers, all built from csrc/sweep_tile.hpp -- write the bits they wrote when each was a kernel file of its own:
tests/golden/sweep_1n_bits.npz, recorded by tools/lab/record_sweep_bits.py from that build.  Losses, gradient slices, weight
gradients (written and added to), filtered and raw ranks, the whole backward of sf_mix_bce_all / sf_mix3_bce_all at col_chunk = 64, and
the TransE loss, logit gradient, ranks and top-k lists, on the inputs of tests/sweep_bits_case.py.

A bit that differs means the arithmetic moved (an order of summation, a contraction, the tie rule): restore the expression; recording
again from the build under test would pin nothing."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import sweep_bits_case as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLDEN, "sweep_1n_bits.npz")) as z:
        return {k: np.array(z[k]) for k in z.files}


@pytest.mark.parametrize("name", list(C.CASES))
def test_bits_of_the_separate_kernel_files(name, recorded):
    ref = {k[len(name) + 1:]: v for k, v in recorded.items() if k.startswith(name + "/")}
    got = C.pack(C.outputs(name))
    assert set(ref) == set(got), "the fixture holds other outputs than this build produces"
    assert list(ref["#names"]) == list(got["#names"])
    bad = []
    for i, k in enumerate(got["#names"]):
        if not np.array_equal(ref["#sha"][i], got["#sha"][i]):
            bad.append(f"{k} (digest; float64 sum {got['#sum'][i]!r}, recorded {ref['#sum'][i]!r})")
    for k in sorted(set(ref) - {"#names", "#sha", "#sum"}):
        a, b = torch.from_numpy(got[k]), torch.from_numpy(ref[k])
        if not torch.equal(a, b):
            bad.append(f"{k} ({int((a != b).sum()) if a.shape == b.shape else 'shape'} entries)")
    assert not bad, f"{name}: {len(bad)} outputs differ from the recorded bits: " + "; ".join(bad)
