#!/usr/bin/env python3
"""Generate the score-function search fixture under tests/golden/ by RUNNING THE REFERENCE (see make_golden.py for the stand-ins and
the rules).  Arrays only.

    python tests/golden/make_golden_sf_mix.py

  sf_mix_small   models.cell_lp.Cell_SF(gamma) on CPU -- MixedOp_SF over SF_OPS = ['sf_TransE', 'sf_DisMult'], the cell the
                 reference's supernet forward was written to end in (models/model_search_lp.py:160-161) -- for two cases,
                 (B, N, D) = (70, 130, 33) and (5, 70, 8): the [B, N] mixed score for W = softmax(alpha), alpha = [[0.4, -0.2]], the
                 BCELoss against labels drawn at density 0.1 and smoothed as utils/data_set.py:21-23 smooths them, and the gradients
                 with respect to all_ent, sub_emb, rel_emb and alpha.

As in make_golden_transe.py, the reference's gamma = 40 would saturate every TransE prediction at this size: gamma is the rounded
median L1 distance of the batch, recorded together with the fraction of cells whose TransE component lies in (0.01, 0.99).  The labels
are stored as the 0 / 1 matrix (uint8) and the smoothing; a test rebuilds the float32 labels with the reference's expression, and
W = softmax(alpha) is not stored.  What remains is float32 data that does not compress: case a's inputs (130 + 2 * 70 rows of 33), its
[70, 130] score and its three gradients are 27 000 floats, 108 KB of the file's 111 KB.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins, npify  # noqa: E402

ALPHA = [[0.4, -0.2]]
LABEL_SMOOTH = 0.1
CASES = {"a": (70, 130, 33), "b": (5, 70, 8)}


def smooth(label01, num_ent, label_smooth=LABEL_SMOOTH):
    """utils/data_set.py:21-23"""
    return (1.0 - label_smooth) * label01 + (1.0 / num_ent)


def case(tag, B, N, D, seed, st):
    import models.cell_lp as CL
    gen = torch.Generator().manual_seed(seed)
    ent, sub, rel = (0.5 * torch.randn(n, D, generator=gen) for n in (N, B, B))
    label01 = (torch.rand(B, N, generator=gen) < 0.1).float()
    label01[0, 0] = 1.0                                        # never an all-zero matrix
    with torch.no_grad():
        dist = torch.norm((sub + rel).unsqueeze(1) - ent, p=1, dim=2)
    gamma = float(torch.round(dist.median()))
    assert gamma > 0
    cell = CL.Cell_SF(gamma)
    assert [type(op[0]).__name__ for op in cell.cell_score._ops[0]._ops] == ["sf_TransE_op", "sf_DisMult_op"]
    ent, sub, rel = (t.clone().requires_grad_(True) for t in (ent, sub, rel))
    alpha = torch.tensor(ALPHA, dtype=torch.float32, requires_grad=True)
    W = torch.softmax(alpha, dim=1)
    score = cell(ent, sub, rel, W)
    loss = torch.nn.BCELoss()(score, smooth(label01, N))
    loss.backward()
    with torch.no_grad():
        p0 = torch.sigmoid(gamma - dist)
        frac = float(((p0 > 0.01) & (p0 < 0.99)).float().mean())
    assert frac > 0.5, frac
    st.update({f"{tag}/ent": ent, f"{tag}/sub": sub, f"{tag}/rel": rel, f"{tag}/alpha": alpha,
               f"{tag}/label01": label01.to(torch.uint8), f"{tag}/label_smooth": np.array(LABEL_SMOOTH), f"{tag}/gamma": np.array(gamma),
               f"{tag}/unsaturated_fraction": np.array(frac), f"{tag}/score": score, f"{tag}/loss": loss,
               f"{tag}/g_ent": ent.grad, f"{tag}/g_sub": sub.grad, f"{tag}/g_rel": rel.grad, f"{tag}/g_alpha": alpha.grad})
    print("sf_mix_small %s: B=%d N=%d D=%d gamma=%g loss=%.6f unsaturated=%.3f g_alpha=%s" % (tag, B, N, D, gamma, float(loss.detach()), frac,
                                                                                            alpha.grad.tolist()))


def main():
    _install_standins()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    st = {}
    for i, (tag, (B, N, D)) in enumerate(CASES.items()):
        case(tag, B, N, D, 41 + i, st)
    np.savez_compressed(os.path.join(OUT, "sf_mix_small.npz"), **npify(st))


if __name__ == "__main__":
    main()
