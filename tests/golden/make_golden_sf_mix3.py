#!/usr/bin/env python3
"""Generate the three-way score-function search fixture under tests/golden/ by RUNNING THE REFERENCE (see make_golden.py for the
stand-ins and the rules).  Arrays only.

    python tests/golden/make_golden_sf_mix3.py

  sf_mix3_small  models.cell_lp.MixedOp_SF(gamma, ['sf_TransE', 'sf_DisMult', 'sf_ConvE']) on CPU in train mode -- the reference's
                 scorer registry has the third entry (models/operations_lp.py:26-30) and its MixedOp_SF takes the list as an argument
                 (models/cell_lp.py:36-50) -- for two cases, (B, N, D, k_h, k_w, ker_sz, num_filt) = (70, 130, 32, 4, 8, 3, 4) and
                 (5, 70, 8, 2, 4, 2, 3): the [B, N] mixed score for W = softmax(alpha), alpha = [[0.4, -0.2, 0.1]], the BCELoss against
                 labels drawn at density 0.1 and smoothed as utils/data_set.py:21-23 smooths them, and the gradients with respect to
                 all_ent, sub_emb, rel_emb, alpha and every ConvE parameter.

The reference's MixedOp_SF builds its scorers from {'gamma': gamma} alone, so its sf_ConvE is bound to D = 200 = 20 x 10 with 200
filters of 7 x 7: the ConvE entry is replaced after construction by a reference sf_ConvE_op of the case's small size, both dropouts
at 0 (everything else is the reference's constructor and forward).  Its state_dict BEFORE the step is stored: the train-mode forward
updates the BatchNorm running statistics, which the loss does not depend on.  Everything else follows make_golden_sf_mix.py: the
generator, gamma as the rounded median L1 distance of the batch, the label density, the smoothing, W not stored.  The fractions of
cells whose TransE / ConvE component lies in (0.01, 0.99) are asserted above one half and recorded.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins, npify  # noqa: E402
from make_golden_sf_mix import LABEL_SMOOTH, smooth  # noqa: E402

ALPHA = [[0.4, -0.2, 0.1]]
NAMES = ['sf_TransE', 'sf_DisMult', 'sf_ConvE']
CASES = {"a": (70, 130, 32, 4, 8, 3, 4), "b": (5, 70, 8, 2, 4, 2, 3)}


def case(tag, B, N, D, k_h, k_w, ker, filt, seed, st):
    import models.cell_lp as CL
    import models.operations_lp as OL
    gen = torch.Generator().manual_seed(seed)
    ent, sub, rel = (0.5 * torch.randn(n, D, generator=gen) for n in (N, B, B))
    label01 = (torch.rand(B, N, generator=gen) < 0.1).float()
    label01[0, 0] = 1.0                                        # never an all-zero matrix
    with torch.no_grad():
        dist = torch.norm((sub + rel).unsqueeze(1) - ent, p=1, dim=2)
    gamma = float(torch.round(dist.median()))
    assert gamma > 0
    torch.manual_seed(seed)                                    # the ConvE parameters' initial values
    mixed = CL.MixedOp_SF(gamma, NAMES)
    sf_args = {'gamma': gamma, 'embed_dim': D, 'k_h': k_h, 'k_w': k_w, 'ker_sz': ker, 'num_filt': filt, 'conve_hid_drop': 0.0, 'feat_drop': 0.0}
    mixed._ops[2][0] = OL.sf_ConvE_op(sf_args)
    assert [type(op[0]).__name__ for op in mixed._ops] == ["sf_TransE_op", "sf_DisMult_op", "sf_ConvE_op"]
    conve = mixed._ops[2][0]
    with torch.no_grad():                                      # BatchNorm weights and biases away from 1 / 0, so that their gradients count
        for bn in (conve.bn0, conve.bn1, conve.bn2):
            bn.weight.copy_(1.0 + 0.2 * torch.randn(bn.weight.shape, generator=gen))
            bn.bias.copy_(0.1 * torch.randn(bn.bias.shape, generator=gen))
    mixed.train()
    before = {k: v.detach().clone() for k, v in conve.state_dict().items()}
    ent, sub, rel = (t.clone().requires_grad_(True) for t in (ent, sub, rel))
    alpha = torch.tensor(ALPHA, dtype=torch.float32, requires_grad=True)
    W = torch.softmax(alpha, dim=1)
    score = mixed(W[0], ent, sub, rel)
    loss = torch.nn.BCELoss()(score, smooth(label01, N))
    loss.backward()
    with torch.no_grad():
        p0 = torch.sigmoid(gamma - dist)
        p2 = conve(ent, sub, rel)                              # train mode still: the batch's statistics, as in the step above
        frac0 = float(((p0 > 0.01) & (p0 < 0.99)).float().mean())
        frac2 = float(((p2 > 0.01) & (p2 < 0.99)).float().mean())
    assert frac0 > 0.5, frac0
    assert frac2 > 0.5, frac2
    st.update({f"{tag}/ent": ent, f"{tag}/sub": sub, f"{tag}/rel": rel, f"{tag}/alpha": alpha,
               f"{tag}/label01": label01.to(torch.uint8), f"{tag}/label_smooth": np.array(LABEL_SMOOTH), f"{tag}/gamma": np.array(gamma),
               f"{tag}/conve_shape": np.array([D, k_h, k_w, ker, filt]),
               f"{tag}/unsaturated_fraction": np.array(frac0), f"{tag}/unsaturated_fraction_conve": np.array(frac2),
               f"{tag}/score": score, f"{tag}/loss": loss,
               f"{tag}/g_ent": ent.grad, f"{tag}/g_sub": sub.grad, f"{tag}/g_rel": rel.grad, f"{tag}/g_alpha": alpha.grad})
    for k, v in before.items():
        st[f"{tag}/conve/{k}"] = v
    for k, p in conve.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, k
        st[f"{tag}/g_conve/{k}"] = p.grad
    print("sf_mix3_small %s: B=%d N=%d D=%d gamma=%g loss=%.6f unsaturated TransE=%.3f ConvE=%.3f g_alpha=%s" % (
        tag, B, N, D, gamma, float(loss.detach()), frac0, frac2, alpha.grad.tolist()))


def main():
    _install_standins()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    st = {}
    for i, (tag, shape) in enumerate(CASES.items()):
        case(tag, *shape, 41 + i, st)
    np.savez_compressed(os.path.join(OUT, "sf_mix3_small.npz"), **npify(st))


if __name__ == "__main__":
    main()
