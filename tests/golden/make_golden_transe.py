#!/usr/bin/env python3
"""Generate the TransE fixture under tests/golden/ by RUNNING THE REFERENCE (see make_golden.py for the stand-ins and the rules).

    python tests/golden/make_golden_transe.py

  fixednet_transe   models.model_lp.Network with the README genotype's cell and score_func='sf_TransE', small D: one training step
                    (BCE loss against random labels, backward), then one eval-mode forward.

The reference's gamma = 40 is sized for D = 200 embeddings; at this size every prediction would saturate to 1.  gamma is therefore set
to the rounded median L1 distance of the batch (found by one forward without gradients), so that the predictions spread over (0, 1);
it is recorded in the fixture together with the fraction of cells with 0.01 < pred < 0.99.  The width is D = 8: the spread of
the distances grows with D (at D = 32 only a fifth of the cells stay unsaturated around any one gamma, at D = 8 seven in eight).
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins, graph_train_order, make_triples, npify  # noqa: E402

TRANSE_GENOTYPE = ("[Genotype(alpha_cell=[('pre_sub', 1, 0), ('f_sparse_comp', 2, 1), ('f_sparse_comp', 3, 2), ('a_max', 4, 2), "
                   "('a_max', 5, 3), ('f_sparse_last', 6, 5), ('f_sparse_last', 7, 5)], concat_node=[4, 5, 6, 7], score_func='sf_TransE')]")


def case_fixed_net(N=37, T=101, R=5, D=8, D0=6, nbase=4, seed=29):
    from configs.genotypes import Genotype  # noqa: F401  (used by eval)
    import models.model_lp as ML
    import utils.utils as UU
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    tri = make_triples(N, T, R, rng, dup=0)
    g = graph_train_order(N, R, tri)
    genotype = eval(TRANSE_GENOTYPE)
    args = types.SimpleNamespace(feature_dim=D, drop_aggr=0.0, drop_op=0.0, gamma=40.0, embed_dim=D, conve_hid_drop=0.0,
                                 feat_drop=0.0, num_filt=6, ker_sz=3, k_w=4, k_h=8)
    net = ML.Network("cpu", genotype, N, R, D, D0, nbase, torch.nn.BCELoss(), 0.0, args)
    net.apply(UU.weights_init)
    st = {"N": N, "R": R, "D": D, "D0": D0, "nbase": nbase, "genotype": TRANSE_GENOTYPE}
    for n, b in net.named_buffers():
        st[f"buffer0/{n}"] = b.clone()
    net.train()
    B = 7
    subj = torch.from_numpy(rng.integers(0, N, size=B))
    rel = torch.from_numpy(rng.integers(0, 2 * R, size=B))
    label = (torch.rand(B, N) < 0.1).float()
    for n, p in net.named_parameters():
        st[f"param/{n}"] = p.detach().clone()
    # gamma: the rounded median batch distance, from a forward that leaves the network as it was (the buffers are put back)
    saved = {n: b.clone() for n, b in net.named_buffers()}
    net.score_func.gamma = 0.0                                 # pred = sigmoid(-dist): float32 resolves distances up to ~87
    with torch.no_grad():
        p0 = net(g, subj, rel).double()
        assert float(p0.min()) > 0 and float(p0.max()) < 1
        dist = -torch.log(p0 / (1 - p0))
    for n, b in net.named_buffers():
        b.copy_(saved[n])
    gamma = float(torch.round(dist.median()))
    assert gamma > 0
    net.score_func.gamma = gamma
    pred = net(g, subj, rel)
    loss = net.criterion(pred, label)
    loss.backward()
    frac = float(((pred > 0.01) & (pred < 0.99)).float().mean())
    assert frac > 0.5, frac
    src, dst, _ = g.edges(form="all")
    st.update({"src": src, "dst": dst, "etype": g.edata["e_type"], "norm": g.edata["norm"], "subj": subj, "rel": rel, "label": label,
               "pred": pred, "loss": loss, "gamma": np.array(gamma), "unsaturated_fraction": np.array(frac)})
    for n, p in net.named_parameters():
        st[f"gparam/{n}"] = p.grad if p.grad is not None else torch.zeros_like(p)
    for n, b in net.named_buffers():
        st[f"buffer/{n}"] = b
    net.eval()
    with torch.no_grad():
        st["pred_eval"] = net(g, subj, rel)
    np.savez_compressed(os.path.join(OUT, "fixednet_transe.npz"), **npify(st))
    print("wrote fixednet_transe gamma=%g loss=%.6f unsaturated=%.3f" % (gamma, float(loss), frac))


def main():
    _install_standins()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    case_fixed_net()


if __name__ == "__main__":
    main()
