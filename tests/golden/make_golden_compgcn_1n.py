#!/usr/bin/env python3
"""Generate tests/golden/compgcn_conve_1n.npz by RUNNING THE REFERENCE (see make_golden.py for the stand-ins and the rules).

    python tests/golden/make_golden_compgcn_1n.py

models.compgcn.CompGCN_ConvE on the shape of make_golden_conve.py's case_compgcn (N = 45, R = 6, Din = 12, Dout = 20, B = 7, dropout 0,
BatchNorm gains / biases, linear biases and the score bias moved off their defaults), with the one difference that the labels come from
a triple list through the reference's own label code -- utils.process_data.process and utils.data_set.TrainDataset with label
smoothing 0.1 -- so that a test can rebuild them with sampler.LabelIndex (conve_compgcn_small's labels are random and cannot be).
One training step (BCE loss, backward), then one eval-mode forward, which reads the running statistics the step left.

Asserted here (the seed is fixed so that they hold): the batch's (subject, relation) keys are distinct, at least one batch row asks for
heads (rel >= R), and no two eval-mode predictions of a row are equal, so the ranks expected from pred_eval have no ties.
"""
import inspect
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins, graph_train_order, make_triples, npify  # noqa: E402
from make_golden_conve import _exercise, _state  # noqa: E402


def case_compgcn_1n(N=45, T=160, R=6, Din=12, Dout=20, B=7, label_smooth=0.1, seed=11):
    import models.compgcn as C
    from utils.data_set import TrainDataset
    from utils.process_data import process
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 7)
    tri = make_triples(N, T, R, rng)
    g = graph_train_order(N, R, tri)
    E = g.num_edges()
    g.edata["etype"] = g.edata.pop("e_type")
    m = torch.zeros(E, dtype=torch.bool)
    m[: E // 2] = True
    g.edata["in_edges_mask"] = m
    g.edata["out_edges_mask"] = ~m
    src, dst, _ = g.edges(form="all")
    k_w, k_h, ks, F, nb = 4, 5, 3, 6, 3
    net = C.CompGCN_ConvE(nb, 2 * R, N, Din, [Dout], comp_fn="sub", batchnorm=True, dropout=0.0, layer_dropout=[0.0], num_filt=F,
                          hid_drop=0.0, feat_drop=0.0, ker_sz=ks, k_w=k_w, k_h=k_h)
    _exercise(net, gen)
    assert float(net.bias.detach().abs().max()) > 0
    st = {"N": N, "R": R, "Din": Din, "Dout": Dout, "nb": nb, "k_w": k_w, "k_h": k_h, "ks": ks, "F": F, "src": src, "dst": dst,
          "etype": g.edata["etype"], "norm": g.edata["norm"], "in_edges_mask": m, "label_smooth": label_smooth,
          "signature": str(inspect.signature(C.CompGCN_ConvE.__init__))}
    _state(st, "param0", net)

    # the reference's labels: process() -> one training item per known (subject, relation) pair, both directions; TrainDataset
    # smooths them.  The batch is B of those items, so its keys are distinct by construction (asserted all the same).
    triplets = process({"train": [tuple(t) for t in tri.tolist()], "valid": [], "test": []}, R)
    data = TrainDataset(triplets["train"], N, types.SimpleNamespace(lbl_smooth=label_smooth))
    pick = rng.choice(len(data), size=B, replace=False)
    items = [data[int(i)] for i in pick]
    triple = torch.stack([t for t, _ in items])
    label = torch.stack([y for _, y in items])
    subj, rel = triple[:, 0].clone(), triple[:, 1].clone()
    assert len({(int(s), int(r)) for s, r in zip(subj, rel)}) == B, "the batch's keys must be distinct"
    assert int((rel >= R).sum()) >= 1 and int((rel < R).sum()) >= 1, "both directions must be in the batch"
    # an evaluation target per row: the row's smallest known object (the training items carry object -1)
    eval_obj = torch.tensor([min(triplets["train"][int(i)]["label"]) for i in pick], dtype=torch.long)

    net.train()
    pred = net(g, subj, rel)
    loss = torch.nn.functional.binary_cross_entropy(pred, label)
    loss.backward()
    st.update(triples=tri, subj=subj, rel=rel, eval_obj=eval_obj, label=label, pred=pred, loss=loss)
    for n, p in net.named_parameters():
        st[f"gparam/{n}"] = p.grad if p.grad is not None else torch.zeros_like(p)
        st[f"pshape/{n}"] = np.array(p.shape)
    assert float(st["gparam/bias"].abs().max()) > 0
    for n, b in net.named_buffers():
        st[f"buffer/{n}"] = b
    net.eval()
    with torch.no_grad():
        pred_eval = net(g, subj, rel)
    for row in pred_eval:
        assert torch.unique(row).numel() == N, "two eval-mode predictions of a row are equal: the expected ranks would have ties"
    st["pred_eval"] = pred_eval
    np.savez_compressed(os.path.join(OUT, "compgcn_conve_1n.npz"), **npify(st))
    print("wrote compgcn_conve_1n: N=%d E=%d loss=%.6f rel=%s" % (N, E, float(loss), rel.tolist()))


def main():
    _install_standins()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    case_compgcn_1n()


if __name__ == "__main__":
    main()
