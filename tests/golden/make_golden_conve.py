#!/usr/bin/env python3
"""Generate the ConvE fixtures under tests/golden/ by RUNNING THE REFERENCE (see make_golden.py for the stand-ins and the rules).

    python tests/golden/make_golden_conve.py

Cases (dropout 0 everywhere; one training step: BCE loss against random labels, backward; then one eval-mode forward, so the
running statistics it reads are the ones the step left):
  conve_sf_small       models.operations_lp.sf_ConvE_op, the stacked image, a few shapes (odd ks * ks, a non-square image)
  conve_compgcn_small  models.compgcn.CompGCN_ConvE on the compgcn_small graph shape: the interleaved image, no conv bias, score bias
  fixednet_conve       models.model_lp.Network with the training driver's default genotype (score_func='sf_ConvE'), small D
"""
import inspect
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins, graph_train_order, make_triples, npify  # noqa: E402

SF_SHAPES = [  # tag, B, N, D, k_h, k_w, ker_sz, num_filt
    ("s0", 6, 11, 16, 8, 2, 2, 3),        # non-square image 16 x 2
    ("s1", 5, 9, 16, 4, 4, 3, 5),         # ks * ks odd
    ("s2", 7, 13, 24, 6, 4, 3, 8),
]
TRAIN_GENOTYPE = ("[Genotype(alpha_cell=[('pre_mult', 1, 0), ('f_sparse_comp', 2, 1), ('f_sparse_comp', 3, 2), ('a_max', 4, 2), "
                  "('a_max', 5, 3), ('f_sparse_last', 6, 5), ('f_sparse_last', 7, 5)], concat_node=[4, 5, 6, 7], score_func='sf_ConvE')]")


def _exercise(mod, gen):
    """BatchNorm gains / biases and linear biases away from their 1 / 0 defaults, so that their gradients are exercised."""
    for n, p in mod.named_parameters():
        if p.dim() == 1:
            with torch.no_grad():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1 + (1.0 if n.endswith("weight") else 0.0))


def _state(st, prefix, mod):
    for n, p in mod.state_dict().items():
        st[f"{prefix}/{n}"] = p.clone()


def case_sf(seed=61):
    import models.operations_lp as OL
    st = {}
    gen = torch.Generator().manual_seed(seed)
    for tag, B, N, D, k_h, k_w, ks, F in SF_SHAPES:
        torch.manual_seed(seed)
        args = {"embed_dim": D, "conve_hid_drop": 0.0, "feat_drop": 0.0, "num_filt": F, "ker_sz": ks, "k_w": k_w, "k_h": k_h}
        op = OL.sf_ConvE_op(args)
        _exercise(op, gen)
        st[f"{tag}/args"] = np.array([B, N, D, k_h, k_w, ks, F])
        _state(st, f"{tag}/param0", op)
        ent = torch.randn(N, D, generator=gen).requires_grad_(True)
        sub_e = torch.randn(B, D, generator=gen).requires_grad_(True)
        rel_e = torch.randn(B, D, generator=gen).requires_grad_(True)
        label = (torch.rand(B, N, generator=gen) < 0.3).float()
        st.update({f"{tag}/ent": ent.detach().clone(), f"{tag}/sub": sub_e.detach().clone(), f"{tag}/rel": rel_e.detach().clone(),
                   f"{tag}/label": label})
        op.train()
        pred = op(ent, sub_e, rel_e)
        loss = torch.nn.functional.binary_cross_entropy(pred, label)
        loss.backward()
        st.update({f"{tag}/pred": pred, f"{tag}/loss": loss, f"{tag}/gent": ent.grad, f"{tag}/gsub": sub_e.grad, f"{tag}/grel": rel_e.grad})
        for n, p in op.named_parameters():
            st[f"{tag}/gparam/{n}"] = p.grad
        for n, b in op.named_buffers():
            st[f"{tag}/buffer/{n}"] = b
        op.eval()
        with torch.no_grad():
            st[f"{tag}/pred_eval"] = op(ent, sub_e, rel_e)
    np.savez_compressed(os.path.join(OUT, "conve_sf_small.npz"), **npify(st))
    print("wrote conve_sf_small")


def case_compgcn(N=45, T=160, R=6, Din=12, Dout=20, seed=11):
    import models.compgcn as C
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
    k_w, k_h, ks, F, nb, B = 4, 5, 3, 6, 3, 7
    net = C.CompGCN_ConvE(nb, 2 * R, N, Din, [Dout], comp_fn="sub", batchnorm=True, dropout=0.0, layer_dropout=[0.0], num_filt=F,
                          hid_drop=0.0, feat_drop=0.0, ker_sz=ks, k_w=k_w, k_h=k_h)
    _exercise(net, gen)
    st = {"N": N, "R": R, "Din": Din, "Dout": Dout, "nb": nb, "k_w": k_w, "k_h": k_h, "ks": ks, "F": F, "src": src, "dst": dst,
          "etype": g.edata["etype"], "norm": g.edata["norm"], "in_edges_mask": m,
          "signature": str(inspect.signature(C.CompGCN_ConvE.__init__))}
    _state(st, "param0", net)
    subj = torch.from_numpy(rng.integers(0, N, size=B))
    rel = torch.from_numpy(rng.integers(0, 2 * R, size=B))
    label = (torch.rand(B, N, generator=gen) < 0.2).float()
    net.train()
    pred = net(g, subj, rel)
    loss = torch.nn.functional.binary_cross_entropy(pred, label)
    loss.backward()
    st.update(subj=subj, rel=rel, label=label, pred=pred, loss=loss)
    for n, p in net.named_parameters():
        st[f"gparam/{n}"] = p.grad if p.grad is not None else torch.zeros_like(p)
        st[f"pshape/{n}"] = np.array(p.shape)
    for n, b in net.named_buffers():
        st[f"buffer/{n}"] = b
    net.eval()
    with torch.no_grad():
        st["pred_eval"] = net(g, subj, rel)
    np.savez_compressed(os.path.join(OUT, "conve_compgcn_small.npz"), **npify(st))
    print("wrote conve_compgcn_small: N=%d E=%d loss=%.6f" % (N, E, float(loss)))


def case_fixed_net(N=37, T=101, R=5, D=32, D0=6, nbase=4, seed=23):
    from configs.genotypes import Genotype  # noqa: F401  (used by eval)
    import models.model_lp as ML
    import utils.utils as UU
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    tri = make_triples(N, T, R, rng, dup=0)
    g = graph_train_order(N, R, tri)
    genotype = eval(TRAIN_GENOTYPE)
    k_h, k_w, ks, F = 8, 4, 3, 6
    args = types.SimpleNamespace(feature_dim=D, drop_aggr=0.0, drop_op=0.0, gamma=40.0, embed_dim=D, conve_hid_drop=0.0,
                                 feat_drop=0.0, num_filt=F, ker_sz=ks, k_w=k_w, k_h=k_h)
    net = ML.Network("cpu", genotype, N, R, D, D0, nbase, torch.nn.BCELoss(), 0.0, args)
    net.apply(UU.weights_init)
    _exercise(net.score_func, torch.Generator().manual_seed(seed + 1))
    st = {"N": N, "R": R, "D": D, "D0": D0, "nbase": nbase, "genotype": TRAIN_GENOTYPE,
          "score_args": np.array([D, F, ks, k_w, k_h])}
    for n, b in net.named_buffers():
        st[f"buffer0/{n}"] = b.clone()
    net.train()
    B = 7
    subj = torch.from_numpy(rng.integers(0, N, size=B))
    rel = torch.from_numpy(rng.integers(0, 2 * R, size=B))
    label = (torch.rand(B, N) < 0.1).float()
    for n, p in net.named_parameters():
        st[f"param/{n}"] = p.detach().clone()
    pred = net(g, subj, rel)
    loss = net.criterion(pred, label)
    loss.backward()
    src, dst, _ = g.edges(form="all")
    st.update({"src": src, "dst": dst, "etype": g.edata["e_type"], "norm": g.edata["norm"], "subj": subj, "rel": rel, "label": label,
               "pred": pred, "loss": loss})
    for n, p in net.named_parameters():
        st[f"gparam/{n}"] = p.grad if p.grad is not None else torch.zeros_like(p)
    for n, b in net.named_buffers():
        st[f"buffer/{n}"] = b
    net.eval()
    with torch.no_grad():
        st["pred_eval"] = net(g, subj, rel)
    np.savez_compressed(os.path.join(OUT, "fixednet_conve.npz"), **npify(st))
    print("wrote fixednet_conve loss=%.6f" % float(loss))


def main():
    _install_standins()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    case_sf()
    case_compgcn()
    case_fixed_net()


if __name__ == "__main__":
    main()
