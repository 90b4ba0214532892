#!/usr/bin/env python3
"""Generate architect_tiny.npz / architect_d24.npz by RUNNING THE REFERENCE's search loop: models/architect_lp.Architect (first-order
step) and the body of search/mr_lp_search.py:train() (lines 230-253) on models/model_search_lp.Network, through the stand-ins of
make_golden.py (which stays as it is; see its docstring for what the stand-ins supply and where to run this).

    python tests/golden/make_golden_architect.py

Per case: one seeded knowledge graph, its first three quarters the training set and the rest the validation set, ONE sampled step
graph of each (kept for all epochs), three epochs with warm_epochs = 0:

    architect.step(train ..., val ..., optimizer, lr, unrolled=False)      Adam(betas (0.5, 0.999)) on the alphas, validation sample
    loss = get_loss(model(train ...)); loss.backward()                     on top of the validation gradients the architect left
    clip_grad_norm_(model.parameters(), grad_norm); optimizer.step(); optimizer.zero_grad()

Stored: both step graphs (train/, val/), the initial param/ and buffer/, the hyper-parameters, and per epoch e the alphas before and
after the architect step, their gradients (the score-function alpha, index 4, has none), both losses and the total gradient norm
clip_grad_norm_ reported; for epoch 0 also every weight's gradient after the architect step (gparam_val), after the training backward
(gparam_acc = validation + training, before clipping) and the weights after the step (param_after) -- in the d24 case gparam_val and
param_after for every sixteenth of the cells' parameters only (the file stays under 1 MiB), gparam_acc for all.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins, make_triples, npify  # noqa: E402

EPOCHS = 3


def sampled_step(ur, tri, sample, R, Nall, seed):
    """One draw of the reference's sampler, as search/mr_lp_search.py:193-226 prepares it."""
    adj, deg = ur.get_adj_and_degrees(Nall, tri)
    np.random.seed(seed)
    with np.errstate(divide="ignore"):
        g, node_id, src_in, edge_type, node_norm, data, labels = ur.generate_sampled_graph_and_labels(tri, sample, 0.5, R, adj, deg, 2, "uniform")
    g2 = g.local_var()
    g2.ndata["norm"] = torch.from_numpy(node_norm).view(-1, 1)
    g2.apply_edges(lambda edges: {"norm": edges.dst["norm"] * edges.src["norm"]})
    g.edata["norm"] = g2.edata["norm"]
    src, dst, _ = g.edges(form="all")
    stored = {"src": src, "dst": dst, "norm": g.edata["norm"], "node_id": node_id, "src_in": src_in, "edge_type": edge_type,
              "data": data, "labels": labels}
    call = (g, torch.from_numpy(node_id).view(-1, 1).long(), torch.from_numpy(src_in), torch.from_numpy(edge_type),
            torch.from_numpy(data), torch.from_numpy(labels))
    return stored, call


def case_architect(name, Nall, T, R, D, D0, nbase, layers, sample, seed, seed_train, seed_val, straddle=True, every=1):
    """every: of the cells' parameters, gparam_val and param_after are stored for each `every`-th only (gparam_acc for all): a case whose
    weights are large keeps its file under the repository's 1 MiB limit."""
    import models.model_search_lp as MS
    from models.architect_lp import Architect
    import utils.utils as UU
    import utils.utils_rgcn as ur
    hyper = dict(lr=0.01, momentum=0.9, weight_decay=0.0, grad_norm=5.0, arch_learning_rate=3e-4, arch_weight_decay=1e-5)
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    tri = make_triples(Nall, T, R, rng, dup=0)
    n_train = T * 3 // 4
    st = {"Nall": Nall, "R": R, "D": D, "D0": D0, "nbase": nbase, "layers": layers, "epochs": EPOCHS}
    st.update({k: np.float64(v) for k, v in hyper.items()})
    tr_st, train = sampled_step(ur, tri[:n_train], sample, R, Nall, seed_train)
    va_st, val = sampled_step(ur, tri[n_train:], sample, R, Nall, seed_val)
    st.update({"train/" + k: v for k, v in tr_st.items()})
    st.update({"val/" + k: v for k, v in va_st.items()})
    net = MS.Network("cpu", Nall, R, layers, 1, 2, 2, D, D0, nbase, 9.0, 0.0, 0.0)
    net.apply(UU.weights_init)
    net.train()
    for n, p in net.named_parameters():
        st[f"param/{n}"] = p.detach().clone()
    for n, b in net.named_buffers():
        st[f"buffer/{n}"] = b.detach().clone()
    optimizer = torch.optim.SGD(net.parameters(), hyper["lr"], momentum=hyper["momentum"], weight_decay=hyper["weight_decay"])
    args = types.SimpleNamespace(momentum=hyper["momentum"], weight_decay=hyper["weight_decay"],
                                 arch_learning_rate=hyper["arch_learning_rate"], arch_weight_decay=hyper["arch_weight_decay"])
    architect = Architect("cpu", net, args)
    kept = {n for i, (n, _) in enumerate(net.named_parameters()) if not n.startswith("cells.") or i % every == 0}
    norms = []
    for e in range(EPOCHS):
        for i, a in enumerate(net.arch_parameters()):
            st[f"e{e}/alpha_before/{i}"] = a.detach().clone()
        architect.step(*train, *val, optimizer, hyper["lr"], unrolled=False)          # (eta, optimizer) swapped, as the driver passes them
        for i, a in enumerate(net.arch_parameters()):
            st[f"e{e}/alpha_after/{i}"] = a.detach().clone()
            if i < 4:
                st[f"e{e}/galpha/{i}"] = a.grad.detach().clone()
        assert net.arch_parameters()[4].grad is None, "the score-function alpha received a gradient"
        st[f"e{e}/arch_loss"] = architect.loss.detach().clone()
        if e == 0:
            for n, p in net.named_parameters():
                assert p.grad is not None, f"{n}: the architect step left no validation gradient"
                if n in kept:
                    st[f"e0/gparam_val/{n}"] = p.grad.detach().clone()
        g, node_id, src_in, edge_type, data, labels = train
        ent, rel = net(g, node_id, src_in, edge_type)
        loss = net.get_loss(g, ent, rel, data, labels)
        loss.backward()
        if e == 0:
            for n, p in net.named_parameters():
                st[f"e0/gparam_acc/{n}"] = p.grad.detach().clone()
        total = torch.nn.utils.clip_grad_norm_(net.parameters(), hyper["grad_norm"])
        optimizer.step()
        if e == 0:
            for n, p in net.named_parameters():
                if n in kept:
                    st[f"e0/param_after/{n}"] = p.detach().clone()
        optimizer.zero_grad()
        st[f"e{e}/loss"] = loss.detach().clone()
        st[f"e{e}/grad_norm"] = total.detach().clone()
        norms.append(float(total))
    # both sides of the clip are pinned (straddle=False: at these sizes the norm stays above the bound for all three epochs, whatever the
    # seeds -- 7.8 .. 25 over fourteen pairs tried -- so that case pins the clipped side only)
    assert max(norms) > hyper["grad_norm"], f"architect_{name}: gradient norms {norms} never reach the clip"
    assert not straddle or max(norms) > hyper["grad_norm"] > min(norms), f"architect_{name}: gradient norms {norms} do not straddle {hyper['grad_norm']}: other seeds"
    path = os.path.join(OUT, f"architect_{name}.npz")
    np.savez_compressed(path, **npify(st))
    print("wrote architect_%s: n=%d/%d grad norms %s losses %s (%d bytes)" % (
        name, len(tr_st["node_id"]), len(va_st["node_id"]), ["%.3f" % v for v in norms],
        ["%.5f" % float(st[f"e{e}/loss"]) for e in range(EPOCHS)], os.path.getsize(path)))


def main():
    _install_standins()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    case_architect("tiny", 80, 400, 5, 8, 6, 11, 2, 60, 61, 61, 62)
    case_architect("d24", 150, 900, 9, 24, 12, 19, 2, 120, 63, 63, 64, straddle=False, every=16)


if __name__ == "__main__":
    main()
