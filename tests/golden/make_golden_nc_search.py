#!/usr/bin/env python3
"""Generate the node-classification SEARCH fixtures under tests/golden/ by RUNNING THE REFERENCE: ``models/model_search.Network``
(with ``models/cell.py``), ``models/architect.Architect`` and the batch body of ``search/mr_nc_search.py:train()`` run as they are on
the stand-ins of make_golden.py / make_golden_nc.py (which stay untouched; see their docstrings for what the stand-ins supply).

    python tests/golden/make_golden_nc_search.py

Every file stores arrays and JSON strings only, and stays below 1 MiB.

  nc_supernet_small   case s16: N 160, 700 triples, 6 relations, 4 classes, D 16, init_fea_dim 8, 5 bases, 2 layers, nodes 3,
                      12 seeds.  One training step (cross-entropy on random labels, backward), then one eval-mode forward.
                      Stored (tensor collections packed, see pack()): param0 (the whole state_dict), the state keys, the alphas, logits, loss, EVERY parameter gradient, the
                      four alpha gradients, every buffer after the step, the eval logits, repr(show_genotypes()).
  nc_supernet_s64     case s64: D 64, 1 layer, nodes 2, a block of more than 128 edge rows (not a multiple of 32).  The same
                      quantities.  The 310 010 parameters and as many gradients do not fit one file below 1 MiB: the floating-point
                      state is rounded to float16 BEFORE the reference runs and stored as float16 (exact), and EVERY parameter
                      gradient (float32) goes to nc_supernet_s64_grads0 / _grads1, half of the values each.
  nc_search_small     three passes of the train() body on the shapes (and from the param0) of case s16 with separate training and
                      validation blocks, warm_epochs = -1: per pass the alphas before and after the architect step, their gradients
                      and both losses; for pass 0 every weight's gradient after the training backward and the weights after the step.
  nc_search_small_weights   the weights at the start of passes 1 and 2 of nc_search_small.  One ReLU or arg-max decision that falls
                      the other way (a BatchNorm output within rounding of 0) changes the gradients behind it by a finite amount, and
                      the reference itself does this under a one-ulp change of its weights (`--sensitivity` measures it: the pass-1
                      alpha gradients then move by 1.1e-5 in 8 of 23 such runs, by 1e-6 or less in the others); a test that lets its own weights drift over the passes would
                      compare two different decision patterns.  The tests reset the weights, like the alphas, from the fixture.

Set-up of every case: all 1-D parameters moved away from 0 / 1 (BatchNorm gains 1 + 0.1 randn; BatchNorm and Linear biases
0.1 randn), alphas 0.5 randn so that the softmax weights differ.
"""
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, npify  # noqa: E402
from make_golden_nc import _install_nc_standins, _store_blocks, full_neighbor_blocks  # noqa: E402

PASSES = 3


def pack(st, prefix, named, half=False):
    """{name: tensor} as ONE array per kind (an .npz member costs ~200 bytes of headers, and a supernet has thousands of tensors):
    prefix/index = JSON [[name, shape, "f" | "i"], ...], prefix/f = the floating-point tensors flattened and concatenated in index
    order (float16 when half: exact for values rounded to float16 beforehand), prefix/i = the integer ones (int64)."""
    named = [(n, t.detach()) for n, t in named]
    index = [[n, list(t.shape), "f" if t.is_floating_point() else "i"] for n, t in named]
    fl = [t.reshape(-1).float() for n, t in named if t.is_floating_point()]
    it = [t.reshape(-1).long() for n, t in named if not t.is_floating_point()]
    st[prefix + "/index"] = np.array(json.dumps(index))
    f = torch.cat(fl) if fl else torch.zeros(0)
    st[prefix + "/f"] = f.half() if half else f
    st[prefix + "/i"] = torch.cat(it) if it else torch.zeros(0, dtype=torch.long)


def make_graph(rng, N, T, R, classes):
    src, dst = rng.integers(0, N, T), rng.integers(0, N, T)
    src[:3], dst[:3] = 5, 7                                          # a duplicated edge
    etype = rng.integers(0, R, T)
    trip_index = torch.stack([torch.arange(T), torch.as_tensor(src), torch.as_tensor(dst)], dim=1)
    labels = torch.as_tensor(rng.integers(0, classes, N))
    return src, dst, etype, trip_index, labels


def make_net(MS, gen, N, classes, R, layers, nodes, D, D0, nbase, half=False):
    net = MS.Network(torch.device("cpu"), N, classes, R, layers, 1, nodes, D, D0, nbase)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
            elif isinstance(m, torch.nn.Linear) and m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
        for a in net.arch_parameters():
            a.copy_(0.5 * torch.randn(a.shape, generator=gen))
        if half:
            for p in net.parameters():
                p.copy_(p.half().float())
    return net


def supernet_case(st, tag, seed, N=160, T=700, R=6, classes=4, D=16, D0=8, nbase=5, batch=12, layers=2, nodes=3, half=False, grad_parts=None):
    import models.model_search as MS
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    src, dst, etype, trip_index, labels = make_graph(rng, N, T, R, classes)
    seeds = rng.choice(N, batch, replace=False)
    blocks = full_neighbor_blocks(src, dst, etype, seeds, layers)
    net = make_net(MS, gen, N, classes, R, layers, nodes, D, D0, nbase, half)
    n_par = sum(p.numel() for p in net.parameters())
    st.update({f"{tag}/args": np.array([N, T, R, classes, D, D0, nbase, batch, layers, nodes]),
               f"{tag}/gsrc": src, f"{tag}/gdst": dst, f"{tag}/getype": etype, f"{tag}/seeds": seeds, f"{tag}/trip_index": trip_index,
               f"{tag}/labels": labels, f"{tag}/state_keys": np.array(json.dumps(list(net.state_dict().keys()))),
               f"{tag}/n_parameters": np.array(n_par)})
    _store_blocks(st, f"{tag}/blocks", blocks)
    pack(st, f"{tag}/param0", [(n, p.clone()) for n, p in net.state_dict().items()], half)
    for i, a in enumerate(net.arch_parameters()):
        st[f"{tag}/alpha/{i}"] = a.detach().clone()
    net.train()
    logits = net(trip_index, blocks)
    loss = net._criterion(logits, labels[torch.as_tensor(seeds)])
    loss.backward()
    st.update({f"{tag}/logits": logits, f"{tag}/loss": loss})
    named = [(n, p.grad) for n, p in net.named_parameters() if p.grad is not None]
    if grad_parts is None:
        pack(st, f"{tag}/gparam", named)
    else:                                                            # every gradient, over several files of about equal size
        total, done, k = sum(g.numel() for _, g in named), 0, 0
        parts = [[] for _ in grad_parts]
        for n, g in named:
            parts[min(len(parts) - 1, done * len(parts) // total)].append((n, g))
            done += g.numel()
        for part_st, part in zip(grad_parts, parts):
            pack(part_st, f"{tag}/gparam", part)
    st[f"{tag}/no_grad_names"] = np.array(json.dumps([n for n, p in net.named_parameters() if p.grad is None]))
    for i, a in enumerate(net.arch_parameters()):
        st[f"{tag}/galpha/{i}"] = a.grad
    pack(st, f"{tag}/buffer", [(n, b.clone()) for n, b in net.named_buffers()])
    net.eval()
    with torch.no_grad():
        st[f"{tag}/logits_eval"] = net(trip_index, blocks)
    st[f"{tag}/genotypes"] = np.array(repr(net.show_genotypes()))
    E = [int(b._src.numel()) for b in blocks]
    print(f"  {tag}: {n_par} parameters, E per block {E}, destinations {[b.number_of_dst_nodes() for b in blocks]}, loss={float(loss.detach()):.6f}")
    return E, net


def case_supernet():
    _install_nc_standins()
    st = {}
    supernet_case(st, "s16", 41)
    path = os.path.join(OUT, "nc_supernet_small.npz")
    np.savez_compressed(path, **npify(st))
    print(f"wrote nc_supernet_small ({os.path.getsize(path)} bytes)")
    st = {}
    grads = [{}, {}]
    E, _ = supernet_case(st, "s64", 42, D=64, batch=40, layers=1, nodes=2, half=True, grad_parts=grads)
    assert E[0] > 128 and E[0] % 32 != 0, f"s64: {E[0]} edge rows: other seeds"
    for name, d in [("nc_supernet_s64", st)] + [(f"nc_supernet_s64_grads{i}", g) for i, g in enumerate(grads)]:
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **npify(d))
        print(f"wrote {name} ({os.path.getsize(path)} bytes)")


def case_search(seed=41, seed_blocks=43, N=160, T=700, R=6, classes=4, D=16, D0=8, nbase=5, batch=12, layers=2, nodes=3):
    """Starts from the graph and the param0 of case s16 (same seed, same construction): the file stores neither again."""
    import models.model_search as MS
    from models.architect import Architect
    hyper = dict(lr=0.005, momentum=0.9, weight_decay=3e-4, arch_learning_rate=3e-4, arch_weight_decay=1e-3, warm_epochs=-1)
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    src, dst, etype, trip_index, labels = make_graph(rng, N, T, R, classes)
    rng.choice(N, batch, replace=False)                              # (case s16's seeds: keeps the generator in step)
    net = make_net(MS, gen, N, classes, R, layers, nodes, D, D0, nbase)
    with np.load(os.path.join(OUT, "nc_supernet_small.npz")) as z16:      # the test takes param0 and the graph from there
        assert np.array_equal(z16["s16/param0/f"], torch.cat([p.reshape(-1) for p in net.state_dict().values() if p.is_floating_point()]).numpy()), \
            "not the param0 of case s16"
        for i, a in enumerate(net.arch_parameters()):
            assert np.array_equal(z16[f"s16/alpha/{i}"], a.detach().numpy())
    rb = np.random.default_rng(seed_blocks)
    perm = rb.permutation(N)
    seeds_tr, seeds_va = perm[:batch], perm[batch:2 * batch]
    blocks_tr = full_neighbor_blocks(src, dst, etype, seeds_tr, layers)
    blocks_va = full_neighbor_blocks(src, dst, etype, seeds_va, layers)
    st = {"passes": PASSES, "train/seeds": seeds_tr, "val/seeds": seeds_va}
    st.update({k: np.float64(v) for k, v in hyper.items()})
    _store_blocks(st, "train/blocks", blocks_tr)
    _store_blocks(st, "val/blocks", blocks_va)
    optimizer = torch.optim.SGD(net.parameters(), hyper["lr"], momentum=hyper["momentum"], weight_decay=hyper["weight_decay"])
    args = types.SimpleNamespace(momentum=hyper["momentum"], weight_decay=hyper["weight_decay"],
                                 arch_learning_rate=hyper["arch_learning_rate"], arch_weight_decay=hyper["arch_weight_decay"])
    architect = Architect("cpu", net, args)
    criterion = torch.nn.CrossEntropyLoss()
    s_tr, s_va = torch.as_tensor(seeds_tr), torch.as_tensor(seeds_va)
    net.train()
    stw = {}
    for e in range(PASSES):                                          # search/mr_nc_search.py:162-182, epoch e > warm_epochs = -1
        if e > 0:
            pack(stw, f"e{e}/param_before", [(n, p.clone()) for n, p in net.named_parameters()])
        for i, a in enumerate(net.arch_parameters()):
            st[f"e{e}/alpha_before/{i}"] = a.detach().clone()
        architect.step(trip_index, blocks_tr, labels, s_tr, blocks_va, s_va, hyper["lr"], optimizer, unrolled=False)
        for i, a in enumerate(net.arch_parameters()):
            st[f"e{e}/alpha_after/{i}"] = a.detach().clone()
            st[f"e{e}/galpha/{i}"] = a.grad.detach().clone()
        st[f"e{e}/arch_loss"] = architect.loss.detach().clone()
        optimizer.zero_grad()
        logits = net(trip_index, blocks_tr)
        loss = criterion(logits, labels[s_tr])
        loss.backward()
        if e == 0:
            pack(st, "e0/gparam_acc", [(n, p.grad.clone()) for n, p in net.named_parameters() if p.grad is not None])
        optimizer.step()
        if e == 0:
            pack(st, "e0/param_after", [(n, p.clone()) for n, p in net.named_parameters()])
        st[f"e{e}/loss"] = loss.detach().clone()
    path = os.path.join(OUT, "nc_search_small.npz")
    np.savez_compressed(path, **npify(st))
    pathw = os.path.join(OUT, "nc_search_small_weights.npz")
    np.savez_compressed(pathw, **npify(stw))
    print(f"wrote nc_search_small_weights ({os.path.getsize(pathw)} bytes)")
    print("wrote nc_search_small: losses %s arch losses %s (%d bytes)" % (
        ["%.5f" % float(st[f"e{e}/loss"]) for e in range(PASSES)], ["%.5f" % float(st[f"e{e}/arch_loss"]) for e in range(PASSES)],
        os.path.getsize(path)))


def sensitivity(runs=23, seed=41, seed_blocks=43, N=160, T=700, R=6, classes=4, D=16, D0=8, nbase=5, batch=12, layers=2, nodes=3):
    """Why the tests reset the weights before passes 1 and 2 (nc_search_small_weights): the reference's own alpha gradients under a
    change of its weights by at most one ulp.  Runs the three passes of case_search once as they are and `runs` times with every
    weight multiplied by 1 + {-1, 0, 1} * 2^-24 (seeded) after pass 0, and prints the largest change of the alpha gradients of
    passes 1 and 2.  A ReLU / arg-max decision at a BatchNorm output within rounding of 0 that falls the other way shows as a jump
    far above rounding (1e-5 against 1e-6 and below).

        python tests/golden/make_golden_nc_search.py --sensitivity"""
    import models.model_search as MS
    from models.architect import Architect
    args = types.SimpleNamespace(momentum=0.9, weight_decay=3e-4, arch_learning_rate=3e-4, arch_weight_decay=1e-3)

    def run(perturb_seed):
        rng = np.random.default_rng(seed)
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        src, dst, etype, trip_index, labels = make_graph(rng, N, T, R, classes)
        rng.choice(N, batch, replace=False)
        net = make_net(MS, gen, N, classes, R, layers, nodes, D, D0, nbase).train()
        perm = np.random.default_rng(seed_blocks).permutation(N)
        s_tr, s_va = torch.as_tensor(perm[:batch]), torch.as_tensor(perm[batch:2 * batch])
        b_tr = full_neighbor_blocks(src, dst, etype, perm[:batch], layers)
        b_va = full_neighbor_blocks(src, dst, etype, perm[batch:2 * batch], layers)
        optimizer = torch.optim.SGD(net.parameters(), 0.005, momentum=0.9, weight_decay=3e-4)
        architect = Architect("cpu", net, args)
        criterion = torch.nn.CrossEntropyLoss()
        galpha = []
        for e in range(PASSES):
            architect.step(trip_index, b_tr, labels, s_tr, b_va, s_va, 0.005, optimizer, unrolled=False)
            galpha.append([a.grad.clone() for a in net.arch_parameters()])
            optimizer.zero_grad()
            criterion(net(trip_index, b_tr), labels[s_tr]).backward()
            optimizer.step()
            if e == 0 and perturb_seed is not None:
                g = torch.Generator().manual_seed(perturb_seed)
                with torch.no_grad():
                    for p in net.parameters():
                        p.mul_(1 + torch.randint(-1, 2, p.shape, generator=g).float() * 2.0 ** -24)
        return galpha

    base = run(None)
    jumps = 0
    for ps in range(1, runs + 1):
        other = run(ps)
        d = [max(float((a - b).abs().max()) for a, b in zip(base[e], other[e])) for e in (1, 2)]
        jumps += max(d) > 5e-6
        print(f"  weights changed by <= 1 ulp (seed {ps}): alpha gradients move by {d[0]:.2e} in pass 1, {d[1]:.2e} in pass 2")
    print(f"sensitivity: {jumps} of {runs} runs move an alpha gradient by more than 5e-6 (largest alpha gradient "
          f"{max(float(a.abs().max()) for a in base[1]):.3f})")


def main():
    torch.set_num_threads(1)
    if "--sensitivity" in sys.argv:
        _install_nc_standins()
        sensitivity()
        return
    case_supernet()
    case_search()


if __name__ == "__main__":
    main()
