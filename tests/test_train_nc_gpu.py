"""train_nc on the MI355X: train_epoch and search_epoch with the HIP networks against hand-written copies of the reference's loops
(tests/test_train_nc_cpu.py) from identical copies of the model and the optimiser, and the host reads of an epoch counted.

Both sides are HIP runs of the same network on the same batches, so the returned triples meet close()'s defaults and the
parameters after the epochs rtol 2e-3, atol 5e-6 (the bound grads_close uses); no tighter bound can be derived."""
import sys

import pytest
import torch

from conftest import load_golden
from test_nc_cpu import close, make_net
import test_nc_search_cpu as SC
from test_train_nc_cpu import reference_search, reference_train, small_graph

from mr_gnas_amd import architect_nc as AN, train_nc as TN

pytestmark = pytest.mark.gpu
DEV = "cuda"


class ReadCounter:
    """Counts the Python-level calls of Tensor.item / tolist / cpu and the file and function they were made from."""

    def __init__(self, monkeypatch):
        self.calls = []
        for nm in ("item", "tolist", "cpu"):
            monkeypatch.setattr(torch.Tensor, nm, self.wrap(nm, getattr(torch.Tensor, nm)))

    def wrap(self, nm, fn):
        def counted(t, *a, **k):
            f = sys._getframe(1).f_code
            self.calls.append((nm, f.co_filename.rsplit("/", 1)[-1], f.co_name))
            return fn(t, *a, **k)
        return counted

    def check(self, epochs):
        mine = [c for c in self.calls if c[1] in ("train_nc.py", "architect_nc.py")]
        assert mine == [("tolist", "train_nc.py", "result")] * epochs, mine


class ConstantSchedule:
    """What the epoch functions need of a scheduler: step() once per epoch, get_last_lr() for the reference loop's `eta`."""

    def __init__(self, lr):
        self.lr, self.steps = lr, 0

    def get_last_lr(self):
        return [self.lr]

    def step(self):
        self.steps += 1


def params_close(a, b, what):
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=2e-3, atol=5e-6, msg=lambda m: f"{what} {n}: {m}")


def test_train_epochs_against_the_reference_loop(monkeypatch):
    z, tag = load_golden("nc_fixednet_small"), "n0"
    layers = int(z[tag + "/args"][8])
    g = small_graph(z, tag).to(DEV)
    trip, labels = z[tag + "/trip_index"].to(DEV), z[tag + "/labels"].to(DEV)
    nids = torch.unique(z[tag + "/gdst"].long())[:22]
    inv_target = torch.arange(int(z[tag + "/args"][0]), device=DEV)
    out = {}
    for which in ("here", "reference"):
        net = make_net(z, tag, DEV)
        opt = torch.optim.SGD(net.parameters(), 0.01, momentum=0.9)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        loader = TN.NodeLoader(g, nids, layers, batch_size=5, shuffle=True, generator=torch.Generator().manual_seed(4))
        crit = torch.nn.CrossEntropyLoss()
        if which == "here":
            counter = ReadCounter(monkeypatch)
            triples = [TN.train_epoch(net, opt, trip, loader, labels, inv_target, crit, sched) for _ in range(2)]
            counter.check(2)
            monkeypatch.undo()
            ev = TN.infer_epoch(net, trip, TN.NodeLoader(g, nids, layers, 5), labels)
            assert ev[0] == ev[1] and 0.0 <= ev[0] <= 1.0
        else:
            triples = [reference_train(trip, loader, labels, inv_target, net, opt, sched, crit) for _ in range(2)]
        out[which] = (triples, net)
    for e, (a, b) in enumerate(zip(out["here"][0], out["reference"][0])):
        print(f"epoch {e}: train_epoch {a}, reference loop {b}")
        close(torch.tensor(a), torch.tensor(b), f"train epoch {e} (macro, micro, loss)")
    params_close(out["here"][1], out["reference"][1], "after two epochs")


def test_search_epochs_against_the_reference_loop(monkeypatch):
    from mr_gnas_amd.optim import ClippedSGD
    z16, z = load_golden(SC.CASES["s16"]), load_golden("nc_search_small")
    layers = int(z16["s16/args"][8])
    g = small_graph(z16, "s16").to(DEV)
    trip, labels = z16["s16/trip_index"].to(DEV), z16["s16/labels"].to(DEV)
    out = {}
    for which in ("here", "reference"):
        net = SC.make_net(z16, "s16", DEV).train()
        opt = ClippedSGD(net.parameters(), float(z["lr"]), momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]), max_norm=0)
        sched = ConstantSchedule(float(z["lr"]))               # (ClippedSGD is no torch Optimizer: torch's schedulers refuse it)
        architect = AN.Architect(DEV, net, SC.search_args(z))
        loader, val_loader = TN.NodeLoader(g, z["train/seeds"].long(), layers, 5), TN.NodeLoader(g, z["val/seeds"].long(), layers, 5)
        crit = torch.nn.CrossEntropyLoss()
        if which == "here":
            counter = ReadCounter(monkeypatch)
            triples = [TN.search_epoch(net, architect, opt, trip, loader, val_loader, labels, e, 0, None, crit, sched) for e in range(2)]
            counter.check(2)
            monkeypatch.undo()
        else:
            triples = [reference_search(trip, loader, val_loader, labels, net, architect, opt, sched, e, 0, crit) for e in range(2)]
        assert sched.steps == 2                                           # once per epoch
        assert triples[0][2] == 1.0 and triples[1][2] != 1.0              # the stale 1.0 of the warm-up epoch, then the architect's loss
        out[which] = (triples, net)
    for e, (a, b) in enumerate(zip(out["here"][0], out["reference"][0])):
        print(f"epoch {e}: search_epoch {a}, reference loop {b}")
        close(torch.tensor(a), torch.tensor(b), f"search epoch {e} (acc, loss, arch loss)")
    params_close(out["here"][1], out["reference"][1], "after two search epochs")
    for i, (a, b) in enumerate(zip(out["here"][1].arch_parameters(), out["reference"][1].arch_parameters())):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=2e-3, atol=5e-6, msg=lambda m: f"alpha {i}: {m}")
