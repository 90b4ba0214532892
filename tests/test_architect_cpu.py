"""mr_gnas_amd.architect on the CPU: Architect + search_epoch driving the ORACLE supernet (oracle/nets.py behind a small adapter, the
alphas' optimiser torch.optim.Adam) against three epochs of the reference's own search loop (tests/golden/make_golden_architect.py),
and the interface of the new pieces.  No GPU."""
import inspect
import types

import pytest
import torch

from conftest import assert_param_grad, load_golden, sub
from mr_gnas_amd import _lib
from mr_gnas_amd.architect import Architect, search_epoch
from oracle import nets as ON
from oracle.graph import OGraph

REFERENCE_STEP_PARAMETERS = ["self", "g_train", "node_id", "src_in", "edge_type", "data", "labels", "g_val", "node_id_val", "src_in_val",
                             "edge_type_val", "data_val", "labels_val", "eta", "optimizer", "unrolled"]      # models/architect_lp.py:37


class OracleSupernet:
    """What Architect and search_epoch use of the reference's Network, on oracle.nets."""

    def __init__(self, z):
        self.z = z
        self.S = {k: v.clone().requires_grad_(True) for k, v in sub(z, "param/").items()}
        self.alphas = [z[f"e0/alpha_before/{i}"].clone().requires_grad_(True) for i in range(5)]

    def parameters(self):
        return list(self.S.values())

    def named_parameters(self):
        return list(self.S.items())

    def arch_parameters(self):
        return self.alphas

    def __call__(self, g, node_id, src_in, edge_type):
        return ON.supernet_forward(g, self.S, self.alphas, node_id, src_in, edge_type, 2 * self.z["R"] + 1, self.z["layers"])

    def get_loss(self, g, ent, rel, data, labels):
        return ON.distmult_bce(ent, rel, data, labels)

    def _loss(self, g, node_id, src_in, edge_type, data, labels):
        return self.get_loss(g, *self(g, node_id, src_in, edge_type), data, labels)


def step_inputs(z, which):
    n = z[which + "/node_id"].numel()
    g = OGraph(n, z[which + "/src"], z[which + "/dst"], z[which + "/edge_type"], z[which + "/norm"])
    return (g, z[which + "/node_id"], z[which + "/src_in"], z[which + "/edge_type"], z[which + "/data"], z[which + "/labels"])


def arch_args(z):
    return types.SimpleNamespace(momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]),
                                 arch_learning_rate=float(z["arch_learning_rate"]), arch_weight_decay=float(z["arch_weight_decay"]))


def as_gparam(d):
    """{name: tensor} in the layout conftest.assert_param_grad reads."""
    return {"gparam/" + k: v for k, v in d.items()}


@pytest.mark.parametrize("case", ["architect_tiny", "architect_d24"])
def test_search_epochs_on_the_oracle_match_the_reference(case, monkeypatch):
    torch.set_num_threads(1)
    z = load_golden(case)
    lr, alr = float(z["lr"]), float(z["arch_learning_rate"])
    model = OracleSupernet(z)
    optimizer = torch.optim.SGD(model.parameters(), lr, momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]))
    architect = Architect("cpu", model, arch_args(z))
    assert isinstance(architect.optimizer, torch.optim.Adam)
    train, val = step_inputs(z, "train"), step_inputs(z, "val")
    seen = {}
    adam_step = architect.optimizer.step

    def after_architect_backward(*a, **k):                  # what the validation backward left, before Adam and the training backward
        seen["galpha"] = [None if a_.grad is None else a_.grad.clone() for a_ in model.alphas]
        seen["gparam_val"] = {n: (None if p.grad is None else p.grad.clone()) for n, p in model.S.items()}
        return adam_step(*a, **k)

    clip = torch.nn.utils.clip_grad_norm_

    def before_clip(params, max_norm, *a, **k):
        assert max_norm == float(z["grad_norm"])
        seen["gparam_acc"] = {n: (None if p.grad is None else p.grad.clone()) for n, p in model.S.items()}
        return clip(params, max_norm, *a, **k)

    monkeypatch.setattr(architect.optimizer, "step", after_architect_backward)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", before_clip)
    assert sorted(sub(z, "e0/gparam_acc/")) == sorted(model.S)
    for e in range(z["epochs"]):
        with torch.no_grad():
            for i, a in enumerate(model.alphas):
                a.copy_(z[f"e{e}/alpha_before/{i}"])
        before = {n: p.detach().clone() for n, p in model.S.items()}
        loss, arch_loss = search_epoch(model, architect, optimizer, train, val, e, 0, grad_norm=float(z["grad_norm"]))
        assert torch.is_tensor(loss) and torch.is_tensor(arch_loss) and arch_loss is not None and not loss.requires_grad
        print(f"{case} epoch {e}: loss {float(loss):.7f} (ref {float(z[f'e{e}/loss']):.7f}) arch loss {float(arch_loss):.7f} "
              f"(ref {float(z[f'e{e}/arch_loss']):.7f})")
        torch.testing.assert_close(arch_loss, z[f"e{e}/arch_loss"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(loss, z[f"e{e}/loss"], rtol=1e-5, atol=1e-6)
        for i in range(4):
            ref = z[f"e{e}/galpha/{i}"]
            err = float((seen["galpha"][i] - ref).abs().max())
            assert err <= 1e-3 * max(float(ref.abs().max()), 1e-8) + 1e-8, f"epoch {e} alpha {i}: gradient err {err:.3e}"
        assert seen["galpha"][4] is None                    # the score-function alpha has no gradient: Adam skips it
        assert torch.equal(model.alphas[4].detach(), z[f"e{e}/alpha_before/4"])
        worst = 0.0
        for i in range(5):
            err = float((model.alphas[i].detach() - z[f"e{e}/alpha_after/{i}"]).abs().max())
            worst = max(worst, err)
            assert err <= 1e-3 * alr, f"epoch {e} alpha {i} after the step: err {err:.3e}"
        print(f"{case} epoch {e}: alphas after the step within {worst:.2e} (allowed {1e-3 * alr:.1e})")
        if e == 0:
            zv, za = as_gparam(sub(z, "e0/gparam_val/")), as_gparam(sub(z, "e0/gparam_acc/"))
            for n in sub(z, "e0/gparam_val/"):              # the validation gradients STAY in the weights ...
                assert_param_grad(zv, n, seen["gparam_val"][n], 1e-3, 2e-6, case + " validation")
            for n in model.S:                               # ... and the weight step is taken on validation + training
                assert_param_grad(za, n, seen["gparam_acc"][n], 1e-3, 2e-6, case + " validation+training")
            zs = as_gparam({n: (z["param/" + n] - v) / lr for n, v in sub(z, "e0/param_after/").items()})
            for n in sub(z, "e0/param_after/"):
                assert_param_grad(zs, n, (before[n] - model.S[n].detach()) / lr, 1e-3, 2e-6, case + " weight step")
        assert all(p.grad is None for p in model.S.values())      # optimizer.zero_grad() ended the epoch


def test_fixture_pins_both_sides_of_the_clip():
    z = load_golden("architect_tiny")
    norms = [float(z[f"e{e}/grad_norm"]) for e in range(z["epochs"])]
    assert max(norms) > float(z["grad_norm"]) > min(norms), norms
    assert len(sub(z, "e0/gparam_val/")) == len(sub(z, "e0/gparam_acc/")) == len(sub(z, "param/"))       # every weight keeps a validation gradient


def test_warm_up_epochs_take_no_architect_step():
    z = load_golden("architect_tiny")
    model = OracleSupernet(z)
    architect = Architect("cpu", model, arch_args(z))
    optimizer = torch.optim.SGD(model.parameters(), float(z["lr"]))
    loss, arch_loss = search_epoch(model, architect, optimizer, step_inputs(z, "train"), step_inputs(z, "val"), 1, 2)
    assert torch.equal(arch_loss, torch.ones(1))
    for i, a in enumerate(model.alphas):
        assert torch.equal(a.detach(), z[f"e0/alpha_before/{i}"])
    assert torch.isfinite(loss) and all(p.grad is None for p in model.S.values())


def test_weight_grads_false_leaves_the_weights_alone():
    z = load_golden("architect_tiny")
    model = OracleSupernet(z)
    architect = Architect("cpu", model, arch_args(z), weight_grads=False)
    train, val = step_inputs(z, "train"), step_inputs(z, "val")
    architect.step(*train, *val, None, None, False)
    assert all(p.grad is None for p in model.S.values())
    torch.testing.assert_close(architect.loss.detach(), z["e0/arch_loss"], rtol=1e-5, atol=1e-6)
    for i in range(5):
        assert float((model.alphas[i].detach() - z[f"e0/alpha_after/{i}"]).abs().max()) <= 1e-3 * float(z["arch_learning_rate"])
    assert model.alphas[4].grad is None


def test_architect_interface():
    assert list(inspect.signature(Architect.step).parameters) == REFERENCE_STEP_PARAMETERS
    z = load_golden("architect_tiny")
    model = OracleSupernet(z)
    args = arch_args(z)
    architect = Architect("cpu", model, args)
    assert architect.network_momentum == args.momentum and architect.network_weight_decay == args.weight_decay
    assert architect.model is model and architect.device == "cpu" and torch.equal(architect.loss, torch.ones(1))
    group = architect.optimizer.param_groups[0]
    assert group["lr"] == args.arch_learning_rate and tuple(group["betas"]) == (0.5, 0.999) and group["weight_decay"] == args.arch_weight_decay
    assert all(a is b for a, b in zip(group["params"], model.alphas))
    train, val = step_inputs(z, "train"), step_inputs(z, "val")
    with pytest.raises(NotImplementedError, match="model.new"):
        architect.step(*train, *val, 0.01, None, True)


def test_fused_adam_has_no_cpu_form_and_the_abi_declares_it():
    from mr_gnas_amd.optim import ClippedSGD, FusedAdam
    with pytest.raises(_lib.MrgnasError):
        FusedAdam([torch.zeros(3, requires_grad=True)])
    with pytest.raises(_lib.MrgnasError):
        ClippedSGD([torch.zeros(3, requires_grad=True)], 0.1)
    assert issubclass(FusedAdam, torch.optim.Optimizer)
    assert "mrg_adam_step" in _lib.SIGNATURES and "mrg_adam_step" in _lib.declared_symbols()
    assert _lib.ABI_VERSION >= 21
    lib = _lib.load()                                         # argument validation happens before any launch
    import ctypes
    P = ctypes.c_void_p
    tables = [P(16)] * 4
    assert lib.mrg_adam_step(*tables, 3, P(16), P(16), P(16), 0, P(16), P(16), P(16), 0.9, 0.999, 1e-8, 0.0, None) == 0      # nothing to do
    assert lib.mrg_adam_step(None, *tables[1:], 3, P(16), P(16), P(16), 5, P(16), P(16), P(16), 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert lib.mrg_adam_step(*tables, 3, P(16), P(16), P(16), 5, P(16), P(16), None, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert lib.mrg_adam_step(*tables, 3, P(16), P(16), P(16), 1 << 31, P(16), P(16), P(16), 0.9, 0.999, 1e-8, 0.0, None) == -2
