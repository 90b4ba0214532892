"""mr_gnas_amd.architect_unrolled on the CPU (no GPU): the engine on its torch path against a LITERAL restatement of the reference's
``_backward_step_unrolled`` (models/architect_lp.py:26-103, models/architect.py:23-99), in float64.

The restatement below makes a copy where the reference calls ``model.new()`` (which cannot run), then follows the reference line by
line: ``_compute_unrolled_model``, the validation backward on the copy, ``_hessian_vector_product`` with its add / sub / add on the
original, ``g.data.sub_(eta, ig.data)``.  One more necessary difference: the reference's ``torch.autograd.grad(loss, arch_parameters())``
raises for an alpha the loss does not reach (the score-function alpha); the restatement passes allow_unused=True and skips it.

Link prediction runs on the CPU ORACLE supernet (oracle/nets.py behind tests/test_architect_cpu.py's adapter, re-declared here for
float64); node classification on the package's CPU supernet in float64 (tests/test_nc_search_cpu.make_net64: that path accepts
float64) against a ``copy.deepcopy`` restatement.  The helpers are shared with tests/test_unrolled_gpu.py."""
import copy
import ctypes
import types

import pytest
import torch

from conftest import load_golden, sub
from mr_gnas_amd import _lib, architect as A, architect_nc as AN
from oracle import nets as ON
from oracle.graph import OGraph

R_SMALL = 1e-2
BUF_SEED = 1


class OracleSupernet64:
    """What the architects use of the reference's Network, on oracle.nets in float64."""

    def __init__(self, z, S=None, alphas=None):
        self.z = z
        S = {k: v.double() for k, v in sub(z, "param/").items()} if S is None else S
        self.S = {k: v.detach().clone().requires_grad_(True) for k, v in S.items()}
        alphas = [z[f"e0/alpha_before/{i}"].double() for i in range(5)] if alphas is None else alphas
        self.alphas = [a.detach().clone().requires_grad_(True) for a in alphas]

    def parameters(self):
        return list(self.S.values())

    def named_parameters(self):
        return list(self.S.items())

    def arch_parameters(self):
        return self.alphas

    def __call__(self, g, node_id, src_in, edge_type):
        return ON.supernet_forward(g, self.S, self.alphas, node_id, src_in, edge_type, 2 * self.z["R"] + 1, self.z["layers"])

    def _loss(self, g, node_id, src_in, edge_type, data, labels):
        return ON.distmult_bce(*self(g, node_id, src_in, edge_type), data, labels)

    def copy_from_theta(self, theta):
        """Where the reference calls new() + load_state_dict: the same network on the weights `theta` (flat) and copies of the alphas."""
        S, o = {}, 0
        for k, v in self.S.items():
            S[k] = theta[o:o + v.numel()].view(v.shape)
            o += v.numel()
        assert o == theta.numel()
        return OracleSupernet64(self.z, S, self.alphas)


def step_inputs64(z, which):
    n = z[which + "/node_id"].numel()
    g = OGraph(n, z[which + "/src"], z[which + "/dst"], z[which + "/edge_type"], z[which + "/norm"].double())
    return (g, z[which + "/node_id"], z[which + "/src_in"], z[which + "/edge_type"], z[which + "/data"], z[which + "/labels"].double())


def arch_args(z):
    return types.SimpleNamespace(momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]),
                                 arch_learning_rate=float(z["arch_learning_rate"]), arch_weight_decay=float(z["arch_weight_decay"]))


def seeded_buffers(params, seed=BUF_SEED):
    """0.01 * randn (float32 values) from a seeded CPU generator, one per parameter in order."""
    gen = torch.Generator().manual_seed(seed)
    return [0.01 * torch.randn(tuple(p.shape), generator=gen) for p in params]


def _concat(xs):
    return torch.cat([x.reshape(-1) for x in xs])


def restatement(model, make_copy, train_loss, val_loss, eta, bufs, momentum, weight_decay, allow_unused=False):
    """The reference's _backward_step_unrolled.  train_loss(m) / val_loss(m): m._loss on the training / validation sample;
    make_copy(model, theta): where the reference calls _construct_model_from_theta.  Returns dict(loss, dalpha, ig, final) -- lists
    with None for an alpha the loss does not reach -- and the copy.  allow_unused=True (node classification, whose Network owns
    weights no loss reaches: the reference's allow_unused=False raises there): such a weight has a zero gradient."""
    params = list(model.parameters())
    # _compute_unrolled_model
    loss = train_loss(model)
    theta = _concat(params).detach()
    moment = _concat(bufs).mul(momentum) if bufs is not None else torch.zeros_like(theta)
    g = torch.autograd.grad(loss, params, allow_unused=allow_unused)
    dtheta = _concat([torch.zeros_like(p) if x is None else x for x, p in zip(g, params)]).detach() + weight_decay * theta
    unrolled = make_copy(model, theta.sub(moment + dtheta, alpha=eta))
    # _backward_step_unrolled
    loss = val_loss(unrolled)
    loss.backward()
    dalpha = [None if v.grad is None else v.grad.detach().clone() for v in unrolled.arch_parameters()]
    vector = [torch.zeros_like(v) if v.grad is None else v.grad.detach() for v in unrolled.parameters()]
    # _hessian_vector_product
    R = R_SMALL / _concat(vector).norm()
    with torch.no_grad():
        for p, v in zip(params, vector):
            p.add_(v, alpha=float(R))
    grads_p = torch.autograd.grad(train_loss(model), model.arch_parameters(), allow_unused=True)
    with torch.no_grad():
        for p, v in zip(params, vector):
            p.sub_(v, alpha=float(2 * R))
    grads_n = torch.autograd.grad(train_loss(model), model.arch_parameters(), allow_unused=True)
    with torch.no_grad():
        for p, v in zip(params, vector):
            p.add_(v, alpha=float(R))
    ig = [None if x is None else (x - y).div_(2 * R) for x, y in zip(grads_p, grads_n)]
    final = [None if g is None else g - eta * i for g, i in zip(dalpha, ig)]
    return dict(loss=loss.detach(), dalpha=dalpha, ig=ig, final=final, R=R, norm=_concat(vector).norm()), unrolled


_REFS = {}


def lp_reference_cached(case):
    """The float64 restatement on the oracle supernet of fixture `case` with eta = lr and the seeded momentum buffers: computed once
    per fixture, shared by the tests (of both files) and left unchanged."""
    if case not in _REFS:
        z = load_golden(case)
        model = OracleSupernet64(z)
        bufs = [b.double() for b in seeded_buffers(model.parameters())]
        train, val = step_inputs64(z, "train"), step_inputs64(z, "val")
        _REFS[case], _ = restatement(model, lambda m, theta: m.copy_from_theta(theta), lambda m: m._loss(*train), lambda m: m._loss(*val),
                                     float(z["lr"]), bufs, float(z["momentum"]), float(z["weight_decay"]))
    return _REFS[case]


def sgd_with_buffers(params, bufs, lr, momentum, weight_decay):
    opt = torch.optim.SGD(params, lr, momentum=momentum, weight_decay=weight_decay)
    for p, b in zip(params, bufs):
        opt.state[p]["momentum_buffer"] = b.to(p.dtype).clone()
    return opt


def close(got, ref, what, rtol=1e-9):
    err, scale = float((got.double() - ref.double()).abs().max()), float(ref.double().abs().max())
    print(f"{what}: err {err:.3e} (max {scale:.3e})")
    assert err <= rtol * scale, f"{what}: err {err:.3e} > {rtol:g} * {scale:.3e}"


@pytest.mark.parametrize("case", ["architect_tiny", "architect_d24"])
def test_engine_matches_the_restatement_in_float64(case):
    from mr_gnas_amd.architect_unrolled import SecondOrderArchitect
    torch.set_num_threads(1)
    z = load_golden(case)
    ref = lp_reference_cached(case)
    model = OracleSupernet64(z)
    before = [p.detach().clone() for p in model.parameters()]
    lr = float(z["lr"])
    opt = sgd_with_buffers(model.parameters(), seeded_buffers(model.parameters()), lr, float(z["momentum"]), float(z["weight_decay"]))
    architect = SecondOrderArchitect("cpu", model, arch_args(z))
    assert isinstance(architect.optimizer, torch.optim.Adam)
    seen = {}
    adam_step = architect.optimizer.step
    architect.optimizer.step = lambda *a, **k: seen.update(final=[None if a_.grad is None else a_.grad.clone() for a_ in model.alphas]) or adam_step(*a, **k)
    alphas_before = [a.detach().clone() for a in model.alphas]
    architect.step(*step_inputs64(z, "train"), *step_inputs64(z, "val"), lr, opt, True)
    close(architect.loss.detach(), ref["loss"], case + " loss")
    close(architect.scal[0], ref["norm"], case + " |v|")
    close(architect.scal[1], ref["R"], case + " R")
    for i in range(4):
        close(architect.dalpha[i], ref["dalpha"][i], f"{case} dalpha {i}")
        close(architect.implicit_grads[i], ref["ig"][i], f"{case} implicit_grads {i}")
        close(seen["final"][i], ref["final"][i], f"{case} alpha.grad {i}")
        assert lr * float(ref["ig"][i].abs().max()) >= 0.05 * float(ref["dalpha"][i].abs().max()), "the implicit term is dead in this fixture"
        assert not torch.equal(model.alphas[i].detach(), alphas_before[i])           # Adam stepped it
    assert ref["dalpha"][4] is None and architect.dalpha[4] is None and architect.implicit_grads[4] is None and seen["final"][4] is None
    assert model.alphas[4].grad is None and torch.equal(model.alphas[4].detach(), alphas_before[4])
    for p, b in zip(model.parameters(), before):                                       # the parameters come back equal
        assert torch.equal(p.detach(), b)
    assert all(p.grad is None for p in model.parameters())                             # the weights' .grad are not touched


def test_zero_moment_branches_and_eta_forms():
    """optimizer None, an SGD that has not stepped yet (the reference's except: branch) and momentum buffers of zeros agree; eta as a
    0-dim tensor equals eta as a float; unrolled=False is the parent's step."""
    from mr_gnas_amd.architect_unrolled import SecondOrderArchitect
    torch.set_num_threads(1)
    z = load_golden("architect_tiny")
    lr = float(z["lr"])
    train, val = step_inputs64(z, "train"), step_inputs64(z, "val")
    grads = {}
    for how in ("none", "fresh_sgd", "zeros", "tensor_eta"):
        model = OracleSupernet64(z)
        params = model.parameters()
        opt = {"none": None, "fresh_sgd": torch.optim.SGD(params, lr, momentum=0.9),
               "zeros": sgd_with_buffers(params, [torch.zeros_like(p) for p in params], lr, 0.9, 0.0),
               "tensor_eta": None}[how]
        architect = SecondOrderArchitect("cpu", model, arch_args(z))
        architect.step(*train, *val, torch.tensor(lr, dtype=torch.float64) if how == "tensor_eta" else lr, opt, True)
        grads[how] = [a.grad.clone() for a in model.alphas[:4]]
    for how in ("fresh_sgd", "zeros", "tensor_eta"):
        assert all(torch.equal(a, b) for a, b in zip(grads[how], grads["none"])), how
    first, parent = OracleSupernet64(z), OracleSupernet64(z)
    SecondOrderArchitect("cpu", first, arch_args(z)).step(*train, *val, lr, None, False)
    A.Architect("cpu", parent, arch_args(z)).step(*train, *val, lr, None, False)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(first.alphas, parent.alphas))
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(first.parameters(), parent.parameters()))      # the validation gradients stay
    with pytest.raises(ValueError, match="eta"):
        SecondOrderArchitect("cpu", first, arch_args(z)).step(*train, *val, None, None, True)


def test_a_failing_pass_puts_the_parameters_back():
    from mr_gnas_amd.architect_unrolled import SecondOrderArchitect
    z = load_golden("architect_tiny")
    model = OracleSupernet64(z)
    before = [p.detach().clone() for p in model.parameters()]
    architect = SecondOrderArchitect("cpu", model, arch_args(z))
    train, val = step_inputs64(z, "train"), step_inputs64(z, "val")
    calls = {"n": 0}
    loss = model._loss

    def failing(*a):
        calls["n"] += 1
        if calls["n"] == 3:                                   # the pass at theta + R v
            raise RuntimeError("boom")
        return loss(*a)

    model._loss = failing
    with pytest.raises(RuntimeError, match="boom"):
        architect.step(*train, *val, float(z["lr"]), None, True)
    assert all(torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))


# ---- node classification ----------------------------------------------------------------------------------------------------------
def nc_setup():
    """(z16, z, inputs) of nc_search_small on the CPU: trip, labels, (train seeds, blocks), (val seeds, blocks)."""
    from test_nc_cpu import fixture_blocks
    from test_nc_search_cpu import CASES
    z16, z = load_golden(CASES["s16"]), load_golden("nc_search_small")
    blocks = {w: fixture_blocks(z, w + "/blocks/") for w in ("train", "val")}
    return z16, z, (z16["s16/trip_index"], z16["s16/labels"], (z["train/seeds"].long(), blocks["train"]), (z["val/seeds"].long(), blocks["val"]))


def nc_reference(z16, z, inputs):
    """The float64 deepcopy restatement on the package's CPU supernet.  Returns (ref, the model after it: its buffers are the end state)."""
    from test_nc_search_cpu import make_net64
    trip, labels, (seeds, blocks), (val_seeds, val_blocks) = inputs
    model = make_net64(z16, "s16").train()
    bufs = [b.double() for b in seeded_buffers(list(model.parameters()))]

    def make_copy(m, theta):
        new = copy.deepcopy(m)                               # state_dict() of the model after the first pass: buffers included
        o = 0
        with torch.no_grad():
            for p in new.parameters():
                p.copy_(theta[o:o + p.numel()].view(p.shape))
                o += p.numel()
        assert o == theta.numel()
        return new

    ref, _ = restatement(model, make_copy, lambda m: m._loss(trip, blocks, labels, seeds), lambda m: m._loss(trip, val_blocks, labels, val_seeds),
                         float(z["lr"]), bufs, float(z["momentum"]), float(z["weight_decay"]), allow_unused=True)
    return ref, model


def test_node_classification_matches_a_deepcopy_restatement_in_float64():
    """float64: model_search_nc's CPU path accepts it (with make_net64's op_forward)."""
    from mr_gnas_amd.architect_unrolled import SecondOrderArchitectNC
    from test_nc_search_cpu import make_net64, search_args
    torch.set_num_threads(1)
    z16, z, inputs = nc_setup()
    ref, ref_model = nc_reference(z16, z, inputs)
    trip, labels, (seeds, blocks), (val_seeds, val_blocks) = inputs
    model = make_net64(z16, "s16").train()
    params = list(model.parameters())
    before = [p.detach().clone() for p in params]
    lr = float(z["lr"])
    opt = sgd_with_buffers(params, seeded_buffers(params), lr, float(z["momentum"]), float(z["weight_decay"]))
    architect = SecondOrderArchitectNC("cpu", model, search_args(z))
    seen = {}
    adam_step = architect.optimizer.step
    architect.optimizer.step = lambda *a, **k: seen.update(final=[a_.grad.clone() for a_ in model.arch_parameters()]) or adam_step(*a, **k)
    architect.step(trip, blocks, labels, seeds, val_blocks, val_seeds, lr, opt, True)
    close(architect.loss.detach(), ref["loss"], "nc loss")
    for i in range(4):
        close(architect.dalpha[i], ref["dalpha"][i], f"nc dalpha {i}")
        close(architect.implicit_grads[i], ref["ig"][i], f"nc implicit_grads {i}")
        close(seen["final"][i], ref["final"][i], f"nc alpha.grad {i}")
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    assert all(p.grad is None for p in params)
    got, want = dict(model.named_buffers()), dict(ref_model.named_buffers())
    assert got.keys() == want.keys() and any(n.endswith("running_mean") for n in got)
    for n, b in want.items():
        if n.endswith("num_batches_tracked"):
            assert int(got[n]) == int(b) == 3, n                # three training-mode passes on the training sample, none from validation
        else:
            torch.testing.assert_close(got[n], b, rtol=1e-9, atol=1e-12, msg=lambda m: f"buffer {n}: {m}")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def test_the_parents_still_raise_and_the_abi_declares_the_kernels():
    from mr_gnas_amd import architect_unrolled as AU
    from test_architect_cpu import OracleSupernet, step_inputs
    z = load_golden("architect_tiny")
    with pytest.raises(NotImplementedError, match="model.new"):
        A.Architect("cpu", OracleSupernet(z), arch_args(z)).step(*step_inputs(z, "train"), *step_inputs(z, "val"), 0.01, None, True)
    assert issubclass(AU.SecondOrderArchitect, A.Architect) and issubclass(AU.SecondOrderArchitectNC, AN.Architect)
    import inspect
    assert list(inspect.signature(AU.SecondOrderArchitect.step).parameters) == list(inspect.signature(A.Architect.step).parameters)
    assert list(inspect.signature(AU.SecondOrderArchitectNC.step).parameters) == list(inspect.signature(AN.Architect.step).parameters)
    with pytest.raises(ValueError, match="eta"):
        A.search_epoch(None, None, None, (None,) * 6, (None,) * 6, 0, 0, unrolled=True)
    with pytest.raises(ValueError, match="lr"):
        AN.search_step(None, None, None, None, (None, None), (None, None), None, 1, 0, None, unrolled=True)
    names = ["mrg_unrolled_virtual_step", "mrg_unrolled_radius", "mrg_unrolled_shift", "mrg_unrolled_alpha_grad"]
    for n in names:
        assert n in _lib.SIGNATURES and n in _lib.declared_symbols(), n
    assert _lib.ABI_VERSION == 23
    lib = _lib.load()
    assert lib.mrg_abi_version() == 23
    P = ctypes.c_void_p
    t = P(16)
    # argument validation happens before any launch
    assert lib.mrg_unrolled_virtual_step(t, t, None, t, t, t, t, 0, t, 0.9, 0.0, None) == 0                  # nothing to do
    assert lib.mrg_unrolled_virtual_step(None, t, t, t, t, t, t, 5, t, 0.9, 0.0, None) == -1
    assert lib.mrg_unrolled_virtual_step(t, t, t, None, t, t, t, 5, t, 0.9, 0.0, None) == -1
    assert lib.mrg_unrolled_virtual_step(t, t, t, t, t, t, t, 5, None, 0.9, 0.0, None) == -1
    assert lib.mrg_unrolled_virtual_step(t, t, None, t, t, t, t, 1 << 31, t, 0.9, 0.0, None) == -2
    assert lib.mrg_unrolled_radius(t, t, t, t, 5, t, 0.01, None, None) == -1
    assert lib.mrg_unrolled_radius(None, t, t, t, 5, t, 0.01, t, None) == -1
    assert lib.mrg_unrolled_radius(t, t, t, t, 5, None, 0.01, t, None) == -1
    assert lib.mrg_unrolled_radius(t, t, t, t, 5, t, 0.0, t, None) == -2
    assert lib.mrg_unrolled_radius(t, t, t, t, 1 << 31, t, 0.01, t, None) == -2
    assert lib.mrg_unrolled_shift(t, t, t, t, t, t, 5, t, 2, None) == -3
    assert lib.mrg_unrolled_shift(t, t, None, t, t, t, 0, None, 0, None) == 0
    assert lib.mrg_unrolled_shift(t, None, t, t, t, t, 5, t, 1, None) == -1
    assert lib.mrg_unrolled_shift(t, t, None, t, t, t, 5, t, 1, None) == -1
    assert lib.mrg_unrolled_shift(t, t, t, t, t, t, 5, None, -1, None) == -1
    assert lib.mrg_unrolled_shift(t, t, t, t, t, t, 1 << 31, t, 1, None) == -2
    assert lib.mrg_unrolled_alpha_grad(t, None, t, t, t, t, t, t, 0, t, t, None) == 0
    assert lib.mrg_unrolled_alpha_grad(None, None, t, t, t, t, t, t, 5, t, t, None) == -1
    assert lib.mrg_unrolled_alpha_grad(t, None, t, None, t, t, t, t, 5, t, t, None) == -1
    assert lib.mrg_unrolled_alpha_grad(t, None, t, t, t, t, t, t, 5, t, None, None) == -1
    assert lib.mrg_unrolled_alpha_grad(t, None, t, t, t, t, t, t, 1 << 31, t, t, None) == -2
    from mr_gnas_amd.optim import _ParamTables
    with pytest.raises(_lib.MrgnasError):                    # the tables have no CPU form
        _ParamTables("x", [torch.zeros(3, requires_grad=True)], 0, width=2)
