"""Node-classification architecture search on CPU tensors (no GPU): cell_nc / model_search_nc / architect_nc in their torch formulation
against the reference's values (tests/golden/make_golden_nc_search.py: models/model_search.Network, models/architect.Architect and the
batch body of search/mr_nc_search.py:train() run unchanged).  The helpers here are shared with tests/test_nc_search_gpu.py.

Bounds are those of tests/test_nc_cpu.py (close() defaults for outputs; gradients rtol 2e-3, atol 5e-6 over ALL stored parameters with
no exclusions; alpha gradients 2e-3 * max|ref| + 1e-7; running statistics rtol 1e-4, atol 1e-5) and, for the three search passes, the
procedure of tests/test_architect_cpu.py (alphas reset from the fixture before each pass, a shadow torch.optim.Adam on the test's own
gradients within 1e-3 * arch lr, losses rtol 1e-4 / atol 1e-6, the weight step as (before - after) / lr).

Case s64 stores its state in float16 (exact: the reference ran on the rounded values) and every parameter gradient in two further
files: 310 010 parameters and as many gradients do not fit one fixture below the repository's file size limit."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import load_golden
from test_nc_cpu import close, fixture_blocks

from mr_gnas_amd import architect_nc as AN, cell_nc as CN, model_search_nc as MS, operations_nc as ON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"s16": "nc_supernet_small", "s64": "nc_supernet_s64"}
GRAD_PARTS = {"s64": ["nc_supernet_s64_grads0", "nc_supernet_s64_grads1"]}


def unpack(z, prefix):
    """{name: tensor} of a collection stored by make_golden_nc_search.pack()."""
    out, fo, io = {}, 0, 0
    f, i = z[prefix + "/f"].float(), z[prefix + "/i"]
    for name, shape, kind in json.loads(z[prefix + "/index"]):
        n = 1
        for s in shape:
            n *= s
        if kind == "f":
            out[name] = f[fo:fo + n].reshape(shape).clone()
            fo += n
        else:
            out[name] = i[io:io + n].reshape(shape).clone()
            io += n
    assert fo == f.numel() and io == i.numel(), prefix
    return out


def stored_gradients(z, tag):
    """Every parameter gradient of case `tag`: in the case's own file, or (s64) in its two gradient files."""
    if tag + "/gparam/index" in z:
        return unpack(z, tag + "/gparam")
    out = {}
    for part in GRAD_PARTS[tag]:
        out.update(unpack(load_golden(part), tag + "/gparam"))
    return out


def make_net(z, tag, device="cpu", state=None):
    N, T, R, classes, D, D0, nbase, batch, layers, nodes = [int(v) for v in z[tag + "/args"]]
    net = MS.Network(torch.device(device), N, classes, R, layers, 1, nodes, D, D0, nbase)
    net.load_state_dict(unpack(z, tag + "/param0") if state is None else state)
    net = net.to(device)
    with torch.no_grad():
        for i, a in enumerate(net.arch_parameters()):
            a.copy_(z[f"{tag}/alpha/{i}"])
    return net


def make_net64(z, tag, state=None, alphas=None):
    """The same network in float64 on the CPU, from param0 (or `state`, a full or partial state_dict laid over it; `alphas`): the
    yardstick for the fixture's own (float32) error."""
    net = make_net(z, tag)
    if state is not None:
        net.load_state_dict(state, strict=False)
    net = net.double()
    alphas = [(z[f"{tag}/alpha/{i}"] if alphas is None else alphas[i]).double().clone().requires_grad_(True) for i in range(4)]
    net.alphas_zero_cell, net.alphas_first_cell, net.alphas_middle_cell, net.alphas_last_cell = alphas
    net._arch_parameters = alphas

    def op_forward(self, op, g, h, h_in):                  # the reference's `.float()` between the stages would undo the float64
        nh = op[0](g, h, h_in)
        for i in range(1, len(op)):
            nh = op[i](nh)
        return nh

    for m in net.modules():
        if isinstance(m, CN.MixedOp):
            m.op_forward = types.MethodType(op_forward, m)
    return net


class Yardstick:
    """One training-mode forward + backward of the network in float64 on the CPU (weights `state`, alphas `alphas`), run when first
    asked for.  For a HIP result that misses a bound taken from the CPU tests: the fixture is itself a float32 run, and where one
    ReLU / arg-max decision falls the other way than in exact arithmetic its own error is far above rounding (measured: 7.5e-4 on the
    alpha gradients of nc_search_small's first pass, 1.5e-5 on case s16's logits).  The HIP error against this run may then be at
    most twice the fixture's own."""

    def __init__(self, z, tag, state, alphas, trip, labels, seeds, blocks):
        self.args, self._out = (z, tag, state, alphas, trip, labels, seeds, blocks), None

    def __call__(self):
        if self._out is None:
            z, tag, state, alphas, trip, labels, seeds, blocks = self.args
            net = make_net64(z, tag, state, alphas).train()
            net._loss(trip, blocks, labels, seeds).backward()
            self._out = ({n: p.grad for n, p in net.named_parameters() if p.grad is not None}, [a.grad for a in net.arch_parameters()])
        return self._out


def within_twice_the_fixture(got, ref, exact, what):
    got_err, ref_err = float((got.double().cpu() - exact).abs().max()), float((ref.double() - exact).abs().max())
    print(f"{what}: misses the float32 bound; against float64: here {got_err:.3e}, the fixture {ref_err:.3e}")
    assert got_err <= 2.0 * ref_err, f"{what}: err {got_err:.3e} against float64, the fixture's own is {ref_err:.3e}"


def grads_close(net, ref, no_grad, rtol=2e-3, atol=5e-6, what="", yard=None):
    """Every stored parameter gradient against the reference's; a parameter the reference gave no gradient has none (or zero) here.
    yard: None, or the Yardstick a tensor that misses the bound is judged by."""
    seen = 0
    for n, p in net.named_parameters():
        if n in no_grad:
            assert p.grad is None or not p.grad.any(), n
        elif n in ref:
            assert p.grad is not None, f"{what} {n}: no gradient"
            if yard is not None and not torch.allclose(p.grad.cpu(), ref[n], rtol=rtol, atol=atol):
                within_twice_the_fixture(p.grad, ref[n], yard()[0][n], f"{what} {n} grad")
            else:
                torch.testing.assert_close(p.grad.cpu(), ref[n], rtol=rtol, atol=atol, msg=lambda m: f"{what} {n} grad: {m}")
            seen += 1
    assert seen == len(ref)


def alpha_grads_close(grads, refs, what="", yard=None):
    for i, (g, ref) in enumerate(zip(grads, refs)):
        assert g is not None, f"{what} alpha {i}: no gradient"
        err = float((g.cpu() - ref).abs().max())
        if err > 2e-3 * float(ref.abs().max()) + 1e-7 and yard is not None:
            within_twice_the_fixture(g, ref, yard()[1][i], f"{what} alpha {i} gradient")
        else:
            assert err <= 2e-3 * float(ref.abs().max()) + 1e-7, f"{what} alpha {i}: gradient err {err:.3e} (max {float(ref.abs().max()):.3e})"


def buffers_close(net, ref, what=""):
    got = dict(net.named_buffers())
    for n, b in ref.items():
        if n.endswith("num_batches_tracked"):
            assert int(got[n]) == int(b), f"{what} {n}"
        else:
            torch.testing.assert_close(got[n].cpu(), b, rtol=1e-4, atol=1e-5, msg=lambda m: f"{what} buffer {n}: {m}")


def check_step(z, tag, net, dev="cpu", logits_tol=None):
    """One training step and one eval forward of `net` against case `tag`."""
    blocks = [b.to(dev) for b in fixture_blocks(z, tag + "/blocks/")] if dev != "cpu" else fixture_blocks(z, tag + "/blocks/")
    trip, labels, seeds = z[tag + "/trip_index"].to(dev), z[tag + "/labels"].to(dev), z[tag + "/seeds"].long().to(dev)
    net.train()
    logits = net(trip, blocks)
    loss = net._criterion(logits, labels[seeds])
    loss.backward()
    tol = logits_tol or {}
    close(logits, z[tag + "/logits"], tag + " logits", **tol)
    close(loss.reshape(1), z[tag + "/loss"].reshape(1), tag + " loss")
    yard = None if dev == "cpu" else Yardstick(z, tag, None, None, z[tag + "/trip_index"], z[tag + "/labels"], z[tag + "/seeds"].long(),
                                               fixture_blocks(z, tag + "/blocks/"))
    gref, no_grad = stored_gradients(z, tag), set(json.loads(z[tag + "/no_grad_names"]))
    assert set(gref) | no_grad == {n for n, _ in net.named_parameters()}, f"{tag}: the fixture does not hold every parameter's gradient"
    grads_close(net, gref, no_grad, what=tag, yard=yard)
    alpha_grads_close([a.grad for a in net.arch_parameters()], [z[f"{tag}/galpha/{i}"] for i in range(4)], tag, yard)
    buffers_close(net, unpack(z, tag + "/buffer"), tag)
    net.eval()
    with torch.no_grad():
        close(net(trip, blocks), z[tag + "/logits_eval"], tag + " eval logits", **tol)
    return blocks


@pytest.mark.parametrize("tag", ["s16", "s64"])
def test_contract_matches_the_reference(tag):
    z = load_golden(CASES[tag])
    net = make_net(z, tag)
    assert list(net.state_dict().keys()) == json.loads(z[tag + "/state_keys"])
    ref = unpack(z, tag + "/param0")
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.items()}
    assert sum(p.numel() for p in net.parameters()) == int(z[tag + "/n_parameters"])
    assert [tuple(a.shape) for a in net.arch_parameters()] == [tuple(z[f"{tag}/alpha/{i}"].shape) for i in range(4)]
    assert all(a.requires_grad and a.is_leaf and not isinstance(a, torch.nn.Parameter) for a in net.arch_parameters())
    assert not any("alpha" in k for k in net.state_dict())
    assert repr(net.show_genotypes()) == z[tag + "/genotypes"]
    assert type(net.show_genotype(0)).__name__ == "Genotype" and net.show_genotype(0).score_func is None
    with pytest.raises(NotImplementedError):
        net.new()


def test_fresh_alphas_and_load_alpha():
    torch.manual_seed(0)
    net = MS.Network(torch.device("cpu"), 30, 3, 4, 2, 1, 3, 8, 4, 3, dropout=0.25)
    assert net._dropout == 0.25
    assert [tuple(a.shape) for a in net.arch_parameters()] == [(2, len(ON.PRE_OPS)), (12, len(ON.FIRST_OPS)), (6, len(ON.MIDDLE_OPS)), (24, len(ON.LAST_OPS))]
    assert all(0 < float(a.detach().abs().max()) < 1e-2 for a in net.arch_parameters())          # 1e-3 * randn
    new = [torch.full_like(a, 0.5) for a in net.arch_parameters()]
    net.load_alpha(new)
    assert all(torch.equal(a.detach(), b) for a, b in zip(net.arch_parameters(), new))
    W = net.show_weights(1)
    assert [tuple(w.shape) for w in W] == [(1, 3), (6, 4), (3, 3), (12, 4)]
    assert all(torch.allclose(w.sum(1), torch.ones(w.shape[0])) for w in W)


@pytest.mark.parametrize("tag", ["s16", "s64"])
def test_cpu_supernet_matches_the_reference(tag):
    torch.set_num_threads(1)
    z = load_golden(CASES[tag])
    check_step(z, tag, make_net(z, tag))


def test_f_zero_branch_has_the_reference_semantics():
    """Linear(0 * x) = bias on every row: BatchNorm's running variance goes to 0.9 * 1 after one step, the Linear's weight gets a
    ZERO gradient tensor (not None), and the branch contributes w_k * ReLU(beta_k) to every row."""
    z = load_golden(CASES["s16"])
    net = make_net(z, "s16")
    check_step(z, "s16", net)
    first = net.cells[0].cell_first._ops[0]
    k = ON.FIRST_OPS.index("f_zero")
    lin, bn = first._ops[k][1], first._ops[k][2]
    assert torch.allclose(bn.running_var, torch.full_like(bn.running_var, 0.9), rtol=0, atol=1e-6)
    assert lin.weight.grad is not None and lin.weight.grad.shape == lin.weight.shape and not lin.weight.grad.any()
    assert bn.bias.grad is not None and bn.bias.grad.abs().max() > 0
    mop = CN.MixedOp(8, ON.FIRST_OPS).train()
    with torch.no_grad():
        mop._ops[k][2].bias.copy_(torch.linspace(-1, 1, 8))
    w = torch.zeros(4)
    w[k] = 0.7
    blk = fixture_blocks(z, "s16/blocks/")[1]
    x = torch.randn(blk.num_edges(), 8)
    out = mop(w, blk, x, x)
    # BatchNorm of a constant column is (b - mean(b)) / sqrt(0 + eps): the mean of equal float32 values is off by a few ulp of
    # |b| <= 0.5 (6e-8 each), which 1 / sqrt(1e-5) = 316 magnifies -- 8 ulp give 1.5e-4 (the reference shows the same noise)
    torch.testing.assert_close(out, (0.7 * torch.relu(mop._ops[k][2].bias.detach())).expand_as(out), rtol=1e-5, atol=1.5e-4)
    mop.eval()                                               # eval mode: BatchNorm of the bias rows on the running statistics
    bn = mop._ops[k][2]
    ref = torch.relu((mop._ops[k][1].bias - bn.running_mean) / torch.sqrt(bn.running_var + bn.eps) * bn.weight + bn.bias)
    torch.testing.assert_close(mop(w, blk, x, x), (0.7 * ref.detach()).expand_as(out), rtol=1e-5, atol=1e-6)


def zero_bias_noise(net, gref):
    """{name: extra absolute bound} for the Linear biases of the f_zero candidates.  Their exact gradient is 0 (BatchNorm of a
    constant column does not depend on the constant), so what the reference stores there is its own rounding noise, magnified by
    1 / sqrt(eps) = 316: up to 1.8e-6 in nc_supernet_small and 5.0e-6 in nc_search_small.  A relative bound against noise means
    nothing, and two such noises differ by up to their sum; for these 36 tensors twice the reference's largest own error (the
    largest |gradient| it stores for any of them) joins the absolute bound."""
    names = [f"{n}._ops.{m._operations.index('f_zero')}.1.bias" for n, m in net.named_modules()
             if isinstance(m, CN.MixedOp) and "f_zero" in m._operations]
    worst = max(float(gref[n].abs().max()) for n in names)
    return {n: 2.0 * worst for n in names}


def search_args(z):
    return types.SimpleNamespace(momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]),
                                 arch_learning_rate=float(z["arch_learning_rate"]), arch_weight_decay=float(z["arch_weight_decay"]))


def run_search_passes(z16, z, net, architect, optimizer, dev, monkeypatch):
    """The three passes of nc_search_small with test_architect_cpu.py's procedure; works on the CPU and on HIP."""
    lr, alr = float(z["lr"]), float(z["arch_learning_rate"])
    blocks = {w: [b.to(dev) if dev != "cpu" else b for b in fixture_blocks(z, w + "/blocks/")] for w in ("train", "val")}
    trip, labels = z16["s16/trip_index"].to(dev), z16["s16/labels"].to(dev)
    train, val = (z["train/seeds"].long().to(dev), blocks["train"]), (z["val/seeds"].long().to(dev), blocks["val"])
    alphas = net.arch_parameters()
    shadow_p = [a.detach().clone().cpu().requires_grad_(True) for a in alphas]
    shadow = torch.optim.Adam(shadow_p, lr=alr, betas=(0.5, 0.999), weight_decay=float(z["arch_weight_decay"]))
    shadow64_p = [a.detach().clone().cpu().double().requires_grad_(True) for a in alphas]
    shadow64 = torch.optim.Adam(shadow64_p, lr=alr, betas=(0.5, 0.999), weight_decay=float(z["arch_weight_decay"]))
    seen = {}
    adam_step = architect.optimizer.step

    def after_architect_backward(*a, **k):
        seen["galpha"] = [a_.grad.detach().clone().cpu() for a_ in alphas]
        seen["val_grads"] = sum(p.grad is not None for p in net.parameters())
        return adam_step(*a, **k)

    sgd_step = optimizer.step

    def before_weight_step(*a, **k):
        seen["gparam"] = {n: (None if p.grad is None else p.grad.detach().clone().cpu()) for n, p in net.named_parameters()}
        return sgd_step(*a, **k)

    monkeypatch.setattr(architect.optimizer, "step", after_architect_backward)
    monkeypatch.setattr(optimizer, "step", before_weight_step)
    criterion = torch.nn.CrossEntropyLoss()
    zw = load_golden("nc_search_small_weights")
    keep = {}
    for e in range(int(z["passes"])):
        with torch.no_grad():
            for i, a in enumerate(alphas):
                a.copy_(z[f"e{e}/alpha_before/{i}"])
                shadow_p[i].copy_(z[f"e{e}/alpha_before/{i}"])
                shadow64_p[i].copy_(z[f"e{e}/alpha_before/{i}"])
            wb = None
            if e > 0:
                # the weights too are reset from the fixture: one ReLU / arg-max decision at a BatchNorm output within rounding of 0
                # moves the gradients behind it by a finite amount, and weights that drifted by an ulp would decide differently
                # (tests/golden/make_golden_nc_search.py, nc_search_small_weights)
                wb = unpack(zw, f"e{e}/param_before")
                for n, p in net.named_parameters():
                    p.copy_(wb[n])
        before = {n: p.detach().clone().cpu() for n, p in net.named_parameters()}
        loss, arch_loss, logits = AN.search_step(net, architect, optimizer, trip, train, val, labels, e, int(z["warm_epochs"]), criterion, lr)
        assert all(torch.is_tensor(t) and t.device.type == torch.device(dev).type and not t.requires_grad for t in (loss, arch_loss, logits))
        print(f"pass {e}: loss {float(loss):.7f} (ref {float(z[f'e{e}/loss']):.7f}) arch loss {float(arch_loss):.7f} (ref {float(z[f'e{e}/arch_loss']):.7f})")
        torch.testing.assert_close(arch_loss.cpu(), z[f"e{e}/arch_loss"], rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(loss.cpu(), z[f"e{e}/loss"], rtol=1e-4, atol=1e-6)
        assert seen["val_grads"] > 0                                      # the architect step did run a backward through the weights
        cpu_blocks = {w: fixture_blocks(z, w + "/blocks/") for w in ("train", "val")}
        yard = None if dev == "cpu" else Yardstick(z16, "s16", wb, [z[f"e{e}/alpha_before/{i}"] for i in range(4)], z16["s16/trip_index"],
                                                   z16["s16/labels"], z["val/seeds"].long(), cpu_blocks["val"])
        alpha_grads_close(seen["galpha"], [z[f"e{e}/galpha/{i}"] for i in range(4)], f"pass {e}", yard)
        for i in range(4):
            shadow_p[i].grad = seen["galpha"][i].clone()
        shadow.step()
        if yard is not None:
            for i in range(4):
                shadow64_p[i].grad = yard()[1][i].clone()
            shadow64.step()
        for i in range(4):
            err = float((alphas[i].detach().cpu() - shadow_p[i].detach()).abs().max())
            assert err <= 1e-3 * alr, f"pass {e} alpha {i}: {err:.3e} off torch.optim.Adam on the same gradients"
            err = float((alphas[i].detach().cpu() - z[f"e{e}/alpha_after/{i}"]).abs().max())
            print(f"pass {e} alpha {i} after the step: {err:.3e} off the fixture (allowed {1e-3 * alr:.1e})")
            if err > 1e-3 * alr and yard is not None:
                # Adam on the fixture's gradients, which are off by up to 1e-3 (above): the yardstick is Adam in float64 on the
                # float64 gradients of every pass so far
                within_twice_the_fixture(alphas[i].detach(), z[f"e{e}/alpha_after/{i}"], shadow64_p[i].detach(), f"pass {e} alpha {i} after the step")
            else:
                assert err <= 1e-3 * alr, f"pass {e} alpha {i} after the step: err {err:.3e}"
        if e == 0:
            # the weights' gradients are those of the TRAINING sample alone (optimizer.zero_grad() follows the architect step)
            gref = unpack(z, "e0/gparam_acc")
            noise = zero_bias_noise(net, gref)
            yard = None if dev == "cpu" else Yardstick(z16, "s16", None, [z[f"e0/alpha_after/{i}"] for i in range(4)], z16["s16/trip_index"],
                                                       z16["s16/labels"], z["train/seeds"].long(), cpu_blocks["train"])
            for n, g in seen["gparam"].items():
                if n not in gref:
                    assert g is None or not g.any(), n
                elif yard is not None and not torch.allclose(g, gref[n], rtol=2e-3, atol=5e-6 + noise.get(n, 0.0)):
                    within_twice_the_fixture(g, gref[n], yard()[0][n], f"training gradient {n}")
                else:
                    torch.testing.assert_close(g, gref[n], rtol=2e-3, atol=5e-6 + noise.get(n, 0.0), msg=lambda m: f"training gradient {n}: {m}")
            after = unpack(z, "e0/param_after")
            p0 = unpack(z16, "s16/param0")
            wd = float(z["weight_decay"])
            for n, p in net.named_parameters():
                # both sides round p - lr * step to float32 (half an ulp of |p| each), and the division by lr magnifies it
                ulp = 2.0 ** -23 * float(p0[n].abs().max()) / lr
                got, ref = (before[n] - p.detach().cpu()) / lr, (p0[n] - after[n]) / lr
                if yard is not None and n in gref and not torch.allclose(got, ref, rtol=2e-3, atol=5e-6 + noise.get(n, 0.0) + ulp):
                    exact = yard()[0][n] + wd * p0[n].double()          # the first step of SGD with momentum: gradient + weight decay
                    got_err, ref_err = float((got.double() - exact).abs().max()), float((ref.double() - exact).abs().max())
                    print(f"weight step {n}: against float64: here {got_err:.3e}, the fixture {ref_err:.3e}")
                    assert got_err <= 2.0 * ref_err + ulp, f"weight step {n}: err {got_err:.3e}, the fixture's own {ref_err:.3e}"
                else:
                    torch.testing.assert_close(got, ref, rtol=2e-3, atol=5e-6 + noise.get(n, 0.0) + ulp, msg=lambda m: f"weight step {n}: {m}")
            keep.update(noise=noise, yard=yard, p0=p0, wd=wd, names=set(gref))
        if e == 1:
            # the second weight step carries the momentum of the first: momentum * (first step) + gradient + weight decay, against
            # the fixture's weights at the start of pass 2.  (The optimiser's momentum buffer is the test's own from pass 0.)
            nxt, mom, wd = unpack(zw, "e2/param_before"), float(z["momentum"]), keep["wd"]
            yard = None if dev == "cpu" else Yardstick(z16, "s16", wb, [z[f"e1/alpha_after/{i}"] for i in range(4)], z16["s16/trip_index"],
                                                       z16["s16/labels"], z["train/seeds"].long(), cpu_blocks["train"])
            for n, p in net.named_parameters():
                ulp = 2.0 ** -23 * float(wb[n].abs().max()) / lr
                tol = 5e-6 + (1.0 + mom) * keep["noise"].get(n, 0.0) + ulp
                got, ref = (before[n] - p.detach().cpu()) / lr, (wb[n] - nxt[n]) / lr
                if yard is not None and n in keep["names"] and not torch.allclose(got, ref, rtol=2e-3, atol=tol):
                    exact = mom * (keep["yard"]()[0][n] + wd * keep["p0"][n].double()) + yard()[0][n] + wd * wb[n].double()
                    got_err, ref_err = float((got.double() - exact).abs().max()), float((ref.double() - exact).abs().max())
                    print(f"second weight step {n}: against float64: here {got_err:.3e}, the fixture {ref_err:.3e}")
                    assert got_err <= 2.0 * ref_err + ulp, f"second weight step {n}: err {got_err:.3e}, the fixture's own {ref_err:.3e}"
                else:
                    torch.testing.assert_close(got, ref, rtol=2e-3, atol=tol, msg=lambda m: f"second weight step {n}: {m}")


def test_search_passes_match_the_reference(monkeypatch):
    torch.set_num_threads(1)
    z16, z = load_golden(CASES["s16"]), load_golden("nc_search_small")
    net = make_net(z16, "s16").train()
    optimizer = torch.optim.SGD(net.parameters(), float(z["lr"]), momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]))
    architect = AN.Architect("cpu", net, search_args(z))
    assert isinstance(architect.optimizer, torch.optim.Adam)
    run_search_passes(z16, z, net, architect, optimizer, "cpu", monkeypatch)


def test_warm_up_takes_no_architect_step_and_unrolled_raises():
    z16, z = load_golden(CASES["s16"]), load_golden("nc_search_small")
    net = make_net(z16, "s16").train()
    optimizer = torch.optim.SGD(net.parameters(), float(z["lr"]))
    architect = AN.Architect("cpu", net, search_args(z))
    blocks = fixture_blocks(z, "train/blocks/")
    train = (z["train/seeds"].long(), blocks)
    before = [a.detach().clone() for a in net.arch_parameters()]
    loss, arch_loss, logits = AN.search_step(net, architect, optimizer, z16["s16/trip_index"], train, train, z16["s16/labels"], 3, 3,
                                             torch.nn.CrossEntropyLoss())          # epoch == warm_epochs: strict comparison
    assert torch.equal(arch_loss, torch.ones(1)) and torch.isfinite(loss) and logits.shape == (12, 4)
    assert all(torch.equal(a.detach(), b) for a, b in zip(net.arch_parameters(), before))
    with pytest.raises(NotImplementedError):
        architect.step(z16["s16/trip_index"], blocks, z16["s16/labels"], train[0], blocks, train[0], 0.01, optimizer, True)
    group = architect.optimizer.param_groups[0]
    assert group["lr"] == float(z["arch_learning_rate"]) and tuple(group["betas"]) == (0.5, 0.999)
    assert group["weight_decay"] == float(z["arch_weight_decay"])


def test_import_leaves_tensor_indexing_alone():
    code = ("import sys, torch; sys.path.insert(0, %r); before = torch.Tensor.__getitem__; "
            "import mr_gnas_amd.cell_nc, mr_gnas_amd.model_search_nc, mr_gnas_amd.architect_nc; "
            "assert torch.Tensor.__getitem__ is before; assert 'mr_gnas_amd.operations_lp' not in sys.modules; print('ok')"
            % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
