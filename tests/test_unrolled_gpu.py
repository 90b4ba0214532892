"""The second-order (unrolled) architect step on HIP: the mrg_unrolled_* kernels (csrc/optim.hip) one by one against float64 torch, and
architect_unrolled.SecondOrderArchitect / SecondOrderArchitectNC end to end against the float64 restatement of the reference's
``_backward_step_unrolled`` (tests/test_unrolled_cpu.py: on the CPU oracle supernet for link prediction, on a CPU copy of the network for
node classification).

Kernel bounds (float32 roundings of 2^-24 each, against the float64 value of the same float32 inputs):
  virtual step   2^-21 * (|p| + |eta| * (|mu buf| + |g| + |wd p|))      five roundings, a factor 2 for contraction
  shift +-1      2^-22 * (|p| + |R v|);  sign 0 and ``backup``: bit for bit
  scal           rtol 2^-22 against the float64 norm;  |v| = 0: R = 0, 1 / (2 R) = 0
  combine        2^-21 * (|dalpha| + |eta| * (|gp| + |gn|) / (2 R))
End to end: loss rtol 1e-4 / atol 1e-6; dalpha, implicit_grads and the final alpha.grad within 2e-3 * max|ref| + 1e-7 (the tolerances of
tests/test_architect_gpu.py and tests/test_nc_search_gpu.py for alpha gradients)."""
import sys

import pytest
import torch

from conftest import load_golden, sub
from poison import poisoned
from test_unrolled_cpu import (R_SMALL, arch_args, lp_reference_cached, nc_reference, nc_setup, seeded_buffers)

from mr_gnas_amd import architect as A, architect_nc as AN
from mr_gnas_amd._lib import call, ptr, stream_of
from mr_gnas_amd.architect_unrolled import SecondOrderArchitect, SecondOrderArchitectNC
from mr_gnas_amd.optim import ClippedSGD, FusedAdam, _ParamTables

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [1, 3, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 5]
VIEW = 6                                                      # this tensor's gradient / vector starts one element into a larger buffer
NULL = 2                                                      # the entry that is null in the "one_null" cases


# ---- kernels ------------------------------------------------------------------------------------------------------------------
def randn_list(gen, view=VIEW):
    out = [torch.randn(n, generator=gen).to(DEV) for n in SIZES]
    out[view] = torch.randn(SIZES[view] + 1, generator=gen).to(DEV)[1:]
    assert out[view].data_ptr() % 16 == 4 and out[view].is_contiguous()
    return out


class Lists:
    """Parameter tensors of SIZES with their tables, a backup and the scal / eta / partial device memory."""

    def __init__(self, gen, eta=0.025):
        self.params = [torch.randn(n, generator=gen).to(DEV) for n in SIZES]
        self.tab = _ParamTables("test", self.params, 0, width=2)
        self.flat, self.backup, self.b_ptrs = self.tab.flat_state(64, zero=False)
        self.flat.fill_(float("nan"))
        self.partial = torch.full((self.tab.n_chunks,), float("nan"), dtype=torch.float64, device=DEV)
        self.scal = torch.full((3,), float("nan"), device=DEV)
        self.eta = torch.tensor([eta], device=DEV)
        assert self.tab.n_chunks == 12

    def chunks(self):
        t = self.tab
        return ptr(t.chunk_tensor), ptr(t.chunk_off), ptr(t.chunk_len), t.n_chunks

    def virtual(self, g, bufs, momentum, wd):
        held = self.tab.stage(g) if bufs is None else self.tab.stage(g, bufs)
        call("mrg_unrolled_virtual_step", (ptr(self.tab.p_ptrs), self.tab.table(0), None if bufs is None else self.tab.table(1), ptr(self.b_ptrs),
                                           *self.chunks(), ptr(self.eta), momentum, wd, stream_of(self.flat)))
        return held

    def radius(self, v):
        held = self.tab.stage(v)
        call("mrg_unrolled_radius", (self.tab.table(0), *self.chunks(), ptr(self.partial), R_SMALL, ptr(self.scal), stream_of(self.flat)))
        return held

    def shift(self, sign):
        call("mrg_unrolled_shift", (ptr(self.tab.p_ptrs), ptr(self.b_ptrs), self.tab.table(0) if sign else None, *self.chunks(),
                                    ptr(self.scal) if sign else None, sign, stream_of(self.flat)))


@pytest.mark.parametrize("bufs_mode", ["absent", "present", "one_null"])
def test_virtual_step_radius_and_shifts_against_float64(bufs_mode):
    for wd, momentum in ((0.0, 0.0), (3e-4, 0.9), (0.0, 0.9), (3e-4, 0.0)):
        gen = torch.Generator().manual_seed(11)
        L = Lists(gen)
        old = [p.clone() for p in L.params]
        g = randn_list(gen)
        bufs = None if bufs_mode == "absent" else [torch.randn(n, generator=gen).to(DEV) for n in SIZES]
        if bufs_mode == "one_null":
            bufs[NULL] = None
        L.virtual(g, bufs, momentum, wd)
        eta = L.eta.double()
        worst = 0.0
        for i, (p, o, gi, k) in enumerate(zip(L.params, old, g, L.backup)):
            assert torch.equal(k, o), f"backup {i}"                                          # bit for bit
            m = torch.zeros_like(o).double() if bufs is None or bufs[i] is None else momentum * bufs[i].double()
            ref = o.double() - eta * (m + (gi.double() + wd * o.double()))
            bound = 2.0 ** -21 * (o.double().abs() + eta.abs() * (m.abs() + gi.double().abs() + (wd * o.double()).abs()))
            ratio = float(((p.double() - ref).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{bufs_mode} wd {wd} momentum {momentum} tensor {i}: {ratio:.3f} of the bound"
        print(f"virtual step, bufs {bufs_mode} wd {wd} momentum {momentum}: worst error {worst:.3f} of the bound")
        # the radius of a list v (one tensor an unaligned view; one null entry in the one_null case) and the three shifts
        v = randn_list(gen)
        if bufs_mode == "one_null":
            v[NULL] = None
        L.radius(v)
        norm = torch.sqrt(sum((x.double() ** 2).sum() for x in v if x is not None))
        want = torch.stack([norm, R_SMALL / norm, norm / (2.0 * R_SMALL)])
        rel = ((L.scal.double() - want).abs() / want).cpu()
        print(f"scal {L.scal.tolist()} relative errors {rel.tolist()}")
        assert float(rel.max()) <= 2.0 ** -22
        R = L.scal[1].double()
        for sign in (+1, -1):
            L.shift(sign)
            for i, (p, o, x) in enumerate(zip(L.params, old, v)):
                if x is None:
                    assert torch.equal(p, o), f"shift {sign} tensor {i}: a null vector leaves backup"
                    continue
                ref = o.double() + sign * R * x.double()
                bound = 2.0 ** -22 * (o.double().abs() + (R * x.double()).abs())
                assert bool(((p.double() - ref).abs() <= bound).all()), f"shift {sign} tensor {i}"
                assert not torch.equal(p, o) or o.numel() < 4
        L.shift(0)
        for i, (p, o) in enumerate(zip(L.params, old)):
            assert torch.equal(p, o), f"restore {i}"                                          # bit for bit
        assert all(torch.equal(k, o) for k, o in zip(L.backup, old))


def test_zero_norm_gives_zero_radius_and_a_finite_result():
    gen = torch.Generator().manual_seed(12)
    L = Lists(gen)
    old = [p.clone() for p in L.params]
    L.virtual(randn_list(gen), None, 0.9, 0.0)
    zero = [torch.zeros(n, device=DEV) for n in SIZES]
    L.radius(zero)
    assert L.scal.tolist() == [0.0, 0.0, 0.0]
    L.shift(+1)
    assert all(torch.equal(p, o) for p, o in zip(L.params, old))
    A_ = Alphas(gen)
    out, ig = A_.combine(L.eta, L.scal)
    for i in A_.live:
        assert torch.equal(ig[i], torch.zeros_like(ig[i])) and torch.equal(out[i], A_.dalpha[i])        # the implicit term is zero


class Alphas:
    """Five architecture-parameter shapes (one of more than a chunk) with dalpha / gp / gn; the last has no gradient."""
    SHAPES = [(2, 3), (12, 4), (1100, 4), (24, 4), (1, 2)]

    def __init__(self, gen):
        self.alphas = [torch.zeros(s, device=DEV) for s in self.SHAPES]
        self.tab = _ParamTables("test", self.alphas, 0, width=5)
        mk = lambda: [torch.randn(s, generator=gen).to(DEV) for s in self.SHAPES]
        self.dalpha, self.gp, self.gn = mk(), mk(), mk()
        self.gn = [a + 1e-3 * b for a, b in zip(self.gp, self.gn)]                                    # a finite difference: nearly equal
        self.gp[4] = self.gn[4] = None
        self.live = range(4)
        assert self.tab.n_chunks == 6

    def combine(self, eta, scal):
        out, ig = ([torch.full(s, 7.0, device=DEV) for s in self.SHAPES] for _ in range(2))
        t = self.tab
        held = t.stage(out, ig, self.dalpha, self.gp, self.gn)
        call("mrg_unrolled_alpha_grad", (t.table(0), t.table(1), t.table(2), t.table(3), t.table(4), ptr(t.chunk_tensor), ptr(t.chunk_off),
                                         ptr(t.chunk_len), t.n_chunks, ptr(eta), ptr(scal), stream_of(out[0])))
        del held
        return out, ig


def test_combine_against_float64():
    gen = torch.Generator().manual_seed(13)
    A_ = Alphas(gen)
    eta = torch.tensor([0.025], device=DEV)
    scal = torch.tensor([3.0, 0.01 / 3.0, 150.0], device=DEV)
    out, ig = A_.combine(eta, scal)
    e, inv = eta.double(), scal[2].double()
    for i in A_.live:
        d, a, c = A_.dalpha[i].double(), A_.gp[i].double(), A_.gn[i].double()
        bound = 2.0 ** -21 * (d.abs() + e * (a.abs() + c.abs()) * inv)
        assert bool(((ig[i].double() - (a - c) * inv).abs() <= 2.0 ** -22 * (a.abs() + c.abs()) * inv).all()), f"ig {i}"
        ratio = float(((out[i].double() - (d - e * (a - c) * inv)).abs() / bound).max())
        print(f"combine alpha {i}: worst error {ratio:.3f} of the bound")
        assert ratio <= 1.0
    assert torch.equal(out[4], torch.full_like(out[4], 7.0)) and torch.equal(ig[4], torch.full_like(ig[4], 7.0))       # no gradient: untouched


# ---- link prediction end to end -----------------------------------------------------------------------------------------------
def lp_setup(case, net=None):
    """The HIP SearchNetwork of fixture `case`, a ClippedSGD whose momentum buffers hold the seeded 0.01 * randn (drawn in the
    oracle's parameter order, placed by name), the architect and the two samples."""
    from test_architect_gpu import golden_net, step_inputs
    z = load_golden(case)
    net = golden_net(z) if net is None else net
    names = list(sub(z, "param/"))
    by_name = dict(zip(names, seeded_buffers([z["param/" + n] for n in names])))
    opt = ClippedSGD(list(net.parameters()), float(z["lr"]), momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]),
                     max_norm=float(z["grad_norm"]))
    with torch.no_grad():
        for (n, _), b in zip(net.named_parameters(), opt.bufs):
            b.copy_(by_name[n])
    architect = SecondOrderArchitect(DEV, net, arch_args(z))
    return z, net, opt, architect, step_inputs(z, "train"), step_inputs(z, "val")


def within(got, ref, what):
    err, scale = float((got.detach().double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: HIP err {err:.3e} (max|ref| {scale:.3e}, allowed {2e-3 * scale + 1e-7:.3e})")
    assert err <= 2e-3 * scale + 1e-7, f"{what}: err {err:.3e}, max|ref| {scale:.3e}"


def record_training_weights(net, is_training):
    """Wraps net._loss: the weights at every pass on the TRAINING sample (is_training(*args) tells)."""
    seen, loss = [], net._loss

    def wrapped(*a):
        if is_training(*a):
            seen.append([p.detach().clone() for p in net.parameters()])
        return loss(*a)

    net._loss = wrapped
    return seen


def buffers_equal_three_training_passes(twin, seen, run, what):
    """The buffers after the step are those of a twin that ran three training-mode forward passes on the training sample (at the
    weights each pass saw: theta, theta + R v, theta - R v) and none on the validation sample."""
    assert len(seen) == 3
    for weights in seen:
        with torch.no_grad():
            for p, w in zip(twin.parameters(), weights):
                p.copy_(w)
        run(twin)
    return dict(twin.named_buffers())


@pytest.mark.parametrize("case", ["architect_tiny", "architect_d24"])
def test_link_prediction_step_matches_the_float64_restatement(case):
    from test_architect_gpu import golden_net
    ref = lp_reference_cached(case)
    z, net, opt, architect, train, val = lp_setup(case)
    lr, alr = float(z["lr"]), float(z["arch_learning_rate"])
    for i in range(4):                                        # on the reference alone: the implicit term is alive
        ratio = lr * float(ref["ig"][i].abs().max()) / float(ref["dalpha"][i].abs().max())
        print(f"{case} alpha {i}: eta * max|ig| / max|dalpha| = {ratio:.3f}")
        assert ratio >= 0.05
    assert isinstance(architect.optimizer, FusedAdam)
    alphas = net.arch_parameters()
    params = list(net.parameters())
    before = [p.detach().clone() for p in params]
    shadow = [a.detach().clone().requires_grad_(True) for a in alphas]
    shadow_opt = torch.optim.Adam(shadow, lr=alr, betas=(0.5, 0.999), weight_decay=float(z["arch_weight_decay"]))
    seen_weights = record_training_weights(net, lambda *a: a[0] is train[0])
    seen = {}
    adam_step = architect.optimizer.step
    architect.optimizer.step = lambda: seen.update(final=[None if a.grad is None else a.grad.clone() for a in alphas]) or adam_step()
    architect.step(*train, *val, lr, opt, True)
    torch.testing.assert_close(architect.loss.detach().double().cpu(), ref["loss"], rtol=1e-4, atol=1e-6)
    for i in range(4):
        within(architect.dalpha[i], ref["dalpha"][i], f"{case} dalpha {i}")
        within(architect.implicit_grads[i], ref["ig"][i], f"{case} implicit_grads {i}")
        within(seen["final"][i], ref["final"][i], f"{case} alpha.grad {i}")
    torch.testing.assert_close(architect.scal[0].double().cpu(), ref["norm"], rtol=2e-3, atol=0.0)
    assert architect.scal.is_cuda and all(t.is_cuda for t in architect.dalpha[:4] + architect.implicit_grads[:4])
    # the score-function alpha of SearchNetwork: no gradient, not stepped
    assert seen["final"][4] is None and alphas[4].grad is None and architect.dalpha[4] is None and architect.implicit_grads[4] is None
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b)                     # bit for bit
    assert all(p.grad is None for p in params)
    for s_, g in zip(shadow, seen["final"]):
        s_.grad = None if g is None else g.clone()
    shadow_opt.step()
    for i in range(5):
        err = float((alphas[i].detach() - shadow[i].detach()).abs().max())
        assert err <= 1e-3 * alr, f"alpha {i} after the step: {err:.3e} from torch.optim.Adam on the same gradients"
    twin = golden_net(z)

    def run(t):
        t._loss(*train)

    want = buffers_equal_three_training_passes(twin, seen_weights, run, case)
    got = dict(net.named_buffers())
    assert got.keys() == want.keys() and len(got) > 0
    for n, b in want.items():
        assert torch.equal(got[n], b), f"buffer {n}: {float((got[n].double() - b.double()).abs().max()):.3e}"
    assert any(n.endswith("num_batches_tracked") and int(b) == int(z["buffer/" + n]) + 3 for n, b in got.items())


def test_score_search_network_gives_the_fifth_alpha_a_gradient():
    from test_sf_mix_gpu import search_case
    net, graph, data, li, _, _, _ = search_case()
    params = list(net.parameters())
    before = [p.detach().clone() for p in params]
    opt = ClippedSGD(params, 0.01, momentum=0.9, weight_decay=3e-4, max_norm=5.0)
    architect = SecondOrderArchitect(DEV, net, arch_args(load_golden("architect_tiny")))
    alphas = net.arch_parameters()
    a4 = alphas[4].detach().clone()
    architect.step(*graph, data, li, *graph, data, li, 0.01, opt, True)
    assert all(a.grad is not None and bool(torch.isfinite(a.grad).all()) for a in alphas)
    assert architect.implicit_grads[4] is not None and float(architect.implicit_grads[4].abs().max()) > 0
    assert not torch.equal(alphas[4].detach(), a4)
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before)) and all(p.grad is None for p in params)


# ---- node classification end to end -------------------------------------------------------------------------------------------
def nc_hip_setup():
    from test_nc_search_cpu import make_net, search_args
    z16, z, inputs = nc_setup()
    net = make_net(z16, "s16", DEV).train()
    params = list(net.parameters())
    opt = ClippedSGD(params, float(z["lr"]), momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]), max_norm=0)
    with torch.no_grad():
        for b, s in zip(opt.bufs, seeded_buffers(params)):
            b.copy_(s)
    trip, labels, (seeds, blocks), (val_seeds, val_blocks) = inputs
    dev_inputs = (trip.to(DEV), labels.to(DEV), (seeds.to(DEV), [b.to(DEV) for b in blocks]), (val_seeds.to(DEV), [b.to(DEV) for b in val_blocks]))
    return z16, z, inputs, net, opt, SecondOrderArchitectNC(DEV, net, search_args(z)), dev_inputs


def test_node_classification_step_matches_the_float64_restatement():
    from test_nc_search_cpu import make_net
    z16, z, inputs, net, opt, architect, (trip, labels, (seeds, blocks), (val_seeds, val_blocks)) = nc_hip_setup()
    ref, _ = nc_reference(z16, z, inputs)
    lr, alr = float(z["lr"]), float(z["arch_learning_rate"])
    alphas, params = net.arch_parameters(), list(net.parameters())
    before = [p.detach().clone() for p in params]
    shadow = [a.detach().clone().requires_grad_(True) for a in alphas]
    shadow_opt = torch.optim.Adam(shadow, lr=alr, betas=(0.5, 0.999), weight_decay=float(z["arch_weight_decay"]))
    seen_weights = record_training_weights(net, lambda *a: a[1] is blocks)       # (both samples share trip: told apart by the blocks)
    seen = {}
    adam_step = architect.optimizer.step
    architect.optimizer.step = lambda: seen.update(final=[a.grad.clone() for a in alphas]) or adam_step()
    architect.step(trip, blocks, labels, seeds, val_blocks, val_seeds, lr, opt, True)
    torch.testing.assert_close(architect.loss.detach().double().cpu(), ref["loss"], rtol=1e-4, atol=1e-6)
    for i in range(4):
        within(architect.dalpha[i], ref["dalpha"][i], f"nc dalpha {i}")
        within(architect.implicit_grads[i], ref["ig"][i], f"nc implicit_grads {i}")
        within(seen["final"][i], ref["final"][i], f"nc alpha.grad {i}")
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b)
    assert all(p.grad is None for p in params)
    for s_, g in zip(shadow, seen["final"]):
        s_.grad = g.clone()
    shadow_opt.step()
    for i in range(4):
        err = float((alphas[i].detach() - shadow[i].detach()).abs().max())
        assert err <= 1e-3 * alr, f"alpha {i} after the step: {err:.3e} from torch.optim.Adam on the same gradients"
    twin = make_net(z16, "s16", DEV).train()
    want = buffers_equal_three_training_passes(twin, seen_weights, lambda t: t._loss(trip, blocks, labels, seeds), "nc")
    got = dict(net.named_buffers())
    assert got.keys() == want.keys() and any(n.endswith("running_mean") for n in got)
    for n, b in want.items():
        assert torch.equal(got[n], b), f"buffer {n}: {float((got[n].double() - b.double()).abs().max()):.3e}"
    assert all(int(b) == 3 for n, b in got.items() if n.endswith("num_batches_tracked"))


# ---- no host reads, stale memory, drivers -------------------------------------------------------------------------------------
def test_the_step_reads_nothing_from_the_device(monkeypatch):
    """Tensor.item / tolist / cpu / __float__ during step(unrolled=True), counted as tests/test_train_nc_gpu.py counts them for an epoch
    (whatever file they are called from) when made on a DEVICE tensor: none.  The first step is a warm-up: the step graphs' plans are
    built once, and their sizes then arrive in pinned host memory (graph._Plan: reading that host tensor is no device read)."""
    z, net, opt, architect, train, val = lp_setup("architect_d24")
    lr = float(z["lr"])
    architect.step(*train, *val, lr, opt, True)
    torch.cuda.synchronize()
    calls = []

    def wrap(nm, fn):
        def counted(t, *a, **k):
            if t.is_cuda:
                f = sys._getframe(1).f_code
                calls.append((nm, f.co_filename.rsplit("/", 1)[-1], f.co_name))
            return fn(t, *a, **k)
        return counted

    with monkeypatch.context() as m:
        for nm in ("item", "tolist", "cpu", "__float__"):
            m.setattr(torch.Tensor, nm, wrap(nm, getattr(torch.Tensor, nm)))
        architect.step(*train, *val, lr, opt, True)
        architect.step(*train, *val, torch.tensor([lr], device=DEV), opt, True)             # eta as a device tensor
    assert calls == [], calls


def test_the_step_does_not_depend_on_stale_memory(monkeypatch):
    """One second-order step from the same start under tests/poison.py: clean, clean, NaN, huge.  The architect is built inside the
    block: its backup buffer, norm partials and scal are allocated uninitialised."""
    runs = []
    for pattern in ("clean", "clean", "nan", "huge"):
        with poisoned(monkeypatch, pattern) as fills:
            z, net, opt, architect, train, val = lp_setup("architect_tiny")
            seen = {}
            adam_step = architect.optimizer.step
            architect.optimizer.step = lambda: seen.update(final=[None if a.grad is None else a.grad.clone() for a in net.arch_parameters()]) or adam_step()
            architect.step(*train, *val, float(z["lr"]), opt, True)
        assert fills.tensors > 0
        runs.append((seen["final"][:4], architect.loss.detach().clone(), [p.detach().clone() for p in net.parameters()],
                     [a.detach().clone() for a in net.arch_parameters()]))
    for k, r in enumerate(runs[1:], 1):
        assert all(torch.equal(a, b) for a, b in zip(r[0], runs[0][0])), f"run {k}: alpha.grad"
        assert torch.equal(r[1], runs[0][1]), f"run {k}: loss"
        assert all(torch.equal(a, b) for a, b in zip(r[2], runs[0][2])), f"run {k}: parameters"
        assert all(torch.equal(a, b) for a, b in zip(r[3], runs[0][3])), f"run {k}: alphas"
    assert bool(torch.isfinite(runs[0][1])) and all(bool(torch.isfinite(g).all()) for g in runs[0][0])


def test_search_epoch_passes_unrolled_through():
    lr = None
    out = {}
    for how in ("plain", "unrolled_false", "unrolled_true"):
        z, net, opt, architect, train, val = lp_setup("architect_tiny")
        lr = float(z["lr"])
        kw = {"plain": {}, "unrolled_false": dict(unrolled=False, eta=None), "unrolled_true": dict(unrolled=True, eta=lr)}[how]
        loss, arch_loss = A.search_epoch(net, architect, opt, train, val, 0, 0, **kw)
        assert loss.is_cuda and bool(torch.isfinite(loss)) and bool(torch.isfinite(arch_loss))
        out[how] = (loss, arch_loss, [a.detach().clone() for a in net.arch_parameters()], [p.detach().clone() for p in net.parameters()])
    a, b, c = out["plain"], out["unrolled_false"], out["unrolled_true"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2] + a[3], b[2] + b[3]))                   # the defaults: today's call, bit for bit
    assert not torch.equal(a[2][0], c[2][0])                                                  # the second-order step moved the alphas elsewhere
    with pytest.raises(ValueError, match="eta"):
        A.search_epoch(net, architect, opt, train, val, 0, 0, unrolled=True)


def test_search_step_passes_unrolled_through():
    out = {}
    for how in ("plain", "unrolled_false", "unrolled_true"):
        z16, z, _, net, opt, architect, (trip, labels, train, val) = nc_hip_setup()
        lr = float(z["lr"])
        kw = {"plain": {}, "unrolled_false": dict(unrolled=False), "unrolled_true": dict(unrolled=True)}[how]
        loss, arch_loss, logits = AN.search_step(net, architect, opt, trip, train, val, labels, 1, 0, torch.nn.CrossEntropyLoss(), lr, **kw)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(arch_loss)) and bool(torch.isfinite(logits).all())
        out[how] = (loss, arch_loss, logits, [a.detach().clone() for a in net.arch_parameters()], [p.detach().clone() for p in net.parameters()])
    a, b, c = out["plain"], out["unrolled_false"], out["unrolled_true"]
    assert all(torch.equal(a[k], b[k]) for k in range(3))
    assert all(torch.equal(x, y) for x, y in zip(a[3] + a[4], b[3] + b[4]))
    assert not torch.equal(a[3][0], c[3][0])
