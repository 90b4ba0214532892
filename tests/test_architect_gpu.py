"""optim.FusedAdam (mrg_adam_step) against torch.optim.Adam in float32 and float64, and architect.Architect / search_epoch on the HIP
supernet against three epochs of the reference's own search loop (tests/golden/make_golden_architect.py).

The Adam criterion, everywhere below: three optimisers run on the device from the same start -- FusedAdam, torch.optim.Adam in
float32, torch.optim.Adam in float64 (the truth) -- and after every step, for every tensor,

    max|fused - f64|  <=  2 * max|torch32 - f64|  +  2^-23 * max|p|

The yardstick is torch's own float32 error, measured in the same test; the factor 2 covers a different contraction and a different
sqrt / divide rounding, the last term one rounding of the stored parameter."""
import types

import pytest
import torch

from conftest import assert_param_grad, load_golden, sub
from mr_gnas_amd import graph as G, supernet as S
from mr_gnas_amd._lib import MrgnasError
from mr_gnas_amd.architect import Architect, search_epoch
from mr_gnas_amd.optim import ClippedSGD, FusedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"

# tests/test_ops_gpu.py::test_clipped_sgd_equals_torch_clip_grad_norm_and_sgd's shapes (ragged sizes around the 4096-element chunk) + a small one
SHAPES = [(200, 400), (200,), (1,), (4096,), (4097,), (3, 5, 7), (14541, 100), (475, 200), (8191,), (6, 5)]
NEVER, MISSES_STEP_1, SMALL_GRADS = 2, 4, 9


def trio(shapes, gen):
    mine = [torch.randn(*s, device=DEV, generator=gen).requires_grad_(True) for s in shapes]
    t32 = [p.detach().clone().requires_grad_(True) for p in mine]
    t64 = [p.detach().double().requires_grad_(True) for p in mine]
    return mine, t32, t64


def feed(step, sets, gen):
    """The same random gradients to every parameter set: one tensor never gets one, one misses step 1, step 3's are 100 x smaller,
    the last tensor's 1000 x smaller."""
    for i, ps in enumerate(zip(*sets)):
        if i == NEVER or (i == MISSES_STEP_1 and step == 1):
            for p in ps:
                p.grad = None
            continue
        g = torch.randn(ps[0].shape, device=DEV, generator=gen) * (0.01 if step == 3 else 1.0) * (1e-3 if i == SMALL_GRADS else 1.0)
        for p in ps:
            p.grad = g.to(p.dtype).clone()


def assert_within_twice_torch(mine, t32, t64, what):
    rows = torch.stack([torch.stack(((a.detach().double() - c.detach()).abs().max(), (b.detach().double() - c.detach()).abs().max(),
                                     c.detach().abs().max())) for a, b, c in zip(mine, t32, t64)]).cpu()
    for i, (e_mine, e_torch, pmax) in enumerate(rows.tolist()):
        bound = 2.0 * e_torch + 2.0 ** -23 * pmax
        print(f"{what} tensor {i}: fused err {e_mine:.3e} torch32 err {e_torch:.3e} bound {bound:.3e}")
        assert e_mine <= bound, f"{what} tensor {i}: |fused - f64| {e_mine:.3e} > 2 * {e_torch:.3e} + 2^-23 * {pmax:.3e}"


@pytest.mark.parametrize("betas,wd", [((0.9, 0.999), 0.0), ((0.5, 0.999), 1e-3), ((0.9, 0.999), 3e-4)])
def test_fused_adam_is_as_accurate_as_torch_adam(betas, wd):
    gen = torch.Generator(device=DEV).manual_seed(3)
    mine, t32, t64 = trio(SHAPES, gen)
    start = mine[NEVER].detach().clone()
    opt = FusedAdam(mine, lr=1e-3, betas=betas, weight_decay=wd)
    o32 = torch.optim.Adam(t32, lr=1e-3, betas=betas, weight_decay=wd)
    o64 = torch.optim.Adam(t64, lr=1e-3, betas=betas, weight_decay=wd)
    for step in range(6):
        feed(step, (mine, t32, t64), gen)
        for o in (opt, o32, o64):
            o.step()
        assert_within_twice_torch(mine, t32, t64, f"betas {betas} wd {wd} step {step}")
    assert torch.equal(mine[NEVER].detach(), start)                       # never had a gradient: untouched, bit for bit
    steps = [float(opt.state[p]["step"]) for p in mine]
    assert steps[NEVER] == 0 and steps[MISSES_STEP_1] == 5 and all(s == 6 for i, s in enumerate(steps) if i not in (NEVER, MISSES_STEP_1))
    for p, q in zip(mine, t32):                                           # per-parameter counts, as torch keeps them
        assert float(opt.state[p]["step"]) == (float(o32.state[q]["step"]) if q in o32.state else 0.0)
        assert opt.state[p]["exp_avg"].shape == p.shape and opt.state[p]["exp_avg_sq"].shape == p.shape


def test_fused_adam_edge_cases():
    gen = torch.Generator(device=DEV).manual_seed(4)
    # a non-contiguous gradient; parameters and gradients that are NOT 16-byte aligned (contiguous views at odd element offsets,
    # more than one chunk): the 4-byte path, chunk by chunk
    base = torch.randn(3 + 9000, device=DEV, generator=gen)
    head = base[:3].clone()
    mine = [torch.randn(200, 400, device=DEV, generator=gen).requires_grad_(True), base[3:].detach().requires_grad_(True),
            torch.randn(37, device=DEV, generator=gen).requires_grad_(True)]
    assert mine[1].data_ptr() % 16 == 12 and mine[1].is_contiguous()
    t32 = [p.detach().clone().requires_grad_(True) for p in mine]
    t64 = [p.detach().double().requires_grad_(True) for p in mine]
    opt, o32, o64 = FusedAdam(mine, lr=1e-2), torch.optim.Adam(t32, lr=1e-2), torch.optim.Adam(t64, lr=1e-2)
    for step in range(3):
        g0 = torch.randn(400, 200, device=DEV, generator=gen).t()
        g1 = torch.randn(2 + 9000, device=DEV, generator=gen)[2:]
        g2 = torch.randn(1 + 37, device=DEV, generator=gen)[1:]
        assert not g0.is_contiguous() and g1.data_ptr() % 16 == 8
        for ps, g in zip(zip(mine, t32, t64), (g0, g1, g2)):
            ps[0].grad = g                                                # as it is: strided / unaligned
            ps[1].grad, ps[2].grad = g.clone(), g.double()
        for o in (opt, o32, o64):
            o.step()
        assert_within_twice_torch(mine, t32, t64, f"edge cases step {step}")
    assert torch.equal(base[:3], head)                                    # the elements in front of the unaligned view: untouched
    # one parameter group; the flags of torch's Adam this one does not implement are not accepted
    a, b = (torch.zeros(4, device=DEV, requires_grad=True) for _ in range(2))
    with pytest.raises(ValueError):
        FusedAdam([{"params": [a]}, {"params": [b], "lr": 1e-2}])
    opt = FusedAdam([{"params": [a, b]}])
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.zeros(4, device=DEV, requires_grad=True)]})
    for flag in ("amsgrad", "maximize", "foreach", "fused", "differentiable"):
        with pytest.raises(TypeError):
            FusedAdam([a], **{flag: True})
    with pytest.raises(MrgnasError):
        FusedAdam([torch.zeros(4, 6, device=DEV).t().requires_grad_(True)])             # non-contiguous parameter
    with pytest.raises(MrgnasError):
        FusedAdam([torch.zeros(4, device=DEV, dtype=torch.float64, requires_grad=True)])


def test_fused_adam_takes_over_torch_adam_state_and_round_trips():
    gen = torch.Generator(device=DEV).manual_seed(5)
    mine, t32, t64 = trio(SHAPES, gen)
    o32 = torch.optim.Adam(t32, lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-3)
    o64 = torch.optim.Adam(t64, lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-3)
    for step in range(2):                                                 # torch alone: one tensor still has no state, one lags a step behind
        feed(step, (t32, t64), gen)
        o32.step()
        o64.step()
    with torch.no_grad():
        for p, q in zip(mine, t32):
            p.copy_(q)
    opt = FusedAdam(mine)                                                  # other hyper-parameters: the state dict brings torch's
    m_ptr = opt.state[mine[0]]["exp_avg"].data_ptr()
    opt.load_state_dict(o32.state_dict())
    assert opt.state[mine[0]]["exp_avg"].data_ptr() == m_ptr              # copied INTO the flat buffers
    g = opt.param_groups[0]
    assert g["lr"] == 1e-3 and tuple(g["betas"]) == (0.5, 0.999) and g["weight_decay"] == 1e-3
    assert float(opt.state[mine[NEVER]]["step"]) == 0 and float(opt.state[mine[MISSES_STEP_1]]["step"]) == 1 and float(opt.state[mine[0]]["step"]) == 2
    for step in range(2, 4):
        feed(step, (mine, t32, t64), gen)
        for o in (opt, o32, o64):
            o.step()
        assert_within_twice_torch(mine, t32, t64, f"after torch's state, step {step}")
    # state_dict() -> load_state_dict() on a second optimiser: the same bits, and the same next step
    sd = opt.state_dict()
    twin = [p.detach().clone().requires_grad_(True) for p in mine]
    opt2 = FusedAdam(twin)
    opt2.load_state_dict(sd)
    for p, q in zip(mine, twin):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k], opt2.state[q][k]), k
    sd2 = opt2.state_dict()
    assert sd2["param_groups"] == sd["param_groups"]
    assert all(torch.equal(sd["state"][i][k], sd2["state"][i][k]) for i in sd["state"] for k in sd["state"][i])
    feed(4, (mine, twin), gen)
    opt.step()
    opt2.step()
    assert all(torch.equal(p, q) for p, q in zip(mine, twin))


def test_fused_adam_replays_from_a_hip_graph_and_follows_set_lr():
    """backward + FusedAdam.step() captured once and replayed (after tests/test_ops_gpu.py::test_clipped_sgd_replays_from_a_hip_graph):
    the step counts and the learning rate live in device memory, so every replay advances its own bias correction and set_lr()
    between replays is followed -- one eager step, three replays, the rate halved before the third."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    W = [torch.randn(64, 200, device=DEV, generator=gen).requires_grad_(True), torch.randn(5000, device=DEV, generator=gen).requires_grad_(True)]
    r32 = [w.detach().clone().requires_grad_(True) for w in W]
    r64 = [w.detach().double().requires_grad_(True) for w in W]
    x = torch.randn(32, 200, device=DEV, generator=gen)
    lr = 1e-2
    opt, o32, o64 = FusedAdam(W, lr=lr), torch.optim.Adam(r32, lr=lr), torch.optim.Adam(r64, lr=lr)

    def step(ws, o):
        loss = (x.to(ws[0].dtype) @ ws[0].t()).square().mean() + ws[1].square().sum() * 1e-3
        loss.backward()
        o.step()
        o.zero_grad(set_to_none=True)

    def both():
        step(r32, o32)
        step(r64, o64)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(W, opt)                                          # warm-up (eager)
    torch.cuda.current_stream().wait_stream(side)
    both()
    torch.cuda.synchronize()
    assert_within_twice_torch(W, r32, r64, "eager step")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step(W, opt)
    for k in range(3):
        if k == 2:
            opt.set_lr(0.5 * lr)
            o32.param_groups[0]["lr"] = o64.param_groups[0]["lr"] = 0.5 * lr
        graph.replay()
        both()
        torch.cuda.synchronize()
        assert_within_twice_torch(W, r32, r64, f"replay {k}")
    assert [float(opt.state[w]["step"]) for w in W] == [4.0, 4.0] and opt.param_groups[0]["lr"] == 0.5 * lr


# ---------------------------------------------------------------------------
# the architect
# ---------------------------------------------------------------------------
def arch_args(z):
    return types.SimpleNamespace(momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]),
                                 arch_learning_rate=float(z["arch_learning_rate"]), arch_weight_decay=float(z["arch_weight_decay"]))


def step_inputs(z, which):
    n = z[which + "/node_id"].numel()
    g = G.RelGraph(n, z[which + "/src"], z[which + "/dst"], z[which + "/edge_type"], z[which + "/norm"], device=DEV)
    return (g,) + tuple(z[f"{which}/{k}"].to(DEV) for k in ("node_id", "src_in", "edge_type", "data", "labels"))


def golden_net(z, epoch=0):
    net = S.SearchNetwork(DEV, z["Nall"], z["R"], z["layers"], 1, 2, 2, z["D"], z["D0"], z["nbase"], 9.0, 0.0, 0.0).to(DEV)
    net.load_state_dict({**sub(z, "param/"), **sub(z, "buffer/")})
    net.load_alpha([z[f"e{epoch}/alpha_before/{i}"].to(DEV) for i in range(5)])
    net.train()
    return net


def as_gparam(d):
    return {"gparam/" + k: v for k, v in d.items()}


@pytest.mark.parametrize("case", ["architect_tiny", "architect_d24"])
def test_search_epochs_match_the_reference(case):
    """tests/test_architect_cpu.py's procedure on SearchNetwork with FusedAdam (inside Architect) and ClippedSGD(max_norm = grad_norm),
    to tests/test_nets_gpu.py's tolerances.  The alphas after the architect step are compared with a shadow torch.optim.Adam that is
    fed the test's OWN alpha gradients from the same alpha_before: that pins the Adam arithmetic to 1e-3 * lr, apart from the
    gradients' tolerance.  The weight step (before - after) / lr is compared with the same quantity of the fixture; both sides carry
    the rounding of their float32 parameters, half an ulp each, so 2^-23 * max|p| / lr is added to the absolute tolerance."""
    z = load_golden(case)
    lr, alr, clip = float(z["lr"]), float(z["arch_learning_rate"]), float(z["grad_norm"])
    net = golden_net(z)
    params = dict(net.named_parameters())
    optimizer = ClippedSGD(list(net.parameters()), lr, momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]), max_norm=clip)
    architect = Architect(DEV, net, arch_args(z))
    assert isinstance(architect.optimizer, FusedAdam)
    alphas = net.arch_parameters()
    shadow = [a.detach().clone().requires_grad_(True) for a in alphas]
    shadow_opt = torch.optim.Adam(shadow, lr=alr, betas=(0.5, 0.999), weight_decay=float(z["arch_weight_decay"]))
    train, val = step_inputs(z, "train"), step_inputs(z, "val")
    seen = {}
    adam_step, sgd_step = architect.optimizer.step, optimizer.step

    def after_architect_backward():
        seen["galpha"] = [None if a.grad is None else a.grad.clone() for a in alphas]
        seen["gparam_val"] = {n: (None if p.grad is None else p.grad.clone()) for n, p in params.items()}
        return adam_step()

    def before_weight_step():
        seen["gparam_acc"] = {n: (None if p.grad is None else p.grad.clone()) for n, p in params.items()}
        seen["alpha_after"] = [a.detach().clone() for a in alphas]
        return sgd_step()

    architect.optimizer.step, optimizer.step = after_architect_backward, before_weight_step
    for e in range(z["epochs"]):
        net.load_alpha([z[f"e{e}/alpha_before/{i}"].to(DEV) for i in range(5)])
        with torch.no_grad():
            for s_, a in zip(shadow, alphas):
                s_.copy_(a)
        before = {n: p.detach().clone() for n, p in params.items()}
        loss, arch_loss = search_epoch(net, architect, optimizer, train, val, e, 0)
        assert loss.is_cuda and arch_loss.is_cuda
        print(f"{case} epoch {e}: loss {float(loss):.7f} (ref {float(z[f'e{e}/loss']):.7f}) arch loss {float(arch_loss):.7f} "
              f"(ref {float(z[f'e{e}/arch_loss']):.7f}) norm {float(optimizer.norm_coef[0]):.5f} (ref {float(z[f'e{e}/grad_norm']):.5f})")
        torch.testing.assert_close(arch_loss.cpu(), z[f"e{e}/arch_loss"], rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(loss.cpu(), z[f"e{e}/loss"], rtol=1e-4, atol=1e-6)
        for i in range(4):
            ref = z[f"e{e}/galpha/{i}"]
            err = float((seen["galpha"][i].cpu() - ref).abs().max())
            assert err <= 2e-3 * max(float(ref.abs().max()), 1e-8) + 1e-7, f"epoch {e} alpha {i}: gradient err {err:.3e}"
        assert seen["galpha"][4] is None and torch.equal(alphas[4].detach().cpu(), z[f"e{e}/alpha_before/4"])
        for s_, g in zip(shadow, seen["galpha"]):
            s_.grad = None if g is None else g.clone()
        shadow_opt.step()
        for i in range(5):
            err = float((seen["alpha_after"][i] - shadow[i].detach()).abs().max())
            ref_err = float((seen["alpha_after"][i].cpu() - z[f"e{e}/alpha_after/{i}"]).abs().max())
            print(f"{case} epoch {e} alpha {i}: vs shadow Adam {err:.2e} (allowed {1e-3 * alr:.1e}), vs the reference's {ref_err:.2e}")
            assert err <= 1e-3 * alr, f"epoch {e} alpha {i} after the step: {err:.3e} from torch.optim.Adam on the same gradients"
        norm, ref_norm = float(optimizer.norm_coef[0]), float(z[f"e{e}/grad_norm"])
        assert abs(norm - ref_norm) <= 1e-3 * ref_norm, f"epoch {e}: gradient norm {norm} vs {ref_norm}"
        if e == 0:
            zv, za = as_gparam(sub(z, "e0/gparam_val/")), as_gparam(sub(z, "e0/gparam_acc/"))
            assert sorted(sub(z, "e0/gparam_acc/")) == sorted(params)
            for n in sub(z, "e0/gparam_val/"):
                assert_param_grad(zv, n, seen["gparam_val"][n], 2e-3, 5e-6, case + " validation")
            for n in params:
                assert_param_grad(za, n, seen["gparam_acc"][n], 2e-3, 5e-6, case + " validation+training")
            for n, after in sub(z, "e0/param_after/").items():
                zs = {"gparam/" + n: (z["param/" + n].double() - after.double()) / lr}
                got = (before[n].double() - params[n].detach().double()) / lr
                rounding = 2.0 ** -23 * float(z["param/" + n].abs().max()) / lr
                assert_param_grad(zs, n, got, 2e-3, 5e-6 + rounding, case + " weight step")
        assert all(p.grad is None for p in params.values())


def test_weight_grads_false_gives_the_same_alpha_gradients_and_no_weight_gradients():
    z = load_golden("architect_d24")
    val = step_inputs(z, "val")
    train = step_inputs(z, "train")
    res = {}
    for mode in (True, False):
        net = golden_net(z)
        architect = Architect(DEV, net, arch_args(z), weight_grads=mode)
        architect.step(*train, *val, None, None, False)
        res[mode] = ([None if a.grad is None else a.grad.clone() for a in net.arch_parameters()],
                     [p.grad for p in net.parameters()], {k: v.clone() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k},
                     architect.loss.detach().clone(), [a.detach().clone() for a in net.arch_parameters()])
    assert all(g is not None for g in res[True][1]) and all(g is None for g in res[False][1])
    assert res[True][0][4] is None and res[False][0][4] is None
    for i in range(4):
        a, b = res[False][0][i], res[True][0][i]
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        print(f"alpha {i}: gradient without weight gradients differs by {err:.2e} (max {scale:.2e})")
        assert err <= 1e-6 * scale
    assert res[True][2].keys() == res[False][2].keys() and len(res[True][2]) > 0
    for k, v in res[True][2].items():
        assert torch.equal(res[False][2][k], v), k
    assert torch.equal(res[True][3], res[False][3])


def test_architect_step_replays_from_a_hip_graph(monkeypatch):
    """architect.step() -- supernet forward, backward, FusedAdam -- captured once (one stream, as bench.py captures a step) and replayed
    twice after an eager warm-up on a side stream, against a twin stepped eagerly three times."""
    from mr_gnas_amd import cell_lp as CL, functional as K
    monkeypatch.setattr(CL, "MIXED_STREAMS", 1)
    monkeypatch.setattr(K.switches, "SEGMENT_STREAMS", 1)
    z = load_golden("architect_d24")
    alr = float(z["arch_learning_rate"])
    train, val = step_inputs(z, "train"), step_inputs(z, "val")
    net, twin = golden_net(z), golden_net(z)
    architect, twin_architect = Architect(DEV, net, arch_args(z)), Architect(DEV, twin, arch_args(z))

    def step(a):
        a.step(*train, *val, None, None, False)
        for p in a.model.parameters():
            p.grad = None

    for _ in range(3):
        step(twin_architect)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(architect)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step(architect)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(net.arch_parameters(), twin.arch_parameters())):
        err = float((a.detach() - b.detach()).abs().max())
        print(f"alpha {i}: captured vs eager {err:.2e} (allowed {1e-3 * alr:.1e})")
        assert err <= 1e-3 * alr
    torch.testing.assert_close(architect.loss.detach(), twin_architect.loss.detach(), rtol=1e-6, atol=0.0)
    assert [float(architect.optimizer.state[a]["step"]) for a in net.arch_parameters()] == [3.0, 3.0, 3.0, 3.0, 0.0]
