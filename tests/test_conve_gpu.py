"""ConvE scorers on the MI355X (csrc/conve.hip, functional/conve.py): sf_ConvE_op (reference models/operations_lp.py:150-205),
CompGCN_ConvE (models/compgcn.py:188-269) and the training driver's default genotype on FixedNetwork, against the reference's
fixtures and, at full size, against a float64 host evaluation; the HIP path is taken, dropout draws torch's masks, two runs give
the same bits, a captured graph replays the eager result, and the fallbacks run torch's formulation."""
import copy

import pytest
import torch

from conftest import assert_param_grad, load_golden, record_margin, seeded, sub
from mr_gnas_amd import _lib, compgcn as CG, graph as G, operations_lp as O, supernet as S
from mr_gnas_amd import functional as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONVE_FNS = ["mrg_conve_bn0_fwd", "mrg_conve_conv_fwd", "mrg_conve_bn1_fwd", "mrg_conve_fc_fwd", "mrg_conve_fc_bwd",
             "mrg_conve_bn1_bwd", "mrg_conve_conv_bwd", "mrg_conve_finish_bwd"]


def sf_op(z, tag):
    B, N, D, k_h, k_w, ks, F = (int(v) for v in z[f"{tag}/args"])
    op = O.sf_ConvE_op({"embed_dim": D, "conve_hid_drop": 0.0, "feat_drop": 0.0, "num_filt": F, "ker_sz": ks, "k_w": k_w, "k_h": k_h})
    op.load_state_dict(sub(z, f"{tag}/param0/"))
    return op


def run_sf(op, z, tag, dev=DEV, dtype=torch.float32):
    op = op.to(dev, dtype)
    ins = [z[f"{tag}/{n}"].to(dev, dtype).requires_grad_(True) for n in ("ent", "sub", "rel")]
    op.train()
    pred = op(*ins)
    loss = torch.nn.functional.binary_cross_entropy(pred, z[f"{tag}/label"].to(dev, dtype))
    loss.backward()
    return op, ins, pred, loss


def check_sf(z, tag, op, ins, pred, loss, what, eval_too=True, buffers=True):
    zt = sub(z, f"{tag}/")
    torch.testing.assert_close(pred.detach().float().cpu(), zt["pred"], rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(loss.detach().float().cpu(), zt["loss"], rtol=1e-4, atol=1e-6)
    for t, n in zip(ins, ("gent", "gsub", "grel")):
        assert_param_grad({"gparam/" + n: zt[n]}, n, t.grad.float(), 5e-4, 5e-6, what)
    for n, p in op.named_parameters():
        assert_param_grad(zt, n, p.grad.float(), 5e-4, 5e-6, what)
    if buffers:
        bufs = dict(op.named_buffers())
        for n, ref in sub(zt, "buffer/").items():
            torch.testing.assert_close(bufs[n].cpu().to(ref.dtype), ref, rtol=1e-4, atol=1e-5)
    if eval_too:
        op.eval()
        with torch.no_grad():
            got = op(*[t.detach() for t in ins])
        torch.testing.assert_close(got.float().cpu(), zt["pred_eval"], rtol=1e-4, atol=5e-5)


def test_hip_path_taken(monkeypatch):
    z = load_golden("conve_sf_small")

    def refuse(*a, **k):
        raise AssertionError("torch conv2d reached: the ConvE scorer fell back to torch")

    monkeypatch.setattr(torch.nn.functional, "conv2d", refuse)
    monkeypatch.setattr(torch, "conv2d", refuse)
    _lib.meter.start(CONVE_FNS)
    try:
        run_sf(sf_op(z, "s1"), z, "s1")
    finally:
        rec = _lib.meter.stop()
    assert sorted(rec) == sorted(CONVE_FNS)
    assert all(r["launches"] == 1 for r in rec.values())


@pytest.mark.parametrize("tag", ["s0", "s1", "s2"])
def test_sf_conve_matches_the_reference(tag):
    z = load_golden("conve_sf_small")
    op, ins, pred, loss = run_sf(sf_op(z, tag), z, tag)
    check_sf(z, tag, op, ins, pred, loss, f"conve_sf_small/{tag}")


def compgcn_case(z):
    g = G.RelGraph(z["N"], z["src"], z["dst"], z["etype"], z["norm"], device=DEV)
    m = z["in_edges_mask"].to(DEV)
    g.edata["etype"], g.edata["in_edges_mask"], g.edata["out_edges_mask"] = z["etype"].to(DEV), m, ~m
    g.edata["norm"] = z["norm"].to(DEV)
    net = CG.CompGCN_ConvE(z["nb"], 2 * z["R"], z["N"], z["Din"], [z["Dout"]], comp_fn="sub", dropout=0.0, layer_dropout=[0.0],
                           num_filt=z["F"], hid_drop=0.0, feat_drop=0.0, ker_sz=z["ks"], k_w=z["k_w"], k_h=z["k_h"])
    net.load_state_dict(sub(z, "param0/"))
    return g, net.to(DEV)


def test_compgcn_conve_matches_the_reference():
    z = load_golden("conve_compgcn_small")
    g, net = compgcn_case(z)
    net.train()
    _lib.meter.start(["mrg_conve_conv_fwd"])
    pred = net(g, z["subj"].to(DEV), z["rel"].to(DEV))
    assert _lib.meter.stop()["mrg_conve_conv_fwd"]["launches"] == 1
    loss = torch.nn.functional.binary_cross_entropy(pred, z["label"].to(DEV))
    loss.backward()
    torch.testing.assert_close(pred.detach().cpu(), z["pred"], rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(loss.detach().cpu(), z["loss"], rtol=1e-4, atol=1e-6)
    assert sorted(n for n, _ in net.named_parameters()) == sorted(sub(z, "gparam/"))
    for n, p in net.named_parameters():
        assert_param_grad(z, n, p.grad, 5e-4, 5e-6, "conve_compgcn_small")
    bufs = dict(net.named_buffers())
    for n, ref in sub(z, "buffer/").items():
        torch.testing.assert_close(bufs[n].cpu(), ref, rtol=1e-4, atol=1e-5)
    net.eval()
    with torch.no_grad():
        got = net(g, z["subj"].to(DEV), z["rel"].to(DEV))
    torch.testing.assert_close(got.cpu(), z["pred_eval"], rtol=1e-4, atol=5e-5)


def test_fixed_network_with_the_training_drivers_genotype():
    z = load_golden("fixednet_conve")
    genotype = eval(z["genotype"], {"Genotype": S.Genotype})
    D, F, ks, k_w, k_h = (int(v) for v in z["score_args"])
    args = {"gamma": 40.0, "embed_dim": D, "conve_hid_drop": 0.0, "feat_drop": 0.0, "num_filt": F, "ker_sz": ks, "k_w": k_w, "k_h": k_h}
    g = G.RelGraph(z["N"], z["src"], z["dst"], z["etype"], z["norm"], device=DEV)
    net = S.FixedNetwork(DEV, genotype, z["N"], z["R"], z["D"], z["D0"], z["nbase"], score_args=args).to(DEV)
    net.load_state_dict({**sub(z, "param/"), **sub(z, "buffer0/")})
    net.train()
    _lib.meter.start(["mrg_conve_conv_fwd"])
    pred = net(g, z["subj"].to(DEV), z["rel"].to(DEV))
    assert _lib.meter.stop()["mrg_conve_conv_fwd"]["launches"] == 1
    loss = torch.nn.functional.binary_cross_entropy(pred, z["label"].to(DEV))
    loss.backward()
    torch.testing.assert_close(pred.detach().cpu(), z["pred"], rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(loss.detach().cpu(), z["loss"], rtol=1e-4, atol=1e-6)
    assert sorted(n for n, _ in net.named_parameters()) == sorted(sub(z, "gparam/"))
    for n, p in net.named_parameters():
        assert_param_grad(z, n, p.grad if p.grad is not None else torch.zeros_like(p), 5e-4, 5e-6, "fixednet_conve")
    bufs = dict(net.named_buffers())
    for n, ref in sub(z, "buffer/").items():
        torch.testing.assert_close(bufs[n].cpu(), ref, rtol=1e-4, atol=1e-5)
    net.eval()
    with torch.no_grad():
        got = net(g, z["subj"].to(DEV), z["rel"].to(DEV))
    torch.testing.assert_close(got.cpu(), z["pred_eval"], rtol=1e-4, atol=5e-5)


# ---- full size against float64 on the host ------------------------------------------------------------------------------------
FULL = {  # name: (layout, D, k_h, k_w, ks, F) -- the train driver's default, sf_ConvE_op's defaults, CompGCN_ConvE at D = 200
    "train_default": ("sf", 128, 16, 8, 8, 128),
    "sf_defaults": ("sf", 200, 20, 10, 7, 200),
    "compgcn_d200": ("compgcn", 200, 20, 10, 7, 200),
}


CANCELLING = ("bn0.weight", "bn0.bias", "conv2d.bias", "fc.bias")


class _Scorer(torch.nn.Module):
    """The ConvE scorer of either module on given rows: sf_ConvE_op itself, or CompGCN_ConvE's scorer part (its submodules, the
    interleaved image and the score bias) on a seeded n_feats instead of a CompGCN pass."""

    def __init__(self, kind, D, k_h, k_w, ks, F, N):
        super().__init__()
        self.kind = kind
        if kind == "sf":
            self.op = O.sf_ConvE_op({"embed_dim": D, "conve_hid_drop": 0.0, "feat_drop": 0.0, "num_filt": F, "ker_sz": ks,
                                     "k_w": k_w, "k_h": k_h})
        else:
            self.op = CG.CompGCN_ConvE(0, 2, 2, 4, [D], num_filt=F, hid_drop=0.0, feat_drop=0.0, ker_sz=ks, k_w=k_w, k_h=k_h)
            del self.op.compGCN_Model
            self.op.bias = torch.nn.Parameter(torch.zeros(N))

    def forward(self, ent, s, r):
        op = self.op
        if self.kind == "sf":
            return op(ent, s, r)
        if K.conve.hip_path_ok((op.bn0, op.m_conv1, op.bn1, op.fc, op.bn2), (op.bn0, op.bn1, op.bn2), (ent, s, r)):
            return K.conve_scores(s, r, K.conve.INTERLEAVED, (2 * op.k_w, op.k_h), op.bn0, op.m_conv1, op.bn1, op.feature_drop, op.fc,
                                  op.hidden_drop, op.bn2, op._one, ent, op.bias)
        x = op.bn0(op.concat(s, r))
        x = torch.relu(op.bn1(op.m_conv1(x)))
        x = torch.relu(op.bn2(op.fc(x.view(-1, op.flat_sz))))
        return torch.sigmoid(x @ ent.t() + op.bias)


def seeded_scorer(name, N, seed=5):
    kind, D, k_h, k_w, ks, F = FULL[name]
    m = _Scorer(kind, D, k_h, k_w, ks, F, N)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(seeded(n, p.shape, seed, 0.1, 1.0) if p.dim() == 1 and n.endswith("weight") else
                    seeded(n, p.shape, seed, 0.05 if p.dim() == 1 else (1.0 / max(p[0].numel(), 1)) ** 0.5))
    return m


@pytest.mark.parametrize("name", list(FULL))
def test_full_size_against_float64(name):
    B, N = 256, 14541
    D = FULL[name][1]
    m = seeded_scorer(name, N)
    ent, s, r = seeded("ent", (N, D), 1, 0.1), seeded("sub", (B, D), 2), seeded("rel", (B, D), 3)
    gout = seeded("gout", (B, N), 4)
    res = {}
    for tag, dev, dt in (("hip", DEV, torch.float32), ("torch32", DEV, torch.float32), ("ref", "cpu", torch.float64)):
        mm = copy.deepcopy(m).to(dev, dt).train()
        if tag == "torch32":                                        # a hooked submodule: torch's formulation in float32
            mm.op.bn0.register_forward_hook(lambda *a: None)
        xs = [t.to(dev, dt).requires_grad_(True) for t in (ent, s, r)]
        out = mm(*xs)
        (out * gout.to(dev, dt)).sum().backward()
        res[tag] = {"out": out.detach(), **{f"g{i}": x.grad for i, x in enumerate(xs)},
                    **{n: p.grad for n, p in mm.named_parameters()}}
    for k, ref in res["ref"].items():
        got = res["hip"][k].double().cpu()
        scale = float(ref.abs().max())
        tol = (1e-5 if k == "out" else 1e-4) * max(scale, 1e-30)
        # sums that cancel: the gradients of BN0's bias, the conv bias and the fc bias are 0 in exact arithmetic (a BatchNorm
        # follows each in training mode), BN0's gain gradient is one sum over all 2 B D pixels that cancels to ~1e-4 of its terms.
        # No float32 evaluation reaches 1e-4 of their values: they are bounded by the error of torch's own float32 formulation
        if k.endswith(CANCELLING):
            tol = max(tol, 10 * float((res["torch32"][k].double().cpu() - ref).abs().max()))
        err = float((got - ref).abs().max())
        record_margin(f"conve_full/{name}", k, err, scale, tol)
        assert err <= tol, f"{name} {k}: err {err:.3e} scale {scale:.3e}"


def test_dropout_masks_are_torchs():
    B, N, D, k_h, k_w, ks, F = 64, 300, 32, 8, 4, 3, 16
    op = O.sf_ConvE_op({"embed_dim": D, "conve_hid_drop": 0.3, "feat_drop": 0.2, "num_filt": F, "ker_sz": ks, "k_w": k_w, "k_h": k_h})
    op = op.to(DEV).train()
    ref_op = copy.deepcopy(op)
    ins = [seeded(n, (R, D), 9).to(DEV) for n, R in (("ent", N), ("sub", B), ("rel", B))]
    outs = []
    for mod, hip in ((op, True), (ref_op, False)):
        xs = [t.clone().requires_grad_(True) for t in ins]
        torch.manual_seed(17)
        if hip:
            y = mod(*xs)
        else:
            h = mod.conv2d.register_forward_hook(lambda *a: None)     # a hooked submodule: torch's formulation
            y = mod(*xs)
            h.remove()
        y.square().sum().backward()
        outs.append([y.detach()] + [x.grad for x in xs] + [p.grad for p in mod.parameters()])
    names = ["out", "gent", "gsub", "grel"] + [n for n, _ in op.named_parameters()]
    wscale = float(outs[1][names.index("conv2d.weight")].abs().max())
    for n, a, b in zip(names, *outs):
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        if n.endswith(CANCELLING):            # sums that cancel (see CANCELLING): measured against the conv weight gradient's scale
            scale = max(scale, wscale)
        assert err <= 2e-4 * scale + 1e-6, f"{n}: err {err:.3e} scale {scale:.3e}"


def test_two_runs_are_bitwise_equal():
    z = load_golden("conve_sf_small")
    res = []
    for _ in range(2):
        op, ins, pred, _ = run_sf(sf_op(z, "s2"), z, "s2")
        res.append([pred.detach()] + [t.grad for t in ins] + [p.grad for p in op.parameters()] + [b.clone() for b in op.buffers()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_graph_capture_replays_the_eager_step():
    z = load_golden("conve_sf_small")
    tag = "s1"
    op_e, op_g = sf_op(z, tag).to(DEV).train(), sf_op(z, tag).to(DEV).train()
    ins = [z[f"{tag}/{n}"].to(DEV) for n in ("ent", "sub", "rel")]
    label = z[f"{tag}/label"].to(DEV)

    def step(op, xs):
        y = op(*xs)
        loss = torch.nn.functional.binary_cross_entropy(y, label)
        return [y.detach()] + list(torch.autograd.grad(loss, list(xs) + list(op.parameters())))

    xs = [t.clone().requires_grad_(True) for t in ins]
    eager = step(op_e, xs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    warm = sf_op(z, tag).to(DEV).train()
    with torch.cuda.stream(side):
        step(warm, xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(op_g, xs)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        torch.testing.assert_close(b, a, rtol=0, atol=0)


@pytest.mark.parametrize("how", ["float64", "hooked_conv", "momentum_none"])
def test_fallbacks_take_torchs_path(how):
    z = load_golden("conve_sf_small")
    tag = "s1"
    op = sf_op(z, tag)
    dtype = torch.float64 if how == "float64" else torch.float32
    if how == "hooked_conv":
        op.conv2d.register_forward_hook(lambda *a: None)
    if how == "momentum_none":
        for bn in (op.bn0, op.bn1, op.bn2):
            bn.momentum = None
    _lib.meter.start(CONVE_FNS)
    op, ins, pred, loss = run_sf(op, z, tag, dtype=dtype)
    assert _lib.meter.stop() == {}
    check_sf(z, tag, op, ins, pred, loss, f"fallback/{how}", eval_too=how != "momentum_none", buffers=how != "momentum_none")
