"""Node-classification architecture search on HIP: the grouped candidate-Linear kernels (csrc/cand_linear.hip, ABI 22), the NC MixedOp
(cell_nc), the supernet against the reference (model_search_nc; fixtures of tests/golden/make_golden_nc_search.py) and the three search
passes with FusedAdam inside architect_nc.Architect and ClippedSGD(max_norm=0).

Which accuracy bound applies to the kernel.  mrg_cand_linear_fwd runs on the exact-f32 matrix core and walks k in its own order; the
kernel that K.linear dispatches to by default is the split-bf16 row GEMM.  The two do not sum in the same order, so the second of the
issue's two forms applies: the error against a float64 product is at most 1.5 x that of K.linear under mrg_gemm_set_mode(1) (the
exact-f32 row GEMM) plus 1e-6 of the output scale -- the bar of test_split_core_is_as_accurate_as_the_exact_f32_core.  The same holds
for the input gradient.  Column sums meet test_producer_stats_gpu.check_sums (the float64 reordering bound)."""
import pytest
import torch

from conftest import load_golden
from test_nc_cpu import close, fixture_blocks
from test_nc_search_cpu import CASES, check_step, make_net, run_search_passes, search_args
from test_producer_stats_gpu import check_sums

from mr_gnas_amd import _lib, architect_nc as AN, cell_nc as CN, functional as K, graph as G, operations_nc as ON
from mr_gnas_amd.functional import switches as SW

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- kernel ------------------------------------------------------------------------------------------------------------------
def members(rows, D, n, seed, share_x=True):
    gen = torch.Generator().manual_seed(seed)
    xs = [(torch.randn(rows, D, generator=gen) * 1.5 + 0.25).to(DEV) for _ in range(n)]
    if share_x and n >= 3:
        xs[1] = xs[0]                                        # two members read one tensor (f_identity next to another reader)
    Ws = [(torch.randn(D, D, generator=gen) / D ** 0.5).to(DEV) for _ in range(n)]
    bs = [(0.3 * torch.randn(D, generator=gen)).to(DEV) for _ in range(n)]
    gs = [torch.randn(rows, D, generator=gen).to(DEV) for _ in range(n)]
    return xs, Ws, bs, gs


def cand_fwd(xs, Ws, bs, sums):
    rows, D = xs[0].shape
    n = len(xs)
    ys = [torch.full((rows, D), float("nan"), device=DEV) for _ in range(n)]
    blocks = _lib.load().mrg_cand_linear_colsum_blocks(rows, D) if sums else 0
    buf = torch.full((n * blocks * 2 * D,), float("nan"), dtype=torch.float64, device=DEV).view(torch.uint8) if sums else None
    K.call("mrg_cand_linear_fwd", (n, K.ptr_array(xs), K.ptr_array(Ws), K.ptr_array(bs), K.ptr_array(ys), None, rows, D, K.stream_of(xs[0]),
                                   K.ptr(buf), blocks))
    cs = [_lib.ColSums(buf, k * blocks * 2 * D * 8, blocks, 2 * D, rows) for k in range(n)] if sums else None
    return ys, cs


def cand_bwd(gs, Ws):
    rows, D = gs[0].shape
    gxs = [torch.full((rows, D), float("nan"), device=DEV) for _ in gs]
    K.call("mrg_cand_linear_bwd_input", (len(gs), K.ptr_array(gs), K.ptr_array(Ws), K.ptr_array(gxs), None, rows, D, K.stream_of(gs[0])))
    return gxs


def exact_f32_linear(xs, Ws, bs, gs):
    """K.linear and its input gradient on the exact-f32 row GEMM (mrg_gemm_set_mode(1)): the accuracy yardstick."""
    lib = _lib.load()
    lib.mrg_gemm_set_mode(1)
    try:
        ys, gxs = [], []
        for x, W, b, g in zip(xs, Ws, bs, gs):
            x = x.detach().clone().requires_grad_(True)
            y = K.linear(x, W, b)
            (gx,) = torch.autograd.grad(y, x, g)
            ys.append(y.detach())
            gxs.append(gx)
        torch.cuda.synchronize()
    finally:
        lib.mrg_gemm_set_mode(0)
    return ys, gxs


@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("rows", [1, 57, 129, 4099, 40003])
def test_grouped_kernels_against_float64(rows, D):
    for n in (1, 3, 4):
        xs, Ws, bs, gs = members(rows, D, n, 1000 * n + rows + D)
        ys, cs = cand_fwd(xs, Ws, bs, True)
        ys_plain, _ = cand_fwd(xs, Ws, bs, False)
        ys_again, cs_again = cand_fwd(xs, Ws, bs, True)
        gxs, gxs_again = cand_bwd(gs, Ws), cand_bwd(gs, Ws)
        ref_y, ref_gx = exact_f32_linear(xs, Ws, bs, gs)
        for k in range(n):
            what = f"rows {rows} D {D} n {n} member {k}"
            assert torch.equal(ys[k], ys_plain[k]), what + ": the output depends on whether column sums are formed"
            assert torch.equal(ys[k], ys_again[k]) and torch.equal(gxs[k], gxs_again[k]), what + ": two runs differ"
            assert torch.equal(cs[k].buf, cs_again[k].buf), what + ": the column sums of two runs differ"
            y64 = xs[k].double() @ Ws[k].double().t() + bs[k].double()
            gx64 = gs[k].double() @ Ws[k].double()
            for got, yard, ref, name in ((ys[k], ref_y[k], y64, "Y"), (gxs[k], ref_gx[k], gx64, "gX")):
                err, err_yard = float((got.double() - ref).abs().max()), float((yard.double() - ref).abs().max())
                scale = float(ref.abs().max())
                print(f"{what} {name}: err {err:.3e}, exact-f32 row GEMM {err_yard:.3e}, scale {scale:.3e}")
                assert err <= 1.5 * err_yard + 1e-6 * scale, f"{what} {name}: err {err:.3e} against {err_yard:.3e} of the exact-f32 row GEMM"
            check_sums(cs[k], ys[k], what)


@pytest.mark.parametrize("D", [200, 6])
def test_other_widths_take_the_per_member_path(D):
    rows = 129
    xs, Ws, bs, _ = members(rows, D, 3, D)
    lins = []
    for W, b in zip(Ws, bs):
        lin = torch.nn.Linear(D, D).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
        lins.append(lin)
    assert _lib.load().mrg_cand_linear_colsum_blocks(rows, D) == 0
    _lib.meter.start(["mrg_cand_linear_fwd", "mrg_linear_fwd"])
    cands = K.candidate_linears(xs, lins, K.ForEpilogue(stats=True))
    rec = _lib.meter.stop()
    assert "mrg_cand_linear_fwd" not in rec and rec["mrg_linear_fwd"]["launches"] == 3
    for c, x, W, b in zip(cands, xs, Ws, bs):
        assert c.kind == "stored" and c.sums is None
        assert torch.equal(c.y, K.linear(x, W, b))


# ---- MixedOp -----------------------------------------------------------------------------------------------------------------
def mixed_block(E, seed):
    """A block of E edge rows over max(2, E // 5) destinations (one without in-edges)."""
    gen = torch.Generator().manual_seed(seed)
    n_dst = max(2, E // 5)
    dst = torch.randint(0, n_dst - 1, (E,), generator=gen) if E > 1 else torch.zeros(1, dtype=torch.long)
    src = torch.randint(0, n_dst + 7, (E,), generator=gen)
    return G.Block(torch.arange(n_dst + 7), torch.arange(n_dst), src, dst, torch.arange(E))


def mixed_op(ops, D, seed):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    mop = CN.MixedOp(D, ops)
    with torch.no_grad():
        for m in mop.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(D, generator=gen))
                m.bias.copy_(0.1 * torch.randn(D, generator=gen))
            elif isinstance(m, torch.nn.Linear) and m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
    return mop.to(DEV).train()


def mixed_step(mop, w, blk, h, h_in, g, names=None):
    h = h.detach().requires_grad_(True)
    w = w.detach().requires_grad_(True)
    for p in mop.parameters():
        p.grad = None
    if names is not None:
        _lib.meter.start(names)
    out = mop(w, blk, h, h_in)
    rec = _lib.meter.stop() if names is not None else None
    out.backward(g)
    return out.detach(), h.grad, w.grad, rec


def ulp_distance(a, b):
    """The largest distance between two float32 tensors in units in the last place (ordered-integer view of the bit patterns)."""
    def ordered(t):
        i = t.detach().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((ordered(a) - ordered(b)).abs().max())


STAGES = {"pre": ON.PRE_OPS, "first": ON.FIRST_OPS, "middle": ON.MIDDLE_OPS, "last": ON.LAST_OPS}


@pytest.mark.parametrize("E", [57, 4099])
@pytest.mark.parametrize("stage", list(STAGES))
def test_mixed_op_grouped_equals_per_member(stage, E, monkeypatch):
    """The NC MixedOp with its candidate Linears as one grouped launch against one K.linear per candidate.  The grouped kernel
    (exact-f32 core) and K.linear's default kernel (split-bf16 core) do not sum in the same order: there the outputs meet close().
    Against K.linear on the exact-f32 row GEMM (mrg_gemm_set_mode(1)), which sums in the grouped kernel's order, the candidates'
    Linear outputs are torch.equal and the running statistics agree within 1 ulp."""
    D, ops = 64, STAGES[stage]
    blk = mixed_block(E, E).to(DEV)
    gen = torch.Generator().manual_seed(E + len(ops))
    rows_in = blk.number_of_nodes() if stage == "last" else E
    rows_out = blk.number_of_nodes() if stage in ("middle", "last") else E
    h, h_in = torch.randn(rows_in, D, generator=gen).to(DEV), torch.randn(E, D, generator=gen).to(DEV)
    g = torch.randn(rows_out, D, generator=gen).to(DEV)
    w = torch.softmax(torch.randn(len(ops), generator=gen), 0).to(DEV)
    blk.plan()["n_chunks"]                                   # the plan's exact sizes on the host (before any capture)
    names = ["mrg_cand_linear_fwd", "mrg_cand_linear_bwd_input", "mrg_linear_fwd", "mrg_mix_stats_coef", "mrg_mix_fwd"]
    n_live = sum(o != "f_zero" for o in ops)
    state = {k: v.clone() for k, v in mixed_op(ops, D, 5).state_dict().items()}

    def fresh():
        mop = mixed_op(ops, D, 5)
        mop.load_state_dict(state)
        return mop

    monkeypatch.setattr(SW, "CAND_LINEAR_GROUP", False)
    mop_off = fresh()
    out_off, gh_off, gw_off, rec_off = mixed_step(mop_off, w, blk, h, h_in, g, names)
    monkeypatch.setattr(SW, "CAND_LINEAR_GROUP", True)
    mop_on = fresh()
    out_on, gh_on, gw_on, rec_on = mixed_step(mop_on, w, blk, h, h_in, g, names)
    # launch census: one grouped forward, the candidates' n_live row-GEMM launches gone (what is left belongs to the operators
    # themselves, e.g. a_max below its fusion threshold), and the statistics launch still runs (it forms the coefficients)
    assert "mrg_cand_linear_fwd" not in rec_off
    assert rec_on["mrg_cand_linear_fwd"]["launches"] == 1
    lin_on = rec_on.get("mrg_linear_fwd", {"launches": 0})["launches"]
    assert rec_off["mrg_linear_fwd"]["launches"] - lin_on == n_live
    if stage != "middle":
        assert lin_on == 0
    assert rec_on["mrg_mix_stats_coef"]["launches"] == 1 and rec_on["mrg_mix_fwd"]["launches"] == 1
    close(out_on, out_off, f"{stage} E {E} output")
    close(gh_on, gh_off, f"{stage} E {E} input gradient", rtol=2e-4, atol=5e-5)
    close(gw_on, gw_off, f"{stage} E {E} weight-vector gradient", rtol=2e-4, atol=5e-5)
    # The gradient of a candidate's Linear bias is exactly 0 (the training-mode BatchNorm behind it removes a constant): both paths
    # hold the rounding noise of a float32 sum over the rows there.  The comparison point's largest such value is its own error;
    # twice that (two noises differ by up to their sum) joins the absolute bound for these tensors.
    cand_bias = [f"_ops.{k}.1.bias" for k in range(len(ops))]
    noise = 2.0 * max(float(q.grad.abs().max()) for n, q in mop_off.named_parameters() if n in cand_bias)
    for (n, p), (_, q) in zip(mop_on.named_parameters(), mop_off.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            torch.testing.assert_close(p.grad, q.grad, rtol=2e-3, atol=5e-6 + (noise if n in cand_bias else 0.0),
                                       msg=lambda m: f"{stage} E {E} {n} grad: {m}")
    # two eager runs are bit-identical, and a captured forward + backward replays to the same bits
    out2, gh2, gw2, _ = mixed_step(mop_on, w, blk, h, h_in, g)
    assert torch.equal(out2, out_on) and torch.equal(gh2, gh_on) and torch.equal(gw2, gw_on)
    eager_grads = [p.grad.clone() for p in mop_on.parameters() if p.grad is not None]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mixed_step(mop_on, w, blk, h, h_in, g)               # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    hh, ww = h.detach().requires_grad_(True), w.detach().requires_grad_(True)
    params = [p for p in mop_on.parameters() if p.grad is not None]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_c = mop_on(ww, blk, hh, h_in)
        grads_c = torch.autograd.grad(out_c, [hh, ww] + params, g)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c, out_on) and torch.equal(grads_c[0], gh_on) and torch.equal(grads_c[1], gw_on)
    for a, b in zip(grads_c[2:], eager_grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize("E", [57, 4099])
@pytest.mark.parametrize("stage", list(STAGES))
def test_mixed_op_statistics_within_one_ulp_in_the_same_summation_order(stage, E, monkeypatch):
    """Grouped against per candidate under mrg_gemm_set_mode(1): Linear outputs torch.equal, running statistics within 1 ulp."""
    D, ops = 64, STAGES[stage]
    blk = mixed_block(E, E).to(DEV)
    gen = torch.Generator().manual_seed(E + len(ops))
    rows_in = blk.number_of_nodes() if stage == "last" else E
    rows_out = blk.number_of_nodes() if stage in ("middle", "last") else E
    h, h_in = torch.randn(rows_in, D, generator=gen).to(DEV), torch.randn(E, D, generator=gen).to(DEV)
    g = torch.randn(rows_out, D, generator=gen).to(DEV)
    w = torch.softmax(torch.randn(len(ops), generator=gen), 0).to(DEV)
    state = {k: v.clone() for k, v in mixed_op(ops, D, 5).state_dict().items()}

    def fresh():
        mop = mixed_op(ops, D, 5)
        mop.load_state_dict(state)
        return mop

    mop_on = fresh()
    # Running statistics: within 1 ulp where the two paths sum in the same order.  Under mrg_gemm_set_mode(1) K.linear runs on the
    # exact-f32 row GEMM, whose order of k the grouped kernel shares: the candidates' Linear outputs are then the same bits, and what
    # is left between the legs is where the BatchNorm sums come from -- the grouped launch's float64 partials against the statistics
    # sweep, two float64 orders of the same float32 values, rounded to float32 once.  A dropped row or strip, or a wrong row count
    # handed to the statistics launch, moves them by thousands of ulp.
    lib = _lib.load()
    lib.mrg_gemm_set_mode(1)
    try:
        xs = [None if name == "f_zero" else op[0](blk, h, h_in) for name, op in zip(ops, mop_on._ops)]
        lins = [op[1] for op in mop_on._ops]
        monkeypatch.setattr(SW, "CAND_LINEAR_GROUP", False)
        ys_off = [c.y.detach() for c in K.candidate_linears(xs, lins, K.ForEpilogue(stats=True))]
        mop_off1 = fresh()
        out_off1 = mixed_step(mop_off1, w, blk, h, h_in, g)[0]
        monkeypatch.setattr(SW, "CAND_LINEAR_GROUP", True)
        cands = K.candidate_linears(xs, lins, K.ForEpilogue(stats=True))
        mop_on1 = fresh()
        out_on1 = mixed_step(mop_on1, w, blk, h, h_in, g)[0]
        torch.cuda.synchronize()
    finally:
        lib.mrg_gemm_set_mode(0)
    for k, (c, y) in enumerate(zip(cands, ys_off)):
        assert torch.equal(c.y, y), f"{stage} E {E} candidate {k}: grouped and exact-f32 per-member Linear outputs differ"
        if ops[k] != "f_zero":
            check_sums(c.sums, c.y.detach(), f"{stage} E {E} candidate {k}")
    worst = 0
    for (n, a), (_, b) in zip(mop_on1.named_buffers(), mop_off1.named_buffers()):
        if "running_" in n:
            d = ulp_distance(a, b)
            worst = max(worst, d)
            assert d <= 1, f"{stage} E {E} {n}: {d} ulp between the grouped and the per-member path"
    print(f"{stage} E {E}: running statistics within {worst} ulp, outputs within {ulp_distance(out_on1, out_off1)} ulp (same summation order)")
    close(out_on1, out_off1, f"{stage} E {E} output, same summation order")


def test_mixed_op_on_one_row_raises_in_training():
    mop = mixed_op(ON.LAST_OPS, 64, 3)
    blk = mixed_block(1, 1).to(DEV)
    w = torch.full((4,), 0.25, device=DEV)
    x = torch.randn(1, 64, device=DEV)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        mop(w, blk, x, x)
    mop.eval()
    assert mop(w, blk, x, x).shape == (1, 64)


def test_f_zero_branch_on_hip():
    """running_var -> 0.9, a zero (not None) weight gradient, and w_k * ReLU(beta_k) on every row."""
    D, k = 64, ON.FIRST_OPS.index("f_zero")
    mop = mixed_op(ON.FIRST_OPS, D, 11)
    blk = mixed_block(131, 2).to(DEV)
    x = torch.randn(131, D, device=DEV)
    w = torch.zeros(4, device=DEV)
    w[k] = 0.7
    out = mop(w, blk, x, x)
    out.sum().backward()
    lin, bn = mop._ops[k][1], mop._ops[k][2]
    # (b - mean(b)) / sqrt(eps): see test_nc_search_cpu.test_f_zero_branch_has_the_reference_semantics for the 1.5e-4
    torch.testing.assert_close(out, (0.7 * torch.relu(bn.bias.detach())).expand_as(out), rtol=1e-5, atol=1.5e-4)
    torch.testing.assert_close(bn.running_var, torch.full_like(bn.running_var, 0.9), rtol=0, atol=1e-6)
    torch.testing.assert_close(bn.running_mean, 0.1 * lin.bias.detach(), rtol=1e-5, atol=1e-7)
    assert lin.weight.grad is not None and not lin.weight.grad.any()
    assert bn.bias.grad is not None and float(bn.bias.grad.abs().max()) > 0


# ---- network -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["s16", "s64"])
def test_network_matches_the_reference(tag, monkeypatch):
    z = load_golden(CASES[tag])
    layers = int(z[tag + "/args"][8])
    net = make_net(z, tag, DEV)
    assert all(a.is_cuda for a in net.arch_parameters())
    check_step(z, tag, net, DEV, logits_tol=dict(rtol=2e-4, atol=5e-5))
    # launch census of one training forward: one grouped launch per MixedOp, 66 per-candidate row-GEMM launches per layer gone
    nodes = int(z[tag + "/args"][9])
    n_mixed = 1 + sum(1 + i for i in range(nodes)) + nodes + sum(nodes + i for i in range(nodes))
    n_live = 3 + 3 * sum(1 + i for i in range(nodes)) + 3 * nodes + 3 * sum(nodes + i for i in range(nodes))
    if nodes == 3:
        assert (n_mixed, n_live) == (22, 66)
    blocks = [b.to(DEV) for b in fixture_blocks(z, tag + "/blocks/")]
    trip = z[tag + "/trip_index"].to(DEV)
    net.train()
    count = {}
    for on in (True, False):
        monkeypatch.setattr(SW, "CAND_LINEAR_GROUP", on)
        _lib.meter.start(["mrg_cand_linear_fwd", "mrg_linear_fwd"])
        with torch.no_grad():
            net(trip, blocks)
        count[on] = _lib.meter.stop()
    assert count[True]["mrg_cand_linear_fwd"]["launches"] == n_mixed * layers and "mrg_cand_linear_fwd" not in count[False]
    assert count[False]["mrg_linear_fwd"]["launches"] - count[True]["mrg_linear_fwd"]["launches"] == n_live * layers


# ---- search ------------------------------------------------------------------------------------------------------------------
def test_search_passes_on_hip_match_the_reference(monkeypatch):
    from mr_gnas_amd.optim import ClippedSGD, FusedAdam
    z16, z = load_golden(CASES["s16"]), load_golden("nc_search_small")
    net = make_net(z16, "s16", DEV).train()
    optimizer = ClippedSGD(net.parameters(), float(z["lr"]), momentum=float(z["momentum"]), weight_decay=float(z["weight_decay"]), max_norm=0)
    architect = AN.Architect(DEV, net, search_args(z))
    assert isinstance(architect.optimizer, FusedAdam)
    assert architect.loss.is_cuda and torch.equal(architect.loss.cpu(), torch.ones(1))      # what a warm-up step returns: on the device too
    run_search_passes(z16, z, net, architect, optimizer, DEV, monkeypatch)
