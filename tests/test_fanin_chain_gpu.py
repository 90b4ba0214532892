"""The gradient fan-in chain (functional/fanin.py, switches.FANIN_CHAIN): readers of a state add the running sum of the other
readers' gradients in the store of their own last kernel instead of returning a [rows, D] tensor each for a K-way pass.

Kernel level: every new kernel mode (the second addend of the input-gradient GEMMs, the chain mode of a_max's input-gradient
kernel, the accumulate mode of the row-factor gate's backward) against the composition it replaces -- the plain launch followed by
mrg_sum_buffers / mrg_sum_rows_gather over {running sum, plain output} -- elementwise with ``==`` (the same float32 additions in the
same association; only the sign of a zero may differ, which ``==`` does not see), out of place and in place.
Cell level: cell_lp.Cell with the chain on against the chain off.  Fallbacks: the cases in which the chain must step aside."""
import numpy as np
import pytest
import torch

import mr_gnas_amd  # noqa: F401
from mr_gnas_amd import _lib, cell_lp as CL, functional as K, graph as G
from mr_gnas_amd._lib import call, ptr, ptr_array, stream_of
from mr_gnas_amd.functional._base import _ws, gate_ld

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _sum2(a, b):
    """mrg_sum_buffers over {a, b}: (0 + a) + b."""
    return K.sum_buffers([a, b])


# ---- the second addend of the input-gradient GEMMs -----------------------------------------------------------------------------------
# Rows: 1, 127 / 129 (either side of the 128-row workgroup), 16 385 (the first count past the few-row bound, x3_parts.hpp: the
# wave-autonomous kernel below it, the LDS-weight kernels above).  (K = N = 200: rowgemm_x3s_k; reduction 400, N = 200: the pair on
# rowgemm_x3q_k; D = 64: two-tile blocks.)
def _segments(M, empty_middle):
    if empty_middle:
        return M // 2, M // 2
    return M // 3, (2 * M) // 3


@pytest.mark.parametrize("M", [1, 127, 129, 16385])
@pytest.mark.parametrize("D,pair", [(200, False), (200, True), (64, False), (64, True)])
def test_second_addend_of_the_grouped_input_gradient(M, D, pair):
    gen = torch.Generator().manual_seed(M * 7 + D + pair)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    name = "mrg_linear_bwd_input3_pair" if pair else "mrg_linear_bwd_input3"
    ws_bytes = int(getattr(_lib.load(), name + "_workspace_bytes")(D, D))
    assert ws_bytes > 0
    for empty_middle in ((False, True) if M == 129 else (False,)):
        b0, b1 = _segments(M, empty_middle)
        dz1, dz2, direct, total = rnd(M, D), rnd(M, D), rnd(M, D), rnd(M, D)
        W1, W2 = [rnd(D, 2 * D) * 0.1 for _ in range(3)], [rnd(D, 2 * D) * 0.1 for _ in range(3)]
        head = (ptr(dz1), ptr(dz2), ptr_array(W1), ptr_array(W2)) if pair else (ptr(dz1), ptr_array(W1))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

        def run(gX, accumulate, tot=None):
            tail = (ptr(ws), b0, b1, M, D, D, 2 * D, accumulate, stream_of(gX))
            if tot is None:
                call(name, (*head, ptr(gX), *tail))
            else:
                call(name, (*head, ptr(gX), *tail, ptr(tot)), symbol=name + "_acc2")
            return gX
        # with a direct term (accumulate): (product + direct) + total -- the epilogue kind of its own
        ref = _sum2(run(direct.clone(), 1), total)
        got = run(direct.clone(), 1, total)
        assert bool((got == ref).all()), (M, D, pair, empty_middle, "accumulate", float((got - ref).abs().max()))
        # without: product + total, out of place and in place
        ref = _sum2(run(torch.empty(M, D, device=DEV), 0), total)
        got = run(torch.full((M, D), 7.0, device=DEV), 0, total)
        assert bool((got == ref).all()), (M, D, pair, empty_middle, "plain", float((got - ref).abs().max()))
        inplace = total.clone()
        got = run(inplace, 0, inplace)
        assert bool((got == ref).all()), (M, D, pair, empty_middle, "in place", float((got - ref).abs().max()))
        # the direct term and the running sum in one buffer is refused, not computed wrongly
        with pytest.raises(_lib.MrgnasError):
            buf = direct.clone()
            run(buf, 1, buf)


@pytest.mark.parametrize("rows", [1, 129, 16385])
@pytest.mark.parametrize("D", [200, 64, 48])
@pytest.mark.parametrize("mode", [0, 1])
def test_second_addend_of_the_plain_input_gradient(rows, D, mode):
    """mrg_linear_bwd_input_acc2 on both matrix cores: D = 48 is a reduction length the split core refuses, mode 1 switches the split
    core off -- both fall back to the exact-f32 core, they do not fail."""
    gen = torch.Generator().manual_seed(rows + D + mode)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    gY, W, direct, total = rnd(rows, D), rnd(D, 2 * D) * 0.1, rnd(rows, D), rnd(rows, D)
    ws = torch.empty(int(_lib.load().mrg_linear_bwd_input_workspace_bytes(D, D)), dtype=torch.uint8, device=DEV)

    def run(gX, accumulate, tot=None):
        args = (ptr(gY), ptr(W[:, D:]), ptr(gX), ptr(ws), rows, D, D, 2 * D, accumulate, stream_of(gX))
        if tot is None:
            call("mrg_linear_bwd_input", args)
        else:
            call("mrg_linear_bwd_input", args + (ptr(tot),), symbol="mrg_linear_bwd_input_acc2")
        return gX
    _lib.check(_lib.load().mrg_gemm_set_mode(mode))
    try:
        ref = _sum2(run(direct.clone(), 1), total)
        got = run(direct.clone(), 1, total)
        assert bool((got == ref).all()), float((got - ref).abs().max())
        ref = _sum2(run(torch.empty(rows, D, device=DEV), 0), total)
        inplace = total.clone()
        got = run(inplace, 0, inplace)
        assert bool((got == ref).all()), float((got - ref).abs().max())
    finally:
        _lib.check(_lib.load().mrg_gemm_set_mode(0))


# ---- a_max's input-gradient kernel as the member that closes a chain -------------------------------------------------------------------
def _amax_case(kind, D, gen):
    N = 37
    if kind == "random":                # E about 1000; node 5 has no in-edge
        dst = torch.randint(0, N - 1, (1000,), generator=gen)
        dst[dst >= 5] += 1
    elif kind == "hub":                 # node 3 holds more than half the edges
        dst = torch.randint(0, N, (1000,), generator=gen)
        dst[:600] = 3
        dst = dst[torch.randperm(1000, generator=gen)]
    else:                               # one edge
        dst = torch.tensor([11])
    return N, int(dst.numel()), dst


@pytest.mark.parametrize("kind", ["random", "hub", "one_edge"])
@pytest.mark.parametrize("with_total", [False, True])
@pytest.mark.parametrize("with_gather", [False, True])
def test_segmax_bwd_input_chain(kind, with_total, with_gather):
    D = 200
    gen = torch.Generator().manual_seed(len(kind) + 2 * with_total + with_gather)
    N, E, dst = _amax_case(kind, D, gen)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    dst_d = dst.to(DEV).int()
    gout, mx, W = rnd(N, D), rnd(N, D), rnd(D, D) * 0.1
    # arg: for every (node, column) one of the node's in-edges (-1 without one), as the forward leaves it
    arg = torch.full((N, D), -1, dtype=torch.int32)
    for v in range(N):
        es = (dst == v).nonzero().flatten()
        if es.numel():
            arg[v] = es[torch.randint(0, es.numel(), (D,), generator=gen)].int()
    arg = arg.to(DEV)
    total = rnd(E + N, D) if with_total else None
    gh, gself = (rnd(N, D), rnd(N, D)) if with_gather else (None, None)
    head = (ptr(gout), ptr(mx), ptr(dst_d), ptr(arg), ptr(W))
    # what it replaces: the plain launch (+ the self rows, a copy of gout) and the fan-in pass over {total, that}
    plain = torch.empty(E + N, D, device=DEV)
    gy0 = torch.empty(E, D, device=DEV)
    call("mrg_segmax_bwd_input", (*head, ptr(gy0), ptr(plain), None, E, N, D, D, stream_of(plain)))
    plain[E:] = gout
    xs = ([total] if with_total else []) + [plain]
    if with_gather:
        ref = torch.empty(E + N, D, device=DEV)
        call("mrg_sum_rows_gather", (ptr_array(xs), len(xs), ptr(gh), ptr(gself), ptr(dst_d), E, E + N, D, ptr(ref), stream_of(ref)))
    else:
        ref = K.sum_buffers(xs) if with_total else plain
    for in_place in ((False, True) if with_total else (False,)):
        gx = total.clone() if in_place else torch.full((E + N, D), 7.0, device=DEV)
        tot = gx if in_place else total
        gy = torch.empty(E, D, device=DEV)
        call("mrg_segmax_bwd_input", (*head, ptr(gy), ptr(gx), None, E, N, D, D, stream_of(gx), ptr(tot), ptr(gh), ptr(gself)),
             symbol="mrg_segmax_bwd_input_chain")
        assert bool((gy == gy0).all())
        assert bool((gx == ref).all()), (kind, with_total, with_gather, in_place, float((gx - ref).abs().max()))
    # the self rows without the edge gather's partner (a_sum with add_self False): gself absent, gh present
    if with_gather:
        gx = torch.empty(E + N, D, device=DEV)
        call("mrg_segmax_bwd_input", (*head, None, ptr(gx), None, E, N, D, D, stream_of(gx), ptr(total), ptr(gh), None),
             symbol="mrg_segmax_bwd_input_chain")
        ref2 = torch.empty(E + N, D, device=DEV)
        call("mrg_sum_rows_gather", (ptr_array(xs), len(xs), ptr(gh), None, ptr(dst_d), E, E + N, D, ptr(ref2), stream_of(ref2)))
        assert bool((gx == ref2).all())


# ---- the row-factor gate's backward onto the running sum ------------------------------------------------------------------------------
@pytest.mark.parametrize("M,b0,b1", [(1000, 300, 700), (1000, 400, 400), (129, 0, 100), (5, 1, 3)])
@pytest.mark.parametrize("D", [200, 64])
def test_gate_row_bwd_accumulate(M, b0, b1, D):
    gen = torch.Generator().manual_seed(M + b0 + D)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    q, hvec, s, s_in, total = rnd(M), rnd(M), rnd(M, D), rnd(M, D), rnd(M, D)
    uvc = rnd(3, gate_ld(D))
    ws = _ws(int(_lib.load().mrg_gate_bwd_workspace_bytes(M, D)), s)

    def run(gs_in, tot=None):
        d_uvc = torch.empty(3, gate_ld(D), device=DEV)
        args = (ptr(q), ptr(hvec), ptr(s), ptr(s_in), ptr(uvc), ptr(gs_in), ptr(d_uvc), ptr(ws), b0, b1, M, D, stream_of(s))
        if tot is None:
            call("mrg_gate_row_bwd", args)
        else:
            call("mrg_gate_row_bwd", args + (ptr(tot),), symbol="mrg_gate_row_bwd_acc")
        return gs_in, d_uvc
    plain, d0 = run(torch.empty(M, D, device=DEV))
    ref = _sum2(total, plain)
    got, d1 = run(torch.full((M, D), 7.0, device=DEV), total)
    assert bool((got == ref).all()) and bool((d1 == d0).all())
    inplace = total.clone()
    got, d2 = run(inplace, inplace)
    assert bool((got == ref).all()) and bool((d2 == d0).all())


# ---- cell level ------------------------------------------------------------------------------------------------------------------
def _graph(N, E, seed):
    gen = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    return G.RelGraph(N, src.numpy(), dst.numpy(), torch.randint(0, 4, (E,), generator=gen).numpy(),
                      (torch.rand(E, generator=gen) + 0.1).numpy().astype(np.float32), device=DEV)


_CELLS = {}


def _cell_case(D):
    """One cell, graph and set of inputs per width, shared by the tests below (never modified: gradients are cleared per run)."""
    if D not in _CELLS:
        N, E = 50, 400
        g = _graph(N, E, 3 + D)
        torch.manual_seed(D)
        cell = CL.Cell(1, 2, 2, D, 0.1).to(DEV)
        cell.train()
        gen = torch.Generator().manual_seed(5 + D)
        x0, hr0 = torch.randn(E + N, D, generator=gen), torch.randn(E + N, D, generator=gen)
        W = [torch.softmax(torch.randn(r, c, generator=gen), 1).to(DEV).requires_grad_(True)
             for r, c in ((1, len(CL.PRE_OPS)), (3, len(CL.FIRST_OPS)), (2, len(CL.MIDDLE_OPS)), (5, len(CL.LAST_OPS)))]
        gout = torch.randn(N, D, generator=gen).to(DEV)
        _CELLS[D] = (g, cell, x0, hr0, W, gout)
    return _CELLS[D]


def _cell_grads(D, chain, monkeypatch, backward=None, extra=None, count=None):
    """{name: gradient} of one forward + backward of the shared cell with switches.FANIN_CHAIN = chain (dropout masks fixed by the
    seed).  backward(out, gout): another way to run the backward; extra(x): one more term of the loss that reads the input."""
    g, cell, x0, hr0, W, gout = _cell_case(D)
    monkeypatch.setattr(K.switches, "FANIN_CHAIN", chain)
    x, hr = x0.clone().to(DEV).requires_grad_(True), hr0.clone().to(DEV).requires_grad_(True)
    for p in list(cell.parameters()) + W:
        p.grad = None
    for m in cell.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.reset_running_stats()
    torch.manual_seed(11)
    if count is not None:
        # the fan-in launches over the cell's full-size [E + N, D] states (the node-row states of the last stage keep their sums:
        # f_sparse_last is no member of the chain), and -- "all" -- what _lib.meter sees of both entry points
        real, M = K.fanin.call, x.shape[0]

        def spy(name, args, **kw):
            rows = {"mrg_sum_buffers": lambda: args[3] // D, "mrg_sum_rows_gather": lambda: args[6]}.get(name, lambda: None)()
            if rows == M:
                count[name] = count.get(name, 0) + 1
            return real(name, args, **kw)
        monkeypatch.setattr(K.fanin, "call", spy)
        _lib.meter.start(["mrg_sum_buffers", "mrg_sum_rows_gather"])
    out = cell(g, x, hr, *W)
    if backward is not None:
        backward(out, gout)
    else:
        loss = (out * gout).sum()
        if extra is not None:
            loss = loss + extra(x)
        loss.backward()
    if count is not None:
        count["all"] = {k: v["launches"] for k, v in _lib.meter.stop().items()}
        monkeypatch.setattr(K.fanin, "call", real)
    torch.cuda.synchronize()
    res = {"x": x.grad, "hr": hr.grad}
    res.update({f"w{i}": w.grad.clone() for i, w in enumerate(W)})
    res.update({n: p.grad.clone() for n, p in cell.named_parameters() if p.grad is not None})
    return res


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("D", [64, 200])
@pytest.mark.parametrize("fused_aggregators", [True, False])
def test_cell_gradients_with_and_without_the_chain(D, fused_aggregators, monkeypatch):
    """Every input and parameter gradient of cell_lp.Cell(1, 2, 2, D, 0.1) with the chain on against the chain off.

    The chain may change nothing but the association of the float32 sums of the fan-ins; two summation orders of the same n terms
    differ by at most 2 (n - 1) 2^-24 sum|terms| per element (each is within (n - 1) 2^-24 sum|terms| of the exact sum).  For this
    cell it changes not even that.  Readers run in the reverse order of their forward, which is the order of their alias numbers,
    so a chain of the readers that ran first, followed by what arrives through autograd, is the unchained sum term for term:
      state 2 {a_sum's gather, a_mean, a_max}, n = 3;  state 1 {gather, a_mean, a_max, the dense pair}, n = 4;
      state 0's second batch of aliases {row-factor gate, dense pair}, n = 2;
      state 0's first batch {dense pair, dense pair, the second batch's sum}, n = 3: the two pairs are chained, the second batch's
      sum arrives through autograd and is added last by a two-way pass, as the three-way pass added it.
    So every gradient must be EQUAL element for element (== : a zero may change its sign, the K-way pass starts from 0 + a); the
    bound 2 (n - 1) 2^-24 n C max|b| with n = 4, C = 32 (allowance for cancellation inside a fan-in and for the linear maps behind
    it) is what a re-associated sum would have to meet, and is asserted first so that a failure shows its size.
    fused_aggregators: the forms the full-size step takes -- a_max's gradient comes from mrg_segmax_bwd_input, which adds the
    running sum and a_sum's gather itself: states 1 and 2 need no pass.  Not fused (below switches.FUSED_AMAX_MIN_ROWS): a_max's
    gradient is a row GEMM, which cannot add the gather; with the gather waiting, a_max and the dense pair leave the chain and the
    gathered pass adds them in its own order."""
    if fused_aggregators:
        monkeypatch.setattr(K.switches, "FUSED_AMAX_MIN_ROWS", 0)
    n = 4
    bound = 2 * (n - 1) * U * n * 32
    count, count_off = {}, {}
    off = _cell_grads(D, False, monkeypatch, count=count_off)
    on = _cell_grads(D, True, monkeypatch, count=count)
    assert set(on) == set(off)
    worst = {k: _rel(on[k], off[k]) for k in off}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print(f"D={D} fused={fused_aggregators}: largest relative differences {top}, bound {bound:.3e}; full-size fan-in launches without "
          f"the chain {count_off}, with it {count}")
    for k, r in worst.items():
        assert r <= bound, (k, r, bound)
    for k in off:
        assert bool((on[k] == off[k]).all()), (k, worst[k])
    # Full-size fan-in launches (mrg_sum_buffers, mrg_sum_rows_gather).  Without the chain: the two batches of state 0's aliases
    # and the cell's two inputs x and hr (read by cell zero's three compose operators, which are no members of the chain); the
    # gathered sums of states 1 and 2.  With it: state 0's second batch needs none, its first batch a two-way pass instead of a
    # three-way one, and -- fused -- states 1 and 2 none.
    assert (count_off.get("mrg_sum_buffers", 0), count_off.get("mrg_sum_rows_gather", 0)) == (4, 2), count_off
    assert (count.get("mrg_sum_buffers", 0), count.get("mrg_sum_rows_gather", 0)) == ((3, 0) if fused_aggregators else (3, 2)), count
    assert count["all"].get("mrg_sum_rows_gather", 0) == (0 if fused_aggregators else 2), count


# ---- fallbacks: the gradients of the off path, no exception ------------------------------------------------------------------------------
def _same(on, off, bound=2 * 2 * U * 3 * 32):
    assert set(on) == set(off)
    for k in off:
        assert _rel(on[k], off[k]) <= bound, (k, _rel(on[k], off[k]))


def test_fallback_plain_torch_reader(monkeypatch):
    """A plain torch op reads an alias next to the chained readers: its gradient arrives through autograd and is added to the
    running sum by the K-way pass."""
    gen = torch.Generator().manual_seed(2)
    M, D, b0, b1 = 300, 64, 100, 200
    rnd = lambda *sh: torch.randn(*sh, generator=gen).to(DEV)
    Ws = [[rnd(D, D) * 0.1 for _ in range(3)] for _ in range(2)]
    norm = (torch.rand(b1, generator=gen) + 0.1).to(DEV)
    x0, gout = torch.randn(M, D, generator=gen), rnd(M, D)
    f_comp = lambda a, W: K.dense_filter_comp(1, a, None, norm, b0, b1, W[0], None, W[1], None, W[2], None, 1.0)
    res = {}
    for chain in (False, True):
        monkeypatch.setattr(K.switches, "FANIN_CHAIN", chain)
        x = x0.clone().to(DEV).requires_grad_(True)
        fan = K.Fan(x, 4)
        y = f_comp(fan.take(), Ws[0]) + f_comp(fan.take(), Ws[1]) + torch.sin(fan.take())
        unread = fan.take()                         # an alias nobody reads
        (y * gout).sum().backward()
        del unread
        res[chain] = x.grad.clone()
    assert _rel(res[True], res[False]) <= 2 * 2 * U * 3 * 32


def test_fallback_side_streams(monkeypatch):
    """Candidates forced onto side streams: a deposit is taken on another stream than it was written on."""
    monkeypatch.setattr(K.switches, "FORK_MIN_ROWS", 0)
    monkeypatch.setattr(CL, "MIXED_STREAMS", 2)
    off = _cell_grads(64, False, monkeypatch)
    for _ in range(2):
        junk = [torch.full((m,), 7.0, device=DEV) for m in (1000, 5000, 20000, 100000) for _ in range(4)]      # stir the allocator's pools
        del junk
        _same(_cell_grads(64, True, monkeypatch), off)


def test_fallback_second_backward_over_a_retained_graph(monkeypatch):
    def twice(out, gout):
        out.backward(gout, retain_graph=True)
        out.backward(gout)
    off = _cell_grads(64, False, monkeypatch, backward=twice)
    on = _cell_grads(64, True, monkeypatch, backward=twice)
    _same(on, off)
    once = _cell_grads(64, False, monkeypatch)
    assert _rel(on["x"], 2 * once["x"]) <= 2 * 2 * U * 3 * 32 + 2 * U    # both passes counted, none twice


def test_fallback_double_backward(monkeypatch):
    """create_graph: the gradients stay on the tape, nothing is deposited."""
    def with_graph(out, gout):
        out.backward(gout, create_graph=True)
    off = _cell_grads(64, False, monkeypatch, backward=with_graph)
    on = _cell_grads(64, True, monkeypatch, backward=with_graph)
    _same({k: v.detach() for k, v in on.items()}, {k: v.detach() for k, v in off.items()})


def test_fallback_no_grad_forward(monkeypatch):
    g, cell, x0, hr0, W, _ = _cell_case(64)
    outs = []
    for chain in (False, True):
        monkeypatch.setattr(K.switches, "FANIN_CHAIN", chain)
        torch.manual_seed(11)
        with torch.no_grad():
            outs.append(cell(g, x0.to(DEV), hr0.to(DEV), *W))
    assert bool((outs[0] == outs[1]).all())
