"""BatchNorm sums of a first-stage MixedOp formed by the kernels that PRODUCE its candidates (the row GEMM's gate / scale epilogues:
mrg_dense_filter_fwd3_colsum; the row-factor gate: mrg_gate_row_fwd_colsum) and consumed by mrg_mix_stats_coef through
mrg_gated_branch.given, instead of a statistics pass over the stored [rows, D] tensors (functional.switches.PRODUCER_STATS).

Bounds.  The producers add the same float32 values as the pass, each converted to float64, in another order.  Any two float64
summation orders of n terms x_i differ by at most n * 2^-52 * sum |x_i| (each partial sum is off by at most 2^-53 of its
magnitude, which sum |x_i| bounds; two orders, n - 1 additions each) -- a dropped row of typical size is four orders of magnitude
above that.  Coefficients and running statistics are float32 roundings of float64 expressions of those sums: 1 ulp at most."""
import types

import numpy as np
import pytest
import torch

import mr_gnas_amd
from mr_gnas_amd import functional as K, graph as G, operations_lp as O
from test_ops_gpu import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATS = K.ForEpilogue(stats=True)


def total(cs, D):
    """[2, D] float64: a ColSums' partials added up (torch's order: any float64 order is within the bound)."""
    flat = cs.buf.view(torch.float64)[cs.offset // 8:]
    return flat.as_strided((cs.n, 2 * D), (cs.stride, 1)).sum(0).view(2, D)


def check_sums(cs, y, what):
    """cs against the float64 sums of the float32 values y [rows, D]."""
    rows, D = y.shape
    assert cs is not None, f"{what}: the producer left no sums"
    assert cs.rows == rows and cs.n >= 1 and cs.stride >= 2 * D
    got = total(cs, D)
    yd = y.double()
    ref = torch.stack([yd.sum(0), yd.square().sum(0)])
    bound = rows * 2.0 ** -52 * torch.stack([yd.abs().sum(0), yd.square().sum(0)])
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: rows {rows} D {D} partials {cs.n}: worst error / bound {worst:.3e}")
    assert bool((err <= bound).all()), f"{what}: column sums off by {worst:.3e} of the bound"
    # the partial buffer of the headline shape must stay below 8 % of one [rows, D] tensor (128- / 64-row workgroups: 3.1 / 6.3 %)
    return cs.n * 2 * D * 8 / (rows * D * 4)


def params(D, tied_in, gen):
    in_dim = 2 * D
    W = lambda: (torch.randn(D, in_dim, generator=gen) / in_dim ** 0.5).to(DEV)
    b = lambda: (0.1 * torch.randn(D, generator=gen)).to(DEV)
    dense = (W(), b(), W(), b(), W(), b())
    comp = (W(), W(), W())
    gate = []
    for _ in range(3):
        gate += [W(), b(), (torch.randn(1, D, generator=gen) / D ** 0.5).to(DEV)]
    return dense, comp, gate


# x3s (tied: K = D <= 224) and x3q (untied: K = 2 D > 224) shapes; rows that are no multiple of 128 / 64; a width with a partial column
# tile besides 200 (168 = 5 tiles + 8 columns); an empty `in` and an empty `out` direction segment; few rows (<= 16 384: the tied
# product runs on the few-row kernel, which has no sums -- the candidate must come without them and the epilogue fall back)
CASES = [(40003, 17003, 33001, 200), (30011, 0, 21000, 200), (30011, 12000, 12000, 200), (25001, 9000, 20000, 168), (9001, 3000, 6000, 200),
         (130, 50, 100, 200)]


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("M,b0,b1,D", CASES)
def test_producer_sums_against_float64_sums(M, b0, b1, D, tied):
    gen = torch.Generator().manual_seed(M + b0 + D + int(tied))
    s = torch.randn(M, D, generator=gen).to(DEV)
    s_in = s if tied else torch.randn(M, D, generator=gen).to(DEV)
    norm = (torch.rand(b1, generator=gen) + 0.1).to(DEV)
    dense, comp, gate = params(D, tied, gen)
    few = tied and M <= 16384                                 # rowgemm_x3_k (two-tile column blocks): the query answers 0
    lib = mr_gnas_amd._lib.load()
    K_ = D if tied else 2 * D
    for kind in (0, 1):
        blocks = int(lib.mrg_dense_filter3_colsum_blocks(kind, b0, b1, M, D, K_))
        assert (blocks == 0) == few, "which launches have a column-sum form"
    with torch.no_grad():
        stored = K.dense_filter_pair(s, s_in, norm, b0, b1, dense, comp, gate_only=False, for_epilogue=STATS)
        gated = K.dense_filter_pair(s, s_in, norm, b0, b1, dense, comp, gate_only=True, for_epilogue=STATS)
        plain = K.dense_filter_pair(s, s_in, norm, b0, b1, dense, comp, gate_only=False, for_epilogue=True)
        row = K.gate_comp_row_factor(s, s_in, norm, b0, b1, *gate, for_epilogue=STATS)
        row_plain = K.gate_comp_row_factor(s, s_in, norm, b0, b1, *gate)
    torch.cuda.synchronize()
    y_d, y_c = stored[0].y, stored[1].y
    # the sums change nothing else: outputs and the gate are those of the plain launches, bit for bit
    assert torch.equal(y_d, plain[0].y) and torch.equal(y_c, plain[1].y) and torch.equal(gated[1].y, y_c)
    assert plain[0].sums is None and plain[1].sums is None and row_plain.sums is None and row_plain.s_sums is None
    assert gated[0].kind == "gate" and torch.equal(gated[0].y * s * gated[0].c.unsqueeze(1), y_d)
    assert torch.equal(row.y, row_plain.y)
    if few:
        assert all(c.sums is None for c in stored + gated), "few rows: no sums, the statistics pass stays"
    else:
        for tag, c, y in (("f_dense_comp stored", stored[0], y_d), ("f_dense_comp gate only", gated[0], y_d), ("f_comp", stored[1], y_c),
                          ("f_comp (gate-only launch)", gated[1], y_c)):
            share = check_sums(c.sums, y, f"{tag} tied={tied}")
            assert M < 20000 or share <= 0.08
        # stored and gate-only form: the SAME epilogue code formed the sums -- bit-identical partials
        assert torch.equal(total(stored[0].sums, D), total(gated[0].sums, D))
        assert torch.equal(stored[0].sums.buf, gated[0].sums.buf)
    check_sums(row.s_sums, s, f"f_identity tied={tied}")
    check_sums(row.sums, s * row.y.unsqueeze(1), f"row factor tied={tied}")


def first_stage(N, E, R, D, tied, seed):
    from mr_gnas_amd import supernet as S
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.randint(0, N, (E,), generator=gen)
    et = torch.randint(0, 2 * R, (E,), generator=gen)
    g = G.RelGraph(N, src.numpy(), dst.numpy(), et.numpy(), (torch.rand(E, generator=gen) + 0.1).numpy().astype(np.float32), device=DEV)
    h0 = torch.randn(E + N, D, generator=gen)
    hin0 = h0 if tied else torch.randn(E + N, D, generator=gen)
    w0 = torch.softmax(torch.randn(len(O.FIRST_OPS), generator=gen), 0)
    gout = torch.randn(E + N, D, generator=gen).to(DEV)
    torch.manual_seed(seed)
    mixed = S.MixedOp(D, 0.0, O.FIRST_OPS).to(DEV)
    S.xavier_init_(mixed)
    for p in mixed.parameters():                          # biases and gate vectors away from their all-zero / symmetric start
        if p.dim() == 1:
            p.data.add_(0.1 * torch.randn(p.shape, generator=gen).to(DEV))
    return g, mixed, h0, hin0, w0, gout


class Spy:
    """Records (name, args, kw) of every C-ABI call the package's kernel-family modules make."""

    def __init__(self):
        self.calls = []
        self.real = mr_gnas_amd._lib.call
        self.mods = [m for m in vars(K).values() if isinstance(m, types.ModuleType) and getattr(m, "call", None) is self.real]

    def __enter__(self):
        def spy(name, args, **kw):
            self.calls.append((name, args, kw))
            return self.real(name, args, **kw)
        for m in self.mods:
            m.call = spy
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m.call = self.real


STATS_COEF_DESC, COLSTATS_DESC = 13, 6                    # position of the mrg_gated_branch argument


def given_of(gb):
    """Per candidate: partial count of the sums given in a mrg_gated_branch descriptor (0: swept)."""
    if gb is None:
        return [0] * 8
    d = gb._obj
    return [int(d.given_n[k]) if d.given[k] else 0 for k in range(8)]


def run_step(mixed, state0, g, h0, hin0, w0, gout, tied, addend=None):
    mixed.load_state_dict(state0)
    mixed.zero_grad(set_to_none=True)
    h = h0.clone().to(DEV).requires_grad_(True)
    hin = h if tied else hin0.clone().to(DEV).requires_grad_(True)
    w = w0.clone().to(DEV).requires_grad_(True)
    out = mixed(w, g, h, hin, addend=addend)
    fn = out.grad_fn
    assert "MixedEpilogue" in type(fn).__name__
    coef = fn.saved_tensors[1].clone()
    out.backward(gout)
    torch.cuda.synchronize()
    grads = [h.grad] + ([] if tied else [hin.grad]) + [w.grad] + [p.grad.clone() for p in mixed.parameters()]
    return out.detach(), coef, [b.clone() for b in mixed.buffers()], grads


def within_one_ulp(a, b):
    return (a == b) | (torch.nextafter(a, b) == b)


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("N,E,R,D", [(2000, 150000, 9, 200), (1500, 9000, 5, 200), (900, 40000, 4, 168), (300, 5000, 4, 64)])
def test_first_stage_mixedop_with_producer_sums_against_the_statistics_pass(N, E, R, D, tied):
    """Forward + backward with PRODUCER_STATS on against off: coefficients and running statistics within 1 float32 ulp per entry (the
    count that differ is printed), output and gradients within the summation-order tolerances of test_ops_gpu.close; two runs with the
    switch on are bit-identical.  D = 64 and the few-row tied case have no sums in the row GEMM (the pass serves those candidates)."""
    g, mixed, h0, hin0, w0, gout = first_stage(N, E, R, D, tied, 11 * N + E + D + int(tied))
    state0 = {k: v.clone() for k, v in mixed.state_dict().items()}
    res = {}
    try:
        for on in (True, True, False):
            K.switches.PRODUCER_STATS = on
            with Spy() as spy:
                cur = run_step(mixed, state0, g, h0, hin0, w0, gout, tied)
            stats = [a for n, a, _ in spy.calls if n == "mrg_mix_stats_coef"]
            assert len(stats) == 1
            n_given = sum(1 for n_ in given_of(stats[0][STATS_COEF_DESC]) if n_ > 0)
            syms = {kw.get("symbol") for n, _, kw in spy.calls}
            if not on:
                assert n_given == 0 and syms == {None}, "switch off: today's pass, today's entry points"
            else:
                gemm_sums = 128 < D <= 224 and not (tied and E + N <= 16384)
                assert n_given == (4 if gemm_sums else 2), f"{n_given} candidates came with their producer's sums"
                assert ("mrg_dense_filter_fwd3_colsum" in syms) == gemm_sums and "mrg_gate_row_fwd_colsum" in syms
            if on and on in res:
                for i, (a, b) in enumerate(zip([cur[0], cur[1]] + cur[2] + cur[3], [res[on][0], res[on][1]] + res[on][2] + res[on][3])):
                    assert torch.equal(a, b), f"two runs with producer sums differ in tensor {i}"
            res[on] = cur
    finally:
        K.switches.PRODUCER_STATS = True
    (out1, coef1, buf1, gr1), (out0, coef0, buf0, gr0) = res[True], res[False]
    moved = int((coef1 != coef0).sum()) + sum(int((a != b).sum()) for a, b in zip(buf1, buf0) if a.is_floating_point())
    print(f"N={N} E={E} D={D} tied={tied}: {moved} coefficient / running-statistic entries differ (of {coef1.numel()} + buffers)")
    assert bool(within_one_ulp(coef1, coef0).all()), "coefficients: more than 1 ulp"
    for a, b in zip(buf1, buf0):
        assert bool(within_one_ulp(a, b).all()) if a.is_floating_point() else torch.equal(a, b), "running statistics: more than 1 ulp"
    close(out1, out0.cpu(), "output")
    for i, (a, b) in enumerate(zip(gr1, gr0)):
        close(a, b.cpu(), f"gradient {i}")


def test_full_size_first_stage_mixedop_sweeps_no_tensor():
    """Call census at the headline shape (FB15k-237: 544 230 edge rows + 14 541 self rows, D = 200, untied operands): the descriptor
    handed to mrg_mix_stats_coef gives the sums of all four non-zero candidates -- the statistics kernel has nothing to read -- and
    each producer's partial buffer is at most 8 % of one [rows, D] tensor."""
    N, E, D = 14541, 544230, 200
    g, mixed, h0, hin0, w0, gout = first_stage(N, E, 237, D, False, 5)
    state0 = {k: v.clone() for k, v in mixed.state_dict().items()}
    with Spy() as spy:
        run_step(mixed, state0, g, h0, hin0, w0, gout, False)
    stats = [a for n, a, _ in spy.calls if n == "mrg_mix_stats_coef"]
    assert len(stats) == 1 and "mrg_mix_colstats" not in [n for n, _, _ in spy.calls]
    given = given_of(stats[0][STATS_COEF_DESC])
    zero = O.FIRST_OPS.index("f_zero")
    assert [k for k in range(8) if given[k] > 0] == [k for k in range(len(O.FIRST_OPS)) if k != zero], given
    one = (E + N) * D * 4
    for k, n_ in enumerate(given):
        stride = int(stats[0][STATS_COEF_DESC]._obj.given_stride[k])
        assert n_ * stride * 8 <= 0.08 * one, f"candidate {k}: {n_} partials of {stride} doubles"
    names = [n for n, _, _ in spy.calls]
    fwd3 = [(a, kw) for n, a, kw in spy.calls if n == "mrg_dense_filter_fwd3"]
    assert len(fwd3) == 2 and all(kw.get("symbol") == "mrg_dense_filter_fwd3_colsum" for _, kw in fwd3)
    assert names.count("mrg_gate_row_fwd") == 1


def test_producer_sums_are_capturable():
    """One HIP-graph capture of the forward with producer sums, replayed: output and running statistics of the eager run."""
    N, E, R, D = 1200, 60000, 5, 200
    g, mixed, h0, hin0, w0, gout = first_stage(N, E, R, D, False, 3)
    state0 = {k: v.clone() for k, v in mixed.state_dict().items()}
    h, hin, w = h0.to(DEV), hin0.to(DEV), w0.to(DEV)
    with torch.no_grad():
        mixed.load_state_dict(state0)
        out0 = mixed(w, g, h, hin)
        buf0 = [b.clone() for b in mixed.buffers()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mixed(w, g, h, hin)                                 # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        mixed.load_state_dict(state0)
        graph = torch.cuda.CUDAGraph()
        with Spy() as spy, torch.cuda.graph(graph):
            out = mixed(w, g, h, hin)
        assert any(kw.get("symbol") == "mrg_gate_row_fwd_colsum" for _, _, kw in spy.calls)
        assert any(kw.get("symbol") == "mrg_dense_filter_fwd3_colsum" for _, _, kw in spy.calls)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, out0)
    for a, b in zip(mixed.buffers(), buf0):
        assert torch.equal(a, b)


@pytest.mark.parametrize("how", ["eval", "valid_rows", "group"])
def test_the_statistics_pass_stays_where_producer_sums_do_not_apply(how):
    """Eval mode (fixed statistics), a device row count (capacity-padded step graph) and sharded rows (statistics all-reduced over a
    group) keep today's launches: no producer is asked for sums and no descriptor carries any."""
    N, E, R, D = 1200, 60000, 5, 200
    g, mixed, h0, hin0, w0, gout = first_stage(N, E, R, D, False, 9)
    h, hin, w = h0.to(DEV), hin0.to(DEV), w0.to(DEV)
    rows = E + N
    group = None
    if how == "eval":
        mixed.eval()
    elif how == "valid_rows":
        g.valid_rows = {rows: torch.tensor([rows - 7], dtype=torch.int32, device=DEV)}
    else:
        class OneRank:                                        # a communicator of one rank: the sum over ranks is the identity
            is_direct_rccl = True

            def all_reduce(self, t, op):
                return t
        group = OneRank()
    with torch.no_grad(), Spy() as spy:
        out = mixed(w, g, h, hin, group=group, total_rows=rows if group is not None else None)
    torch.cuda.synchronize()
    assert out.shape == (rows, D)
    assert {kw.get("symbol") for _, _, kw in spy.calls} == {None}, "a producer was asked for sums"
    for n, a, _ in spy.calls:
        if n in ("mrg_mix_stats_coef", "mrg_mix_colstats"):
            assert given_of(a[STATS_COEF_DESC if n == "mrg_mix_stats_coef" else COLSTATS_DESC]) == [0] * 8
    names = [n for n, _, _ in spy.calls]
    assert ("mrg_mix_stats_coef" in names) == (how == "valid_rows") and ("mrg_mix_colstats" in names) == (how == "group")
