"""Every lane-geometry instance <VEC, LPR, KMAX> of the row-streaming kernel families on the MI355X (csrc/row_geom.hpp; gate,
compose, dense, accum, segreduce, segstd, mixedop, cell_zero), forward and backward against the float64 restatements of
tests/rowgeom_ref.py (pinned on the CPU by test_row_geometry_cpu.py), at the first and last width of every class, aligned and with
the scalar form forced at a float4 width by a base 4 bytes past a 16-byte boundary (`u`).

Every case brackets its calls with _lib.meter and asserts the entry points it means to test were launched.  A `u` case places the
row operands and the upstream gradient unaligned (parameters stay where nn.Module keeps them) and is also compared with the
aligned run of the same width within twice the bound.

Bounds, all the project's own: outputs and row gradients test_ops_gpu.close() (max error 1e-4 of max(scale, 1) + 2e-5, rms error
1e-4 of the rms); parameter-gradient sums close() with rtol 3e-4, atol 1e-4 (test_star_ops_against_oracle); BatchNorm running
statistics rtol 1e-4, atol 1e-5 (test_conve_gpu).  One bound is widened, for two kinds of tensor: the rms clause of the gate bias
gradients and of the gradient of the architecture weight, to 4 x float32 torch's own error per case (CANCEL_MULT below).  Every
comparison is recorded with conftest.record_margin under "test_row_geometry_gpu.<family>[<class>]".

What the matrix found about routing (asserted below, so a change is noticed):
  * K.compose on plain tensors runs the FLAT kernels mrg_compose_fwd / _bwd, which have no row geometry and no width limit
    (D = 1028 runs); the family's row-geometry kernel is mrg_gather_compose_fwd, reached with LazyRows operands and by
    K.gather_rows.  mrg_sum_buffers is flat as well; the family's row-geometry kernel is mrg_sum_rows_gather.
  * sum / mean on a RelGraph or a Block run mrg_span_gcs forward; mrg_seg_reduce_fwd in its sum / mean modes and
    mrg_seg_reduce_bwd are reached through reducers._seg_fwd and the C ABI.
  * The MixedOp and cell zero admit more candidates forward than backward at the A64k4 widths (rowgeom_ref.mix_limits): the
    forward of K = 2 at D = 1024 runs and its backward is refused by mrg_mix_bwd_reduce before any backward launch.  The tanh
    instances of the MixedOp take five candidates at most, at every width.
  * _lib.meter counts the calls of an entry point that returned MRG_OK and, apart, the ones that returned an error: a refusal
    case asserts that the one error came from the family and that none of the family's entry points completed a call."""
import pytest
import torch

import rowgeom_ref as R
from conftest import record_margin, seeded
from mr_gnas_amd import _lib, functional as K, graph as G
from mr_gnas_amd._lib import call, ptr, ptr_array, stream_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONFIGS = [pytest.param(D, u, id=R.config_id(D, u)) for D, u in R.CONFIGS]
ROWS_TOL = dict(rtol=1e-4, atol=2e-5)           # test_ops_gpu.close
PARAM_TOL = dict(rtol=3e-4, atol=1e-4)          # test_star_ops_against_oracle: close(..., rtol=3e-4, atol=1e-4), its rms clause included
STAT_TOL = dict(rtol=1e-4, atol=1e-5, rms=False)   # test_conve_gpu (torch.testing.assert_close on the running statistics)
# Two kinds of parameter gradient are ONE sum over every row (and column) of mixed-sign terms that cancel: the gate biases
# (d b_x = a_x * sum_r dz_r: 1.2e-3 at D = 64, M = 1031, against terms of total magnitude 0.3) and the architecture weight
# (d w_k = sum_{r, c} g * act(z): 0.3 at D = 256, M = 1031, against 264 000 terms of order 1).  Float32 rounding of the TERMS is
# then more than 1e-4 of the sum, whoever adds them.  For these tensors only, the rms clause is the larger of close()'s and
# CANCEL_MULT x the rms error of the same restatement evaluated in float32 by torch on the CPU, for that case (floor32; two float32
# evaluations differ in the rounding of the terms and in summation order, which moves an error of this kind by a small factor:
# the 4 x that test_gcs_gpu's clause (ii) allows).  The record names the clause that decided.
CANCEL_MULT = 4.0


def is_gate_bias(name):
    return name in ("b", "b_in", "b_out", "b_self")


def rms_err(a, b):
    return float((a.detach().double() - b.detach().double()).square().mean().sqrt())


F32_THREADS = (1, 2, 4, 8)


def floor32(fn, leaves, gout, indices, refs):
    """{i: rms error of gradient i of the restatement fn(*leaves) evaluated in float32 by torch on the CPU, against the float64
    gradient refs[i]} for i in indices.  The error of ONE float32 evaluation of a cancelling sum is a draw: for d w at D = 256, M = 1031 it is 7.9e-5,
    6.8e-5, 4.6e-6 and 4.6e-6 with 1, 2, 4 and 8 threads (torch splits the sum differently).  So the restatement is evaluated at
    each of F32_THREADS and the floor is the rms over them -- the same on every machine, whatever its thread count."""
    before, sq = torch.get_num_threads(), {i: 0.0 for i in indices if refs[i] is not None}
    try:
        for n in F32_THREADS:
            torch.set_num_threads(n)
            L = R.f32(leaves)
            g32 = R.grads(fn(*L), gout, L)
            for i in sq:
                sq[i] += rms_err(g32[i], refs[i]) ** 2
    finally:
        torch.set_num_threads(before)
    return {i: (v / len(F32_THREADS)) ** 0.5 for i, v in sq.items()}


def place(t, unaligned=False):
    return R.place(t, unaligned, DEV)


def leaf(t, unaligned=False):
    return place(t, unaligned).requires_grad_(True)


class Case:
    """One (family, width, placement): holds comparisons to close()'s two bounds, records their margins, and remembers the aligned
    run's results for the `u` comparison."""

    def __init__(self, family, D, unaligned):
        self.name = f"test_row_geometry_gpu.{family}[{R.class_of(D, unaligned)}]"
        self.D, self.un = D, unaligned
        self.failed = []

    def hold(self, tensor, got, ref, rtol, atol, rms=True, factor=1.0, floor=0.0):
        """floor: the rms error of the float32 torch evaluation of a cancelling sum (see CANCEL_MULT), else 0."""
        assert got is not None, f"{self.name} {tensor}: no result"
        got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
        assert got.shape == ref.shape, f"{self.name} {tensor}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
        assert bool(torch.isfinite(got).all()), f"{self.name} {tensor}: non-finite values"
        if ref.numel() == 0:
            return
        scale, err = float(ref.abs().max()), float((got - ref).abs().max())
        bound = factor * (atol + rtol * max(scale, 1.0))
        used, rec = err / bound, (f"D{R.arg_of(self.D, self.un)} {tensor}", err, scale, bound)
        if rms:
            rms_ref, rms_err = float(ref.square().mean().sqrt()), float((got - ref).square().mean().sqrt())
            own, wide = 1e-4 * rms_ref + 1e-9, CANCEL_MULT * floor
            rms_bound = factor * max(own, wide)
            if rms_err / rms_bound > used:
                clause = "rms" if own >= wide else f"rms, {CANCEL_MULT:g} x float32 torch"
                used, rec = rms_err / rms_bound, (f"D{R.arg_of(self.D, self.un)} {tensor} ({clause})", rms_err, rms_ref, rms_bound)
            if wide > own:
                print(f"{self.name} D{R.arg_of(self.D, self.un)} {tensor}: rms err {rms_err:.3e}, float32 torch {floor:.3e}, close()'s rms bound {own:.3e}")
        record_margin(self.name, *rec)                      # the clause that binds
        print(f"{self.name} D{R.arg_of(self.D, self.un)} {tensor}: used {used:.4f} of the bound")
        if not used <= 1.0:
            self.failed.append((tensor, f"err {err:.3e} scale {scale:.3e} used {used:.3f}"))

    def rows(self, tensor, got, ref, **kw):
        self.hold(tensor, got, ref, **ROWS_TOL, **kw)

    def params(self, tensor, got, ref, **kw):
        self.hold(tensor, got, ref, **PARAM_TOL, **kw)

    def stats(self, tensor, got, ref, **kw):
        self.hold(tensor, got, ref, **STAT_TOL, **kw)

    def same_as_aligned(self, results, aligned, kinds, floors=None):
        """The scalar form at a float4 width against the float4 form: within twice the bound of the tensor's kind."""
        for i, ((t, got), (_, ali), kind) in enumerate(zip(results, aligned, kinds)):
            if got is not None:
                getattr(self, kind)(t + " aligned vs unaligned", got, ali, factor=2.0, floor=floors[i] if floors else 0.0)

    def done(self):
        assert not self.failed, f"{self.name}: {self.failed}"


def metered(fn, want, exactly=None):
    """fn() between meter.start() and meter.stop(): every entry point of `want` ran (`exactly`: that many times); returns
    (fn's result, {entry point: launches})."""
    _lib.meter.start()
    try:
        res = fn()
    finally:
        rec = {k: v["launches"] for k, v in _lib.meter.stop().items()}
    for name in want:
        assert rec.get(name, 0) >= 1, f"{name} was not launched: {rec}"
        assert exactly is None or rec[name] == exactly, f"{name}: {rec[name]} launches, expected {exactly}"
    return res, rec


def refused(fn, family_entry_points):
    """fn() raises MRG_E_SHAPE: exactly one call returned an error, it was one of the family's row-geometry entry points, and none of
    them completed a call.  (What the meter can show: the refusing entry points themselves return at their row_geom / LDS check,
    ahead of their first launch -- csrc/*.hip -- which the meter does not see.)"""
    _lib.meter.start()
    try:
        with pytest.raises(_lib.MrgnasError, match=r"code -2\b"):
            fn()
    finally:
        rec = _lib.meter.stop()
    assert not set(rec) & set(family_entry_points), sorted(rec)
    assert sum(_lib.meter.refused.values()) == 1 and set(_lib.meter.refused) <= set(family_entry_points), _lib.meter.refused
    return sorted(rec)


# ---- gate -----------------------------------------------------------------------------------------------------------------------------
GATE_VARIANTS = {1031: ((True, True), (False, False)), 37: ((True, True), (False, False), (True, False), (False, True)), 3: ((True, True),)}


def gate_case(D, M, has_in, has_norm, row_factor=False):
    b0, b1 = R.BOUNDS[M]
    seed = 1000 + D
    s, s_in = R.rows_input("gate s", M, D, seed), (R.rows_input("gate s_in", M, D, seed) if has_in else None)
    g, gq = R.rows_input("gate g", M, D, seed), seeded("gate gq", (M,), seed)
    norm = R.norm_of(b1, seed) if has_norm else None
    P = R.gate_params(D, 2 * D if has_in else D, seed)
    L = R.f64([s, s_in] + P)
    n64 = None if norm is None else norm.double()
    out = R.gate_comp(L[0], L[1], n64, b0, b1, L[2:])
    fvec = R.gate_row_factor(L[0], L[1], n64, b0, b1, L[2:])
    ref = dict(out=out.detach(), grads=R.grads(out, g, L), fvec=fvec.detach(), fgrads=R.grads(fvec, gq, L),
               colsums=torch.stack([L[0].detach().sum(0), L[0].detach().square().sum(0), (L[0] * fvec.view(-1, 1)).detach().sum(0),
                                    (L[0] * fvec.view(-1, 1)).detach().square().sum(0)]))
    # the bias gradients' float32 torch error (CANCEL_MULT), aligned with [out] + grads; 0 for every other tensor
    key, fn, go, g64 = ("ffloors", R.gate_row_factor, gq, ref["fgrads"]) if row_factor else ("floors", R.gate_comp, g, ref["grads"])
    fl = floor32(lambda s_, si_, *p: fn(s_, si_, norm, b0, b1, p), [s, s_in] + P, go, [i for i, n in enumerate(GATE_NAMES) if is_gate_bias(n)], g64)
    ref[key] = [0.0] + [fl.get(i, 0.0) for i in range(len(GATE_NAMES))]
    return dict(s=s, s_in=s_in, g=g, gq=gq, norm=norm, P=P, ref=ref, b=(b0, b1))


GATE_NAMES = ["s", "s_in"] + [f"{w}_{x}" for x in ("in", "out", "self") for w in ("W", "b", "a")]


def run_gate(c, un, row_factor):
    b0, b1 = c["b"]
    s, s_in = leaf(c["s"], un), (leaf(c["s_in"], un) if c["s_in"] is not None else None)
    P = [leaf(p) for p in c["P"]]
    norm = place(c["norm"])
    if not row_factor:
        out = K.gate_comp(s, s_in, norm, b0, b1, *P)
        out.backward(place(c["g"], un))
        extra = None
    else:
        cand = K.gate_comp_row_factor(s, s_in, norm, b0, b1, *P, for_epilogue=K.ForEpilogue(stats=True))
        assert cand.kind == "rowfactor" and cand.y.shape == (c["s"].shape[0],)
        out = cand.y
        out.backward(place(c["gq"], un))
        extra = None
        if cand.sums is not None:
            cs = cand.s_sums
            extra = cs.buf.view(torch.float64).view(cs.n, 4, -1).sum(0)
    return [("out", out)] + [("grad " + n, t.grad if t is not None else None) for n, t in zip(GATE_NAMES, [s, s_in] + P)], extra


@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_gate_comp(D, unaligned):
    """K.gate_comp (mrg_gate_fwd / mrg_gate_bwd) with and without s_in, with and without norm, at 3, 37 and 1031 rows."""
    case = Case("gate", D, unaligned)
    kinds = ["rows", "rows", "rows"] + ["params"] * 9
    for M in R.ROWS:
        for has_in, has_norm in GATE_VARIANTS[M]:
            c = gate_case(D, M, has_in, has_norm)
            (res, _), _ = metered(lambda: run_gate(c, unaligned, False), ["mrg_gate_fwd", "mrg_gate_bwd", "mrg_gate_collapse3", "mrg_gate_param_grad3"], 1)
            tag = f"M{M} in{int(has_in)} norm{int(has_norm)} "
            for (t, got), ref, kind, fl in zip(res, [c["ref"]["out"]] + c["ref"]["grads"], kinds, c["ref"]["floors"]):
                if ref is not None:
                    getattr(case, kind)(tag + t, got, ref, floor=fl)
            if unaligned:
                case.same_as_aligned([(tag + t, x) for t, x in res], run_gate(c, False, False)[0], kinds, c["ref"]["floors"])
    case.done()


@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_gate_row_factor(D, unaligned):
    """K.gate_comp_row_factor (mrg_gate_row_fwd / mrg_gate_row_bwd): the [M] factor, the gradients of s, s_in and every parameter;
    where the class takes one step per lane (mrg_gate_row_colsum_blocks answers non-zero) the colsum form, whose float64 sums are
    the column sums of s, s^2, s * f and (s * f)^2."""
    case = Case("gate_row", D, unaligned)
    kinds = ["rows", "rows", "rows"] + ["params"] * 9
    one_step = R.geom(D, unaligned)[2] == 1
    for M in R.ROWS:
        for has_in, has_norm in GATE_VARIANTS[M][:2]:
            c = gate_case(D, M, has_in, has_norm, row_factor=True)
            (res, sums), _ = metered(lambda: run_gate(c, unaligned, True), ["mrg_gate_row_fwd", "mrg_gate_row_bwd"], 1)
            tag = f"M{M} in{int(has_in)} norm{int(has_norm)} "
            assert (sums is not None) == one_step, f"{tag}: the colsum form ran: {sums is not None}, one step per lane: {one_step}"
            for (t, got), ref, kind, fl in zip(res, [c["ref"]["fvec"]] + c["ref"]["fgrads"], kinds, c["ref"]["ffloors"]):
                if ref is not None:
                    getattr(case, kind)(tag + t, got, ref, floor=fl)
            if sums is not None:
                for i, what in enumerate(("sum s", "sum s^2", "sum s f", "sum (s f)^2")):
                    case.rows(tag + what, sums[i], c["ref"]["colsums"][i])
            if unaligned:
                case.same_as_aligned([(tag + t, x) for t, x in res], run_gate(c, False, True)[0], kinds, c["ref"]["ffloors"])
    case.done()


@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_gate_last(D, unaligned):
    """K.gate_last: every row in the self segment, no s_in, no norm, scale 1."""
    case = Case("gate_last", D, unaligned)
    kinds = ["rows", "rows", "params", "params", "params"]

    def run(s0, g0, P0, un):
        s, P = leaf(s0, un), [leaf(p) for p in P0]
        out = K.gate_last(s, *P)
        out.backward(place(g0, un))
        return [("out", out), ("grad s", s.grad)] + [("grad " + n, p.grad) for n, p in zip("Wba", P)]

    for M in R.ROWS:
        s0, g0 = R.rows_input("gate s", M, D, 1000 + D), R.rows_input("gate g", M, D, 1000 + D)
        P0 = R.gate_params(D, D, 2000 + D, (True, False, False))[:3]
        L = R.f64([s0] + P0)
        ref = R.gate_last(*L)
        refs = [ref.detach()] + R.grads(ref, g0, L)
        floors = [0.0, 0.0, 0.0, floor32(R.gate_last, [s0] + P0, g0, [2], refs[1:])[2], 0.0]      # the bias gradient (CANCEL_MULT)
        res, _ = metered(lambda: run(s0, g0, P0, unaligned), ["mrg_gate_fwd", "mrg_gate_bwd"], 1)
        for (t, got), r, kind, fl in zip(res, refs, kinds, floors):
            getattr(case, kind)(f"M{M} {t}", got, r, floor=fl)
        if unaligned:
            case.same_as_aligned([(f"M{M} {t}", x) for t, x in res], run(s0, g0, P0, False), kinds, floors)
    case.done()


# ---- compose ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_compose(D, unaligned):
    """K.compose for mult / sub / add: with LazyRows operands mrg_gather_compose_fwd (the family's row-geometry kernel; the table
    gradients are mrg_span_gcs sums), and on plain rows the flat mrg_compose_fwd / mrg_compose_bwd.  Forward bit-exact against
    float32 torch, both gradients against float64; K.gather_rows bit-exact."""
    case = Case("compose", D, unaligned)
    for M in R.ROWS:
        seed = 3000 + D + M
        gen = torch.Generator().manual_seed(seed)
        N, Rn = max(2, M // 2), 5
        ent, rel, g = seeded("ent", (N, D), seed), seeded("rel", (Rn, D), seed), R.rows_input("compose g", M, D, 3000 + D)
        ei, ri = torch.randint(0, N, (M,), generator=gen), torch.randint(0, Rn, (M,), generator=gen)
        got = metered(lambda: K.gather_rows(place(ent, unaligned), ei.to(DEV).int()), ["mrg_gather_compose_fwd"], 1)[0]
        assert torch.equal(got.cpu(), ent[ei]), f"M{M} gather"
        for kind in ("mult", "sub", "add"):
            def lazy(un):
                e, r = leaf(ent, un), leaf(rel, un)
                out = K.compose(kind, K.LazyRows(e, K.GatherPlan(ei.to(DEV), N)), K.LazyRows(r, K.GatherPlan(ri.to(DEV), Rn)))
                out.backward(place(g, un))
                return [("out", out), ("grad ent", e.grad), ("grad rel", r.grad)]

            def plain(un):
                s, h = leaf(ent[ei], un), leaf(rel[ri], un)
                out = K.compose(kind, s, h)
                out.backward(place(g, un))
                return [("out", out), ("grad s", s.grad), ("grad hr", h.grad)]

            L = R.f64([ent, rel])
            ref = R.compose(kind, L[0][ei], L[1][ri])
            refs = [ref.detach()] + R.grads(ref, g, L)
            res, rec = metered(lambda: lazy(unaligned), ["mrg_gather_compose_fwd", "mrg_span_gcs"])
            assert rec["mrg_gather_compose_fwd"] == 1 and "mrg_compose_fwd" not in rec
            assert torch.equal(res[0][1].detach().cpu(), R.compose(kind, ent[ei], rel[ri])), f"M{M} {kind}: the fused gather-compose is not bit-exact"
            for (t, x), r in zip(res, refs):
                case.rows(f"M{M} {kind} lazy {t}", x, r)
            S = R.f64([ent[ei], rel[ri]])
            ref = R.compose(kind, *S)
            refs = [ref.detach()] + R.grads(ref, g, S)
            res2, rec = metered(lambda: plain(unaligned), ["mrg_compose_fwd", "mrg_compose_bwd"], 1)
            assert torch.equal(res2[0][1].detach().cpu(), R.compose(kind, ent[ei], rel[ri])), f"M{M} {kind}: compose is not bit-exact"
            for (t, x), r in zip(res2, refs):
                case.rows(f"M{M} {kind} plain {t}", x, r)
            if unaligned:
                case.same_as_aligned([(f"M{M} {kind} lazy {t}", x) for t, x in res], lazy(False), ["rows"] * 3)
                case.same_as_aligned([(f"M{M} {kind} plain {t}", x) for t, x in res2], plain(False), ["rows"] * 3)
    case.done()


# ---- dense --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_dense_dz_pass(D, unaligned):
    """The dense filters' first backward pass, the family's row-geometry kernel, through the C ABI: mrg_dense_filter_dz (one
    direction segment) and mrg_dense_filter_dz3 (all rows; edge rows scaled by norm / 3, self rows by scale_self), kind 0
    (f_dense_comp: dz and the direct term gs) and kind 1 (f_comp)."""
    case = Case("dense_dz", D, unaligned)

    def run(M, kind, un):
        b0, b1 = R.BOUNDS[M]
        g, s = place(R.rows_input("dz g", M, D, 4000 + D), un), place(R.rows_input("dz s", M, D, 4000 + D), un)
        gate = place(torch.sigmoid(R.rows_input("dz z", M, D, 4000 + D)), un)
        norm = place(R.norm_of(max(b1, 1), 4000 + D))
        dz, gs = place(torch.full((M, D), 7.0), un), (place(torch.full((M, D), 7.0), un) if kind == 0 else None)
        call("mrg_dense_filter_dz3", (kind, ptr(g), ptr(s), ptr(gate), ptr(norm), 1.0 / 3.0, 0.75, ptr(dz), ptr(gs), b1, M, D, stream_of(g)))
        dz1, gs1 = place(torch.full((M, D), 7.0), un), (place(torch.full((M, D), 7.0), un) if kind == 0 else None)
        call("mrg_dense_filter_dz", (kind, ptr(g), ptr(s), ptr(gate), None, 0.75, ptr(dz1), ptr(gs1), M, D, stream_of(g)))
        return [("dz3 dz", dz), ("dz3 gs", gs), ("dz dz", dz1), ("dz gs", gs1)]

    for M in R.ROWS:
        b0, b1 = R.BOUNDS[M]
        g, s = (R.rows_input(n, M, D, 4000 + D).double() for n in ("dz g", "dz s"))
        gate = torch.sigmoid(R.rows_input("dz z", M, D, 4000 + D)).double()
        c3 = torch.cat((R.norm_of(max(b1, 1), 4000 + D).double()[:b1] / 3.0, torch.full((M - b1,), 0.75, dtype=torch.float64)))
        c1 = torch.full((M,), float(torch.tensor(0.75)), dtype=torch.float64)
        for kind in (0, 1):
            res, _ = metered(lambda: run(M, kind, unaligned), ["mrg_dense_filter_dz3", "mrg_dense_filter_dz"], 1)
            refs = list(R.dense_dz(kind, g, s, gate, c3)) + list(R.dense_dz(kind, g, s, gate, c1))
            for (t, x), r in zip(res, refs):
                if r is not None:
                    case.rows(f"M{M} kind{kind} {t}", x, r)
            if unaligned:
                case.same_as_aligned([(f"M{M} kind{kind} {t}", x) for t, x in res], run(M, kind, False), ["rows"] * 4)
    case.done()


DENSE_OPS = (("f_dense_comp", 0, True, 1.0 / 3.0), ("f_comp", 1, False, 1.0))


@pytest.mark.parametrize("D,unaligned", [p for p in CONFIGS if p.values[0] >= 4])
def test_dense_filter_comp(D, unaligned):
    """K.dense_filter_comp for f_dense_comp and f_comp, forward and backward against float64.  The row GEMMs around the dz pass
    are not this matrix's subject (their dispatch is not row_geom; D = 1 is left to test_dense_dz_pass for that reason); the case
    prints which entry points the width reached and asserts the dz pass among them: the grouped mrg_dense_filter_dz3 where the
    library offers the grouped gradient GEMMs for the shape (its two workspace queries answer non-zero: the float4 widths from 64
    to 200 of this list), else mrg_dense_filter_dz per segment.  `u`: the
    upstream gradient unaligned -- what the dz pass streams; the operands stay aligned: where the library offers the grouped
    forward (every `u` width but 16) it refuses unaligned operands, which the case asserts."""
    case = Case("dense", D, unaligned)
    kinds = ["rows", "rows", "rows"] + ["params"] * 6

    def run(M, kind, P0, self_scale, un):
        b0, b1 = R.BOUNDS[M]
        s, s_in = leaf(R.rows_input("dense s", M, D, 5000 + D)), leaf(R.rows_input("dense s_in", M, D, 5000 + D))
        P = [None if p is None else leaf(p) for p in P0]
        out = K.dense_filter_comp(kind, s, s_in, place(R.norm_of(max(b1, 1), 5000 + D)), b0, b1, *P, self_scale)
        out.backward(place(R.rows_input("dense g", M, D, 5000 + D), un))
        return [("out", out), ("grad s", s.grad), ("grad s_in", s_in.grad)] + [(f"grad p{i}", None if p is None else p.grad) for i, p in enumerate(P)]

    for M in R.ROWS:
        b0, b1 = R.BOUNDS[M]
        for name, kind, bias, self_scale in DENSE_OPS:
            P0 = R.dense_params(D, 5000 + D, bias)
            L = R.f64([R.rows_input("dense s", M, D, 5000 + D), R.rows_input("dense s_in", M, D, 5000 + D)] + P0)
            ref = R.dense_filter(kind, L[0], L[1], R.norm_of(max(b1, 1), 5000 + D), b0, b1, L[2:], self_scale)
            refs = [ref.detach()] + R.grads(ref, R.rows_input("dense g", M, D, 5000 + D), L)
            res, rec = metered(lambda: run(M, kind, P0, self_scale, unaligned), [])
            lib = _lib.load()
            grouped = lib.mrg_linear_bwd_input3_workspace_bytes(D, D) > 0 and lib.mrg_linear_bwd_weight3_workspace_bytes(b0, b1, M, D, D, D) > 0
            print(f"{case.name} D{R.arg_of(D, unaligned)} M{M} {name}: entry points {sorted(rec)}")
            assert ("mrg_dense_filter_dz3" in rec) == grouped and ("mrg_dense_filter_dz" in rec) == (not grouped), sorted(rec)
            for (t, x), r, kd in zip(res, refs, kinds):
                if r is not None:
                    getattr(case, kd)(f"M{M} {name} {t}", x, r)
            if unaligned:
                case.same_as_aligned([(f"M{M} {name} {t}", x) for t, x in res], run(M, kind, P0, self_scale, False), kinds)
    if unaligned and _lib.load().mrg_dense_filter3_workspace_bytes(D, 2 * D) > 0:
        # unaligned OPERANDS never reach the dz pass at these widths: the grouped row GEMM takes 16-byte aligned rows only
        # (gemm_x3.hpp x3_eligible) and mrg_dense_filter_fwd3 returns MRG_E_SHAPE ahead of its first launch
        for name, kind, bias, self_scale in DENSE_OPS:
            P = [None if p is None else place(p) for p in R.dense_params(D, 5000 + D, bias)]
            s, s_in = leaf(R.rows_input("dense s", 37, D, 5000 + D), True), leaf(R.rows_input("dense s_in", 37, D, 5000 + D), True)
            refused(lambda: K.dense_filter_comp(kind, s, s_in, place(R.norm_of(17, 5000 + D)), 0, 17, *P, self_scale),
                    ["mrg_dense_filter_fwd3", "mrg_dense_filter_fwd", "mrg_dense_filter_dz3", "mrg_dense_filter_dz"])
    case.done()


# ---- accum ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_fan_in_sums(D, unaligned):
    """K.sum_buffers of 2, 3 and 8 tensors (the flat mrg_sum_buffers) and mrg_sum_rows_gather, the family's row-geometry kernel
    (K tensors plus a gather of [N, D] rows: edge row e <- gather_edge[dst[e]], self row n <- gather_self[n]), by the route
    test_fan_in_sum_with_a_gathered_term takes, with and without self rows."""
    case = Case("accum", D, unaligned)
    for M in R.ROWS:
        xs = [R.rows_input(f"sum x{k}", M, D, 6000 + D) for k in range(8)]
        for n in (2, 3, 8):
            run = lambda un: K.sum_buffers([place(x, un) for x in xs[:n]])
            got, _ = metered(lambda: run(unaligned), ["mrg_sum_buffers"], 1)
            case.rows(f"M{M} sum of {n}", got, sum(x.double() for x in xs[:n]))
            if unaligned:
                case.rows(f"M{M} sum of {n} aligned vs unaligned", got, run(False), factor=2.0)
        b0, b1 = R.BOUNDS[M]
        E, N = b1, M - b1
        gen = torch.Generator().manual_seed(6000 + D + M)
        dst = torch.randint(0, N, (E,), generator=gen)
        ge, gself = seeded("gather edge", (N, D), 6000 + D), seeded("gather self", (N, D), 6000 + D)
        for n, with_self in ((0, True), (3, True), (8, False)):
            def run(un):
                out = place(torch.full((M, D), 7.0), un)
                ts = [place(x, un) for x in xs[:n]]
                a, b = place(ge, un), (place(gself, un) if with_self else None)
                call("mrg_sum_rows_gather", (ptr_array(ts), n, ptr(a), ptr(b), ptr(dst.to(DEV).int()), E, M, D, ptr(out), stream_of(out)))
                return out

            got, _ = metered(lambda: run(unaligned), ["mrg_sum_rows_gather"], 1)
            ref = torch.cat((ge[dst], gself if with_self else torch.zeros(N, D))).double() + sum(x.double() for x in xs[:n])
            case.rows(f"M{M} gathered sum of {n} self {int(with_self)}", got, ref)
            if unaligned:
                case.rows(f"M{M} gathered sum of {n} aligned vs unaligned", got, run(False), factor=2.0)
    case.done()


# ---- segreduce / segstd -------------------------------------------------------------------------------------------------------------------
def reducer_case(D):
    src, dst, n_src, n = R.reducer_block(7000 + D)
    E = int(dst.numel())
    msg = seeded("msg", (E, D), 7000 + D, 2.0, 0.5)
    R.condition_max(msg, dst, n)
    std_msg = seeded("msg", (E, D), 7000 + D, 2.0, 0.5)
    std_msg[dst == 21] = 0.75                                   # equal messages in every column / in column 0 only
    std_msg[dst == 22, 0] = -1.5
    return dict(src=src, dst=dst, n_src=n_src, n=n, E=E, msg=msg, std_msg=std_msg, selfr=seeded("self", (n, D), 7000 + D), g=seeded("g", (n, D), 7000 + D))


@pytest.mark.parametrize("with_self", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_segment_reducers(D, unaligned, with_self):
    """Sum, mean and max over the in-edge rows of a block with a 700-edge hub, destinations without in-edges and of in-degree 1:
    mrg_seg_reduce_fwd (reducers._seg_fwd, all three modes), mrg_seg_reduce_bwd_ordered (reducers._seg_bwd) and mrg_seg_reduce_bwd
    (C ABI), then the autograd routes: K.seg_reduce("max") and K.seg_reduce("mean") on a RelGraph and on a Block, and
    K.aggregate_nc("sum") on the Block; the forward of sum and mean is the span kernel."""
    case = Case("segreduce", D, unaligned)
    c = reducer_case(D)
    dst, n, E = c["dst"], c["n"], c["E"]
    blk = G.Block(torch.arange(c["n_src"]), torch.arange(n), c["src"], dst, torch.arange(E)).to(DEV)
    rel = G.RelGraph(n, c["src"] % n, dst, device=DEV)
    assert blk.plan()["n_hubs"] >= 1
    assert R.max_gap(c["msg"].double(), dst, n) >= R.MAX_GAP             # the inputs, before any kernel runs
    sr0 = c["selfr"] if with_self else None

    def direct(kind, un):
        mode = K.REDUCE[kind]
        msg, sr, g = place(c["msg"], un), place(sr0, un), place(c["g"], un)
        out, arg = K._seg_fwd(mode, msg, sr, blk.plan(), n, D)
        gmsg = place(torch.full((E, D), 7.0), un)
        K._seg_bwd(mode, g, blk, arg, gmsg, None)
        gmsg2, gself2 = place(torch.full((E, D), 7.0), un), place(torch.full((n, D), 7.0), un)
        call("mrg_seg_reduce_bwd", (mode, ptr(g), ptr(blk.i32("dst")), ptr(blk.plan()["in_degree"]), ptr(arg), ptr(gmsg2), ptr(gself2), None,
                                    E, n, D, stream_of(g)))
        return [("out", out), ("grad msg (ordered)", gmsg), ("grad msg", gmsg2), ("grad self", gself2)]

    def autograd(fn, un):
        msg, sr = leaf(c["msg"], un), (leaf(sr0, un) if with_self else None)
        out = fn(msg, sr)
        out.backward(place(c["g"], un))
        return [("out", out), ("grad msg", msg.grad), ("grad self", sr.grad if sr is not None else None)]

    for kind in ("sum", "mean", "max"):
        L = R.f64([c["msg"], sr0])
        ref = R.seg_reduce(kind, L[0], L[1], dst, n)
        gm, gs = R.grads(ref, c["g"], L)
        res, _ = metered(lambda: direct(kind, unaligned), ["mrg_seg_reduce_fwd", "mrg_seg_reduce_bwd_ordered", "mrg_seg_reduce_bwd"], 1)
        for (t, x), r in zip(res, [ref.detach(), gm, gm, c["g"].double()]):
            case.rows(f"{kind} {t}", x, r)
        if unaligned:
            case.same_as_aligned([(f"{kind} {t}", x) for t, x in res], direct(kind, False), ["rows"] * 4)
        chunked, spanned = ["mrg_seg_reduce_fwd", "mrg_seg_reduce_bwd_ordered"], ["mrg_span_gcs", "mrg_seg_reduce_bwd_ordered"]
        routes = {"max": [("max on a RelGraph", lambda m, s: K.seg_reduce("max", m, s, rel), chunked),
                          ("max on a Block", lambda m, s: K.seg_reduce("max", m, s, blk), chunked)],
                  "mean": [("mean on a RelGraph", lambda m, s: K.seg_reduce("mean", m, s, rel), spanned),
                           ("mean on a Block", lambda m, s: K.seg_reduce("mean", m, s, blk), spanned)],
                  "sum": [("sum on a Block", lambda m, s: K.aggregate_nc("sum", m, blk) + (s if s is not None else 0), spanned)]}[kind]
        for what, fn, want in routes:
            res, rec = metered(lambda: autograd(fn, unaligned), want, 1)
            assert kind == "max" or "mrg_seg_reduce_fwd" not in rec, sorted(rec)
            for (t, x), r in zip(res, [ref.detach(), gm, gs]):
                if r is not None:
                    case.rows(f"{what} {t}", x, r)
            if unaligned:
                case.same_as_aligned([(f"{what} {t}", x) for t, x in res], autograd(fn, False), ["rows"] * 3)
    case.done()


@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_segment_std(D, unaligned):
    """K.aggregate_std (mrg_seg_std_fwd / mrg_seg_std_bwd) on the reducer block; destinations without in-edges give exactly 0,
    of in-degree 1 and with equal messages sqrt(eps) and no gradient (the assertions of test_a_std_against_float64)."""
    case = Case("segstd", D, unaligned)
    c = reducer_case(D)
    dst, n, E = c["dst"], c["n"], c["E"]
    blk = G.Block(torch.arange(c["n_src"]), torch.arange(n), c["src"], dst, torch.arange(E)).to(DEV)

    def run(un):
        x = leaf(c["std_msg"], un)
        out = K.aggregate_std(x, blk)
        out.backward(place(c["g"], un))
        return [("out", out), ("grad msg", x.grad)]

    (x64,) = R.f64([c["std_msg"]])
    ref = R.seg_std(x64, dst, n)
    res, _ = metered(lambda: run(unaligned), ["mrg_seg_std_fwd", "mrg_seg_std_bwd"], 1)
    for (t, x), r in zip(res, [ref.detach()] + R.grads(ref, c["g"], [x64])):
        case.rows(t, x, r)
    o, gx = res[0][1].detach().cpu(), res[1][1].cpu()
    assert torch.equal(o[1:9], torch.zeros(8, D))                                       # no in-edges: 0
    eps = torch.tensor(1e-5, dtype=torch.float64).sqrt().float()
    assert torch.allclose(o[9:21], eps.expand(12, D), rtol=1e-6, atol=0)                # in-degree 1: sqrt(eps) ...
    assert not gx[(dst >= 9) & (dst < 21)].any()                                        # ... and no gradient
    assert torch.allclose(o[21], eps.expand(D), rtol=1e-6, atol=0) and not gx[dst == 21].any()    # equal messages
    assert torch.allclose(o[22, :1], eps.view(1), rtol=1e-6, atol=0) and not gx[dst == 22, 0].any()
    if unaligned:
        case.same_as_aligned(res, run(False), ["rows"] * 2)
    case.done()


# ---- mixedop ----------------------------------------------------------------------------------------------------------------------------
MIX_MODES = (("relu", True, False), ("relu", False, True), ("tanh", True, True), ("tanh", False, False))     # act, training, addend


def mixed_case(D, rows, Kn, act, training, with_addend):
    """Seeded candidates (candidate 1 of three or more is None), conditioned so that no ReLU argument of the float64 reference lies
    within RELU_MARGIN of zero, and the float64 results."""
    seed = 8000 + D
    present = [not (Kn >= 3 and k == 1) for k in range(Kn)]
    ys = [seeded(f"y{k}", (rows, D), seed, 1.0 + 0.5 * k, 0.5 * k).clone() if p else None for k, p in enumerate(present)]
    gam, bet = [seeded(f"gam{k}", (D,), seed, 0.1, 1.0) for k in range(Kn)], [seeded(f"bet{k}", (D,), seed, 0.3) for k in range(Kn)]
    rm, rv = [seeded(f"rm{k}", (D,), seed, 0.2, 0.5 * k) for k in range(Kn)], [seeded(f"rv{k}", (D,), seed, 0.1, 1.0 + k).abs() + 0.1 for k in range(Kn)]
    w = torch.softmax(seeded("w", (Kn,), seed), 0)
    addend = R.rows_input("mix addend", rows, D, seed) if with_addend else None
    g = R.rows_input("mix g", rows, D, seed)
    live = [k for k in range(Kn) if present[k]]
    args_of = lambda ts: [R.bn_arg(t.double(), gam[k].double(), bet[k].double(), training, rm[k], rv[k]) for k, t in zip(live, ts)]
    margin = None
    if act == "relu":
        stored = [ys[k] for k in live]
        margin = R.condition_relu(stored, args_of, lambda k, bad: (k, bad), seed)
        # an absent candidate's argument is one value per column (BatchNorm of zeros: beta in training mode, beta - rm gamma /
        # sqrt(rv + eps) in eval mode): held to RELU_MARGIN of the candidate's largest, its beta regenerated where it is not
        gen = torch.Generator().manual_seed(seed)
        for k in (k for k in range(Kn) if not present[k]):
            arg = lambda: R.bn_arg(torch.zeros(2, D, dtype=torch.float64), gam[k].double(), bet[k].double(), training, rm[k], rv[k])[0]
            for _ in range(40):
                bad = arg().abs() < 2 * R.RELU_MARGIN * arg().abs().max()
                if not bool(bad.any()):
                    break
                bet[k][bad] += 0.3 * torch.randn(int(bad.sum()), generator=gen)
            margin = min(margin, float(arg().abs().min() / arg().abs().max()))
    L = R.f64([ys[k] for k in live] + gam + bet + [w, addend])
    it = iter(L[:len(live)])
    y64 = [next(it) if p else None for p in present]
    g64, b64 = L[len(live):len(live) + Kn], L[len(live) + Kn:len(live) + 2 * Kn]
    out = R.mixed(y64, g64, b64, L[-2], L[-1], act, training, rm, rv)
    stats = [R.running_stats(ys[k].double(), rm[k], rv[k]) if (training and present[k]) else (rm[k].double(), rv[k].double()) for k in range(Kn)]
    grads = R.grads(out, g, L)

    def restated(*ts):                                          # the same call on other leaves, laid out as L
        it = iter(ts[:len(live)])
        return R.mixed([next(it) if p else None for p in present], ts[len(live):len(live) + Kn], ts[len(live) + Kn:len(live) + 2 * Kn],
                       ts[-2], ts[-1], act, training, rm, rv)

    # float32 torch's error on the gradient of w (CANCEL_MULT), aligned with mixed_refs(); 0 for every other tensor
    iw = len(L) - 2
    floors = [0.0] * (1 + len(L) + 2 * len(live))
    floors[1 + iw] = floor32(restated, [ys[k] for k in live] + gam + bet + [w, addend], g, [iw], grads)[iw]
    return dict(ys=ys, gam=gam, bet=bet, rm=rm, rv=rv, w=w, addend=addend, g=g, margin=margin, present=present, floors=floors,
                ref=dict(out=out.detach(), grads=grads, stats=stats))


def run_mixed(c, act, training, un, backward=True):
    Kn, D = len(c["present"]), c["g"].shape[1]
    bns = [torch.nn.BatchNorm1d(D).to(DEV) for _ in range(Kn)]
    for k, bn in enumerate(bns):
        with torch.no_grad():
            bn.weight.copy_(c["gam"][k]); bn.bias.copy_(c["bet"][k]); bn.running_mean.copy_(c["rm"][k]); bn.running_var.copy_(c["rv"][k])
        bn.train(training)
    ys = [None if y is None else leaf(y, un) for y in c["ys"]]
    w, addend = leaf(c["w"]), (leaf(c["addend"], un) if c["addend"] is not None else None)
    out = K.mixed_epilogue(ys, bns, w, addend=addend, act=act)
    if backward:
        out.backward(place(c["g"], un))
    res = [("out", out)] + [(f"grad y{k}", y.grad) for k, y in enumerate(ys) if y is not None]
    res += [(f"grad gamma{k}", bn.weight.grad) for k, bn in enumerate(bns)] + [(f"grad beta{k}", bn.bias.grad) for k, bn in enumerate(bns)]
    res += [("grad w", w.grad), ("grad addend", addend.grad if addend is not None else None)]
    res += [(f"running_mean{k}", bn.running_mean) for k, bn in enumerate(bns) if c["present"][k]]
    res += [(f"running_var{k}", bn.running_var) for k, bn in enumerate(bns) if c["present"][k]]
    return res


def mixed_kinds(c):
    Kn, nlive = len(c["present"]), sum(c["present"])
    return ["rows"] * (1 + nlive) + ["params"] * (2 * Kn + 1) + ["rows"] + ["stats"] * (2 * nlive)


def mixed_refs(c):
    r = c["ref"]
    live = [k for k, p in enumerate(c["present"]) if p]
    return [r["out"]] + r["grads"] + [r["stats"][k][0] for k in live] + [r["stats"][k][1] for k in live]


MIX_FWD = ["mrg_mix_stats_coef", "mrg_mix_fwd"]
MIX_BWD = ["mrg_mix_bwd_reduce", "mrg_mix_finalize_bwd", "mrg_mix_bwd_apply"]


@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_mixed_epilogue(D, unaligned):
    """K.mixed_epilogue with K = 1, 3 and the largest K the backward admits at the width (rowgeom_ref.mix_limits; 1 at the A64k4
    widths, 5 at most for tanh), one None candidate among three or more, ReLU and tanh, training and eval mode, with and without addend: the output,
    the gradient of every ys[k], w, addend, every BatchNorm gain and bias, and the running statistics.  One candidate beyond the
    backward's limit and at the forward's limit (eight), where the forward admits more than the backward: the forward runs and
    agrees, the backward is refused by mrg_mix_bwd_reduce before anything of the backward is launched.  Nine candidates, and six
    with tanh, are refused before the first launch."""
    case = Case("mixedop", D, unaligned)
    kf, kb = R.mix_limits(D, unaligned)
    kt = R.mix_limits(D, unaligned, R.TANH_MAXK)[1]
    for rows in R.BN_ROWS:
        for act, training, with_addend in (MIX_MODES if rows == R.BN_ROWS[-1] else MIX_MODES[:1]):
            top = kb if act == "relu" else kt
            for Kn in sorted({1, min(3, top), top}):
                c = mixed_case(D, rows, Kn, act, training, with_addend)
                assert c["margin"] is None or c["margin"] >= R.RELU_MARGIN, f"inputs: a ReLU argument at {c['margin']:.2e} of its column's scale"
                res, rec = metered(lambda: run_mixed(c, act, training, unaligned), (MIX_FWD if training else MIX_FWD[1:]) + MIX_BWD, 1)
                assert training or "mrg_mix_stats_coef" not in rec
                tag = f"M{rows} K{Kn} {act} {'train' if training else 'eval'} "
                for (t, x), r, kd, fl in zip(res, mixed_refs(c), mixed_kinds(c), c["floors"]):
                    if r is not None:
                        getattr(case, kd)(tag + t, x, r, floor=fl)
                if unaligned:
                    case.same_as_aligned([(tag + t, x) for t, x in res], run_mixed(c, act, training, False), mixed_kinds(c), c["floors"])
    for Kn in (sorted({kb + 1, kf}) if kb < kf else ()):        # one beyond the backward's limit, and the forward's own limit
        c = mixed_case(D, R.BN_ROWS[0], Kn, "relu", True, False)
        res, rec = metered(lambda: run_mixed(c, "relu", True, unaligned, backward=False), MIX_FWD, 1)
        case.rows(f"K{Kn} forward beyond the backward's limit", res[0][1], c["ref"]["out"])
        refused(lambda: res[0][1].backward(place(c["g"], unaligned)), MIX_BWD)
    for training in (True, False):                              # one beyond the forward's limit (MRG_MIX_MAXK at every width)
        c = mixed_case(D, R.BN_ROWS[0], kf + 1, "relu", training, False)
        refused(lambda: run_mixed(c, "relu", training, unaligned), MIX_FWD + MIX_BWD)
    if kt == R.TANH_MAXK:                                       # the tanh instances: six candidates are refused before the first launch
        for training in (True, False):
            c = mixed_case(D, R.BN_ROWS[0], R.TANH_MAXK + 1, "tanh", training, False)
            refused(lambda: run_mixed(c, "tanh", training, unaligned), MIX_FWD + MIX_BWD)
    case.done()


# ---- cell zero --------------------------------------------------------------------------------------------------------------------------
KINDS = ("mult", "sub", "add")


def zero_case(D, rows, kinds, training):
    seed = 9000 + D
    gen = torch.Generator().manual_seed(seed + rows)
    N, Rn, Kn = max(3, (rows * 3) // 5), 7, len(kinds)
    ent, rel = seeded("ent", (N, D), seed), seeded("rel", (Rn, D), seed)
    ei, ri = torch.randint(0, N, (rows,), generator=gen), torch.randint(0, Rn, (rows,), generator=gen)
    gam, bet = [seeded(f"gam{k}", (D,), seed, 0.1, 1.0) for k in range(Kn)], [seeded(f"bet{k}", (D,), seed, 0.3) for k in range(Kn)]
    rm, rv = [seeded(f"rm{k}", (D,), seed, 0.2) for k in range(Kn)], [seeded(f"rv{k}", (D,), seed, 0.1, 1.5).abs() + 0.1 for k in range(Kn)]
    w, g = torch.softmax(seeded("w", (Kn,), seed), 0), R.rows_input("zero g", rows, D, seed)

    def args_of(ts):
        x, h = ts[0].double()[ei], ts[1].double()[ri]
        return [R.bn_arg(R.compose(kd, x, h), gam[k].double(), bet[k].double(), training, rm[k], rv[k]) for k, kd in enumerate(kinds)]

    def touch(k, bad):
        mask, rmask = torch.zeros(N, D, dtype=torch.bool), torch.zeros(Rn, D, dtype=torch.bool)
        r, col = bad.nonzero(as_tuple=True)
        mask[ei[r], col] = True
        dead = rel[ri[r], col].abs() < 0.05               # a product with a relation entry near zero does not follow the entity's entry
        rmask[ri[r][dead], col[dead]] = True
        return [(0, mask), (1, rmask)]

    tables = [ent, rel]
    margin = R.condition_relu(tables, args_of, touch, seed)
    L = R.f64([ent, rel] + gam + bet + [w])
    out = R.cell_zero(kinds, L[0], L[1], ei, ri, L[2:2 + Kn], L[2 + Kn:2 + 2 * Kn], L[-1], training, rm, rv)
    grads = R.grads(out, g, L)
    restated = lambda *ts: R.cell_zero(kinds, ts[0], ts[1], ei, ri, ts[2:2 + Kn], ts[2 + Kn:2 + 2 * Kn], ts[-1], training, rm, rv)
    # float32 torch's error on the gradient of w (CANCEL_MULT), aligned with [out] + grads; 0 for every other tensor
    floors = [0.0] * len(L) + [floor32(restated, [ent, rel] + gam + bet + [w], g, [len(L) - 1], grads)[len(L) - 1]]
    return dict(ent=ent, rel=rel, ei=ei, ri=ri, gam=gam, bet=bet, rm=rm, rv=rv, w=w, g=g, margin=margin, floors=floors,
                ref=dict(out=out.detach(), grads=grads))


def run_zero(c, kinds, training, un, backward=True):
    Kn, D = len(kinds), c["ent"].shape[1]
    bns = [torch.nn.BatchNorm1d(D).to(DEV) for _ in range(Kn)]
    for k, bn in enumerate(bns):
        with torch.no_grad():
            bn.weight.copy_(c["gam"][k]); bn.bias.copy_(c["bet"][k]); bn.running_mean.copy_(c["rm"][k]); bn.running_var.copy_(c["rv"][k])
        bn.train(training)
    ent, rel, w = leaf(c["ent"], un), leaf(c["rel"], un), leaf(c["w"])
    gp_e, gp_r = K.GatherPlan(c["ei"].to(DEV), c["ent"].shape[0]), K.GatherPlan(c["ri"].to(DEV), c["rel"].shape[0])
    out = K.cell_zero_mixed(kinds, K.LazyRows(ent, gp_e), K.LazyRows(rel, gp_r), bns, w)
    if backward:
        out.backward(place(c["g"], un))
    return ([("out", out), ("grad ent", ent.grad), ("grad rel", rel.grad)] + [(f"grad gamma{k}", bn.weight.grad) for k, bn in enumerate(bns)]
            + [(f"grad beta{k}", bn.bias.grad) for k, bn in enumerate(bns)] + [("grad w", w.grad)])


ZERO_FWD = ["mrg_zero_stats_coef", "mrg_zero_fwd"]
ZERO_BWD = ["mrg_zero_bwd_reduce", "mrg_zero_bwd_apply"]


@pytest.mark.parametrize("D,unaligned", CONFIGS)
def test_cell_zero(D, unaligned):
    """K.cell_zero_mixed over the three compose kinds with LazyRows operands (mrg_zero_*): the output, both table gradients, the
    BatchNorm gradients and w, in training and in eval mode.  Where the backward admits fewer than three candidates (one at the
    A64k4 widths, rowgeom_ref.mix_limits) each kind runs alone, and the three together run forward and are refused backward by
    mrg_zero_bwd_reduce before anything of the backward is launched."""
    case = Case("cell_zero", D, unaligned)
    kf, kb = R.mix_limits(D, unaligned, R.ZERO_MAXK)
    sets = [KINDS] if kb >= 3 else [(kd,) for kd in KINDS]
    for rows in R.BN_ROWS:
        for kinds in sets:
            for training in ((True, False) if rows == R.BN_ROWS[-1] else (True,)):
                c = zero_case(D, rows, kinds, training)
                assert c["margin"] >= R.RELU_MARGIN, f"inputs: a ReLU argument at {c['margin']:.2e} of its column's scale"
                res, rec = metered(lambda: run_zero(c, kinds, training, unaligned), (ZERO_FWD if training else ZERO_FWD[1:]) + ZERO_BWD, 1)
                tag = f"M{rows} {'+'.join(kinds)} {'train' if training else 'eval'} "
                kds = ["rows"] * 3 + ["params"] * (2 * len(kinds) + 1)
                for (t, x), r, kd, fl in zip(res, [c["ref"]["out"]] + c["ref"]["grads"], kds, c["floors"]):
                    getattr(case, kd)(tag + t, x, r, floor=fl)
                if unaligned:
                    case.same_as_aligned([(tag + t, x) for t, x in res], run_zero(c, kinds, training, False), kds, c["floors"])
    if kb < 3 <= kf:
        c = zero_case(D, R.BN_ROWS[0], KINDS, True)
        res, rec = metered(lambda: run_zero(c, KINDS, True, unaligned, backward=False), ZERO_FWD, 1)
        case.rows("three kinds forward beyond the backward's limit", res[0][1], c["ref"]["out"])
        refused(lambda: res[0][1].backward(place(c["g"], unaligned)), ZERO_BWD)
    for training in (True, False):                              # a fourth candidate: beyond ZK, refused before the first launch
        c = zero_case(D, R.BN_ROWS[0], KINDS + ("mult",), training)
        refused(lambda: run_zero(c, KINDS + ("mult",), training, unaligned), ZERO_FWD + ZERO_BWD)
    case.done()


# ---- the widths nobody covers -----------------------------------------------------------------------------------------------------------
def tiny(D, un, M=3):
    return leaf(torch.ones(M, D), un)


def tiny_bns(D, n):
    return [torch.nn.BatchNorm1d(D).to(DEV) for _ in range(n)]


def tiny_block():
    return G.Block(torch.arange(3), torch.arange(2), torch.tensor([0, 1, 2]), torch.tensor([0, 0, 1]), torch.arange(3)).to(DEV)


def tiny_abi(name, D, un, args):
    """A C-ABI call on two tiny [3, D] tensors that stay alive across it: args(a, b, stream) -> the argument tuple."""
    a, b = tiny(D, un).detach(), tiny(D, un).detach()
    call(name, args(a, b, stream_of(a)))
    torch.cuda.synchronize()


def tiny_lazy(D, un):
    idx = torch.tensor([0, 1, 1], device=DEV)
    return K.LazyRows(tiny(D, un, 2), K.GatherPlan(idx, 2)), K.LazyRows(tiny(D, un, 2), K.GatherPlan(idx, 2))


REFUSALS = {
    "gate": (lambda D, u: K.gate_comp(tiny(D, u), tiny(D, u), None, 1, 2, *[place(p) for p in R.gate_params(D, 2 * D, 1)]), ["mrg_gate_fwd", "mrg_gate_bwd"]),
    "gate_last": (lambda D, u: K.gate_last(tiny(D, u), *[place(p) for p in R.gate_params(D, D, 1, (True, False, False))[:3]]), ["mrg_gate_fwd", "mrg_gate_bwd"]),
    "gate_row": (lambda D, u: K.gate_comp_row_factor(tiny(D, u), tiny(D, u), None, 1, 2, *[place(p) for p in R.gate_params(D, 2 * D, 1)]),
                 ["mrg_gate_row_fwd", "mrg_gate_row_bwd"]),
    "compose": (lambda D, u: K.compose("sub", *tiny_lazy(D, u)), ["mrg_gather_compose_fwd"]),
    "gather": (lambda D, u: K.gather_rows(tiny(D, u, 2).detach(), torch.tensor([0, 1, 1], device=DEV, dtype=torch.int32)), ["mrg_gather_compose_fwd"]),
    "dense_dz": (lambda D, u: tiny_abi("mrg_dense_filter_dz", D, u, lambda g, dz, st: (1, ptr(g), None, None, None, 1.0, ptr(dz), None, 3, D, st)),
                 ["mrg_dense_filter_dz"]),
    "dense_dz3": (lambda D, u: tiny_abi("mrg_dense_filter_dz3", D, u, lambda g, dz, st: (1, ptr(g), None, None, None, 1.0, 1.0, ptr(dz), None, 2, 3, D, st)),
                  ["mrg_dense_filter_dz3"]),
    "accum": (lambda D, u: tiny_abi("mrg_sum_rows_gather", D, u, lambda x, out, st: (ptr_array([x]), 1, ptr(x), None, ptr(torch.zeros(2, dtype=torch.int32, device=DEV)),
                                                                                   2, 3, D, ptr(out), st)), ["mrg_sum_rows_gather"]),
    "segreduce": (lambda D, u: K.seg_reduce("max", tiny(D, u), None, tiny_block()), ["mrg_seg_reduce_fwd", "mrg_seg_reduce_bwd_ordered"]),
    "segreduce_bwd": (lambda D, u: K._seg_bwd(0, tiny(D, u, 2).detach(), tiny_block(), None, tiny(D, u).detach(), None), ["mrg_seg_reduce_bwd_ordered"]),
    "segstd": (lambda D, u: K.aggregate_std(tiny(D, u), tiny_block()), ["mrg_seg_std_fwd", "mrg_seg_std_bwd"]),
    "mixedop": (lambda D, u: K.mixed_epilogue([tiny(D, u)], tiny_bns(D, 1), leaf(torch.ones(1))), ["mrg_mix_stats_coef", "mrg_mix_fwd"] + MIX_BWD),
    "mixedop_eval": (lambda D, u: K.mixed_epilogue([tiny(D, u)], [b.eval() for b in tiny_bns(D, 1)], leaf(torch.ones(1))), ["mrg_mix_fwd"] + MIX_BWD),
    "cell_zero": (lambda D, u: K.cell_zero_mixed(KINDS, *tiny_lazy(D, u), tiny_bns(D, 3), leaf(torch.ones(3) / 3)), ZERO_FWD + ZERO_BWD),
    "cell_zero_eval": (lambda D, u: K.cell_zero_mixed(KINDS, *tiny_lazy(D, u), [b.eval() for b in tiny_bns(D, 3)], leaf(torch.ones(3) / 3)), ZERO_FWD[1:] + ZERO_BWD),
}


@pytest.mark.parametrize("family", sorted(REFUSALS))
def test_uncovered_widths_are_refused(family):
    """Returned before any launch of the family's row-geometry entry points: D > 256 with D % 4 != 0, D > 1024, and D > 256 on a
    base that is not 16-byte aligned are MRG_E_SHAPE (as test_gcs_gpu.test_uncovered_widths_are_refused holds fused_gcs)."""
    fn, entry_points = REFUSALS[family]
    for D, unaligned in R.REFUSED:
        ran = refused(lambda: fn(D, unaligned), entry_points)
        print(f"{family} D{R.arg_of(D, unaligned)}: refused; launched before the refusal: {ran}")


def test_flat_kernels_have_no_width_limit():
    """mrg_compose_fwd / _bwd and mrg_sum_buffers walk rows * D floats flat: no row geometry, no refused width."""
    for D, unaligned in R.REFUSED:
        s, h = tiny(D, unaligned), tiny(D, unaligned)
        (out, _), _ = metered(lambda: (K.compose("add", s, h), K.compose("add", s, h).backward(torch.ones_like(s))), ["mrg_compose_fwd", "mrg_compose_bwd"])
        assert torch.equal(out.detach().cpu(), torch.full((3, D), 2.0)) and torch.equal(s.grad.cpu(), torch.ones(3, D))
        got, _ = metered(lambda: K.sum_buffers([s.detach(), h.detach(), s.detach()]), ["mrg_sum_buffers"], 1)
        assert torch.equal(got.cpu(), torch.full((3, D), 3.0))
