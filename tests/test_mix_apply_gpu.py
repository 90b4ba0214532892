"""mrg_mix_bwd_apply (the MixedOp epilogue's gradient store) through the MixedOp autograd path, in every role layout the library's
callers reach and on the any-layout kernel: against a float64 evaluation of the same formulas, run to run, and against the bits
the by-index kernel produced (tests/golden/mix_apply_*.npz, recorded by tools/lab/record_mix_apply_golden.py).

The float64 check taps the C-ABI call: it sees exactly the tensors the kernel was given and the tensors it wrote, so its bound is
the rounding of THIS kernel's expressions and of nothing else.  With u = 2^-24 (half an ulp, the relative error of one float32
operation) every quantity carries a value and an error bound; an operation adds u times the magnitude of its result (an fma: one
rounding; a sum of n terms: (n - 1) u times the sum of their magnitudes) to the propagated bounds of its operands:
  z  = v c0 + c1 (an fma), xh = v c2 - c3 (an fma, or the rounded product minus c3: both roundings are allowed for);  gr = [z > 0] w g  -- where |z| is within its own bound the float32 mask may differ:
  the bound of gr grows by |w g| there;  tanh: th within 5 ulp (the OpenCL bound of tanh) plus (1 - th^2) times the bound of z;
  gy = ((gr - c4) - xh c5) c0 live;  folded stores  gc = gy ck, dz = gc s gate (1 - gate), gs = gc gate [+ gy_identity]
  [+ gy_row f + dz_r u];  the row dot q = sum_c gy_row s over n = D columns: sum |s| bound(gy_row) + n u sum |gy_row s|."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import mr_gnas_amd
from mr_gnas_amd import _lib, functional as K, graph as G, operations_lp as O, supernet as S
from mr_gnas_amd.functional import mixed as MX
from conftest import load_golden
from test_producer_stats_gpu import run_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SWITCHES = ("ROW_FACTOR", "GATED_RECOMPUTE", "FOLD_ROW_SCALE", "FOLD_IDENTITY")
LAYOUTS = {"default": {}, "no_row_factor": {"ROW_FACTOR": False}, "no_gated_recompute": {"GATED_RECOMPUTE": False},
           "no_fold_row_scale": {"FOLD_ROW_SCALE": False}, "no_fold_identity": {"FOLD_IDENTITY": False}}
# (nodes = self rows, edges, in-edges): 1, 4, 5 and 257 rows; 3 in / 2 out / 4 self rows: every direction-segment boundary of the
# row factor's gate vectors inside one block
ROWS = {"1": (1, 0, 0), "4": (2, 2, 1), "5": (1, 4, 4), "257": (57, 200, 90), "3+2+4": (4, 5, 3)}
# D: 200 (float4, 64 lanes per row), 64 (16 lanes), 100 (32 lanes), 264 (two column steps per lane: no row role), 50 (scalar lanes)
WIDTHS = (200, 64, 100, 264, 50)


class SplitGraph(G.RelGraph):
    def bounds(self):
        return self._b0, self.num_edges()


@contextlib.contextmanager
def switched(**kw):
    old = {k: getattr(K.switches, k) for k in SWITCHES}
    try:
        for k, v in kw.items():
            assert k in old
            setattr(K.switches, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(K.switches, k, v)


def make_case(ops, N, E, b0, D, tied, seed):
    """A MixedOp over `ops` on E edge rows (the first b0 of them `in` edges) + N self rows, everything from a seeded CPU generator."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.randint(0, N, (E,), generator=gen)
    et = torch.randint(0, 6, (E,), generator=gen)
    g = SplitGraph(N, src.numpy(), dst.numpy(), et.numpy(), (torch.rand(E, generator=gen) + 0.1).numpy().astype(np.float32), device=DEV)
    g._b0 = b0
    h0 = torch.randn(E + N, D, generator=gen)
    hin0 = h0 if tied else torch.randn(E + N, D, generator=gen)
    w0 = torch.softmax(torch.randn(len(ops), generator=gen), 0)
    gout = torch.randn(E + N, D, generator=gen).to(DEV)
    torch.manual_seed(seed)
    mixed = S.MixedOp(D, 0.0, ops).to(DEV)
    S.xavier_init_(mixed)
    for p in mixed.parameters():                          # biases and gate vectors away from their all-zero / symmetric start
        if p.dim() == 1:
            p.data.add_(0.1 * torch.randn(p.shape, generator=gen).to(DEV))
    state0 = {k: v.clone() for k, v in mixed.state_dict().items()}
    return g, mixed, state0, h0, hin0, w0, gout


# ---- the tap: the tensors behind the pointers of one mrg_mix_bwd_apply call ---------------------------------------------------------
class Tap:
    """While active, functional.mixed's pointer helpers remember the tensor behind every address they hand out, and every
    mrg_mix_bwd_apply call is checked against float64 right after it ran.  `calls`: per call a dict with the decoded layout, the
    worst used fraction of the bound and clones of what the kernel wrote."""

    def __init__(self, check=True):
        self.reg, self.calls, self.check = {}, [], check

    def note(self, t):
        if t is not None:
            self.reg[t.data_ptr()] = t
        return t

    def __enter__(self):
        self.saved = (MX.ptr, MX.ptr_array, _lib.ptr_array, _lib.gated_branch, MX.call)
        ptr, ptr_array, gated_branch, call = _lib.ptr, _lib.ptr_array, _lib.gated_branch, MX.call

        def tap_ptr(t):
            return ptr(self.note(t))

        def tap_ptr_array(ts):
            return ptr_array([self.note(t) for t in ts])

        def tap_gated_branch(spec, row_dq=None, act=0, valid_rows=None, given=None):
            for v in (spec or {}).values():
                if torch.is_tensor(v):
                    self.note(v)
            self.note(row_dq), self.note(valid_rows)
            return gated_branch(spec, row_dq, act=act, valid_rows=valid_rows, given=given)

        def tap_call(name, args, **kw):
            if name != "mrg_mix_bwd_apply":
                return call(name, args, **kw)
            torch.cuda.synchronize()
            call(name, args, **kw)
            torch.cuda.synchronize()
            self.calls.append(check_apply(self.reg, args, self.check))

        MX.ptr, MX.ptr_array, _lib.ptr_array, _lib.gated_branch, MX.call = tap_ptr, tap_ptr_array, tap_ptr_array, tap_gated_branch, tap_call
        return self

    def __exit__(self, *exc):
        MX.ptr, MX.ptr_array, _lib.ptr_array, _lib.gated_branch, MX.call = self.saved


class Q:
    """A float64 value with a bound on the float32 kernel's error in it."""

    def __init__(self, v, e=None):
        self.v, self.e = v, torch.zeros_like(v) if e is None else e


def mul(a, b, n=1):
    """a * b rounded n times (b: a Q or an exact tensor)."""
    if not isinstance(b, Q):
        b = Q(b)
    v = a.v * b.v
    return Q(v, a.e * b.v.abs() + b.e * a.v.abs() + a.e * b.e + n * U * v.abs())


def add(terms):
    """The terms added one after the other."""
    v = sum(t.v for t in terms)
    mag = sum(t.v.abs() for t in terms)
    return Q(v, sum(t.e for t in terms) + (len(terms) - 1) * U * mag)


def check_apply(reg, args, check):
    (g_p, ys_p, gys_p, K_, coef_p, coef2_p, w_p, rs_p, rs_scale, rs_self, rs_edge, on_p, full_p, fs_p, fgate_p, fgs_p, fadd_p,
     rows, D, gb, _st) = args
    cpu = lambda p: None if not p else reg[p.value if isinstance(p, ctypes.c_void_p) else p].detach().double().cpu()
    arr = lambda a: [None] * K_ if a is None else [cpu(a[k]) for k in range(K_)]
    g, coef, coef2, w = cpu(g_p), cpu(coef_p).view(K_, 4, D), cpu(coef2_p).view(K_, 2, D), cpu(w_p)
    ys, gys, full, fs, fgate, fgs, rs = arr(ys_p), arr(gys_p), arr(full_p), arr(fs_p), arr(fgate_p), arr(fgs_p), arr(rs_p)
    on = [int(on_p[k]) if on_p is not None else 0 for k in range(K_)]
    add_from = [int(fadd_p[k]) if fadd_p is not None else -1 for k in range(K_)]
    d = gb._obj if gb is not None else None
    gk, rk, act = (int(d.k), int(d.row_k), int(d.act)) if d is not None else (-1, -1, 0)
    s = cpu(d.s) if d is not None and (gk >= 0 or rk >= 0) else None
    nvalid = rows
    if d is not None and d.valid_rows:
        nvalid = max(0, min(rows, int(reg[d.valid_rows].item())))
    live = (torch.arange(rows) < nvalid).double().view(-1, 1)
    col = lambda t: t.view(-1, 1)
    assert g.shape == (rows, D)
    layout = {"K": K_, "gated": gk, "row": rk, "act": act, "on": on, "add_from": add_from, "stored": [k for k in range(K_) if gys[k] is not None],
              "full": [k for k in range(K_) if full[k] is not None], "nvalid": nvalid, "rows": rows, "D": D}
    out = {"layout": layout, "worst": 0.0,
           "written": [reg[gys_p[k]].clone() if gys_p[k] else None for k in range(K_)] + [reg[fgs_p[k]].clone() if fgs_p is not None and fgs_p[k] else None for k in range(K_)]}
    if d is not None and rk >= 0:
        out["written"].append(reg[d.row_dq].clone())
    if not check:
        return out

    def gy(k):
        c0, c1, c2, c3 = coef[k]
        c4, c5 = coef2[k]
        if k == gk:
            v = mul(mul(Q(ys[k]), s), col(cpu(d.rowscale)))
        elif k == rk:
            v = mul(Q(s), col(cpu(d.row_f)))
        else:
            v = Q(ys[k] if ys[k] is not None else torch.zeros(rows, D, dtype=torch.float64))
        z = v.v * c0 + c1
        ez = v.e * c0.abs() + U * z.abs()
        xh = Q(v.v * c2 - c3, v.e * c2.abs() + U * ((v.v * c2).abs() + (v.v * c2 - c3).abs()))      # (an fma, or a rounded product minus c3)
        wg = mul(Q(g), w[k].expand(rows, D))
        if act == 0:
            gr = Q(torch.where(z > 0, wg.v, torch.zeros_like(z)), torch.where(z > 0, wg.e, torch.zeros_like(z)) + torch.where(z.abs() <= ez, wg.v.abs(), torch.zeros_like(z)))
        else:
            th = torch.tanh(z)
            eth = 10 * U * th.abs() + (1 - th * th) * ez + ez * ez
            one = Q(1 - th * th, 2 * th.abs() * eth + eth * eth + 2 * U)
            gr = mul(wg, one)
        t = add([add([gr, Q(-c4.expand(rows, D))]), Q(-(xh.v * c5), xh.e * c5.abs())])       # (the product is inside an fma: no rounding of its own)
        return mul(mul(t, c0.expand(rows, D)), live.expand(rows, D))

    def ck_of(k):
        if full[k] is not None:
            return Q(col(full[k]).expand(rows, D))
        r = torch.arange(rows)
        edge = rs_scale[k] * (rs[k] if rs[k] is not None else torch.ones(rows, dtype=torch.float64))
        v = torch.where(r < int(rs_edge[k]), edge, torch.full((rows,), float(rs_self[k]), dtype=torch.float64))
        return Q(col(v).expand(rows, D), U * col(v).abs().expand(rows, D))

    def compare(what, got, ref):
        got = got.detach().double().cpu()
        err = (got - ref.v).abs()
        bound = ref.e
        frac = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        frac = 0.0 if float(err.max() if err.numel() else 0.0) == 0.0 else frac
        out["worst"] = max(out["worst"], frac)
        assert bool((err <= bound).all()), f"{what}: {frac:.3f} of the bound (layout {layout})"

    orv = dzr = None
    if rk >= 0:
        orv = gy(rk)
        prod = mul(orv, s)
        q = Q(prod.v.sum(1), prod.e.sum(1) + D * U * prod.v.abs().sum(1))
        compare("row dot", reg[d.row_dq], q)
        dzr = mul(Q(col(q.v).expand(rows, D), col(q.e).expand(rows, D)), col(cpu(d.row_h)).expand(rows, D))
    for k in range(K_):
        if gys[k] is None:
            continue
        o = gy(k)
        if on[k]:
            ck = ck_of(k)
            gc = mul(o, ck)
            if on[k] == 2:
                sv, ga = fs[k], fgate[k]
                terms = [mul(gc, ga)]
                if add_from[k] >= 0:
                    terms = [add(terms + [gy(add_from[k])])]
                if rk >= 0 and k == gk:
                    uvc = reg[d.row_uvc].detach().double().cpu()
                    seg = (torch.arange(rows) >= int(d.b0)).long() + (torch.arange(rows) >= int(d.b1)).long()
                    u = uvc[seg][:, :D]
                    a, b = mul(orv, col(cpu(d.row_f)).expand(rows, D), n=0), mul(dzr, u)
                    terms = [add(terms + [add([a, b])])]
                compare(f"gs_out of candidate {k}", reg[fgs_p[k]], terms[0])
                o = mul(mul(mul(gc, sv), ga), Q(1 - ga, U * (1 - ga).abs()))
            else:
                o = gc
        compare(f"gradient of candidate {k}", reg[gys_p[k]], o)
    return out


def run_tapped(case, tied, check=True, addend=None):
    g, mixed, state0, h0, hin0, w0, gout = case
    with Tap(check) as tap:
        res = run_step(mixed, state0, g, h0, hin0, w0, gout, tied, addend=addend)
    assert len(tap.calls) == 1, "one MixedOp: one gradient store"
    return res, tap.calls[0]


def flat(res):
    out, coef, bufs, grads = res
    return [out, coef] + list(bufs) + list(grads)


def check_case(case, tied, expect=None):
    """float64 check of the launch, the layout the launcher was handed, two runs bit-identical."""
    res1, call1 = run_tapped(case, tied)
    res2, call2 = run_tapped(case, tied, check=False)
    lay = call1["layout"]
    print(f"layout {lay}: worst used fraction of the bound {call1['worst']:.3f}")
    for i, (a, b) in enumerate(zip(flat(res1), flat(res2))):
        assert torch.equal(a, b), f"two runs differ in tensor {i}"
    for i, (a, b) in enumerate(zip(call1["written"], call2["written"])):
        assert (a is None and b is None) or torch.equal(a, b), f"two runs differ in written tensor {i}"
    for k, v in (expect or {}).items():
        assert (lay[k] >= 0 if v is True else lay[k] < 0 if v is False else lay[k] == v), f"layout {lay}: expected {k} = {v}"
    return lay


FIRST = O.FIRST_OPS
IDENT, DENSE, SPARSE, COMP = (FIRST.index(n) for n in ("f_identity", "f_dense_comp", "f_sparse_comp", "f_comp"))


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_first_stage_layouts(layout, tied):
    N, E, b0 = ROWS["257"]
    case = make_case(FIRST, N, E, b0, 200, tied, 1000 + 2 * list(LAYOUTS).index(layout) + int(tied))
    with switched(**LAYOUTS[layout]):
        lay = check_case(case, tied)
    if layout == "default":
        assert lay["gated"] == DENSE and lay["row"] == SPARSE and lay["add_from"][DENSE] == IDENT and lay["on"][DENSE] == 2 and lay["on"][COMP] == 1
        assert lay["stored"] == [DENSE, COMP]
    elif layout == "no_row_factor":
        assert lay["gated"] == DENSE and lay["row"] < 0 and lay["add_from"][DENSE] == IDENT and lay["stored"] == [DENSE, SPARSE, COMP]
    elif layout == "no_gated_recompute":
        assert lay["gated"] < 0 and lay["row"] < 0 and DENSE in lay["stored"]
    elif layout == "no_fold_row_scale":
        assert lay["row"] < 0 and lay["on"][COMP] == 0
    else:
        assert lay["gated"] == DENSE and lay["row"] == SPARSE and lay["add_from"][DENSE] < 0 and IDENT in lay["stored"]


@pytest.mark.parametrize("rows", list(ROWS))
def test_first_stage_row_counts(rows):
    N, E, b0 = ROWS[rows]
    for tied in (True, False):
        lay = check_case(make_case(FIRST, N, E, b0, 200, tied, 2000 + N + E + int(tied)), tied, {"gated": True, "row": True})
        assert lay["rows"] == N + E


@pytest.mark.parametrize("D", WIDTHS)
def test_first_stage_widths(D):
    """The gate-only / row-factor forms exist where one float4 step per lane covers the row (D % 4 == 0, D <= 256); the other
    widths keep the stored candidates and run on the any-layout kernel."""
    for rows in ("3+2+4", "257"):
        N, E, b0 = ROWS[rows]
        lay = check_case(make_case(FIRST, N, E, b0, D, False, 3000 + D + N), False)
        roles = D % 4 == 0 and D <= 256
        assert (lay["gated"] >= 0) == roles and (lay["row"] >= 0) == roles, lay
        assert lay["on"][DENSE] == 2 and lay["on"][COMP] == 1 and lay["add_from"][DENSE] == IDENT


@pytest.mark.parametrize("D", [200, 64, 50])
def test_last_stage_mixedop_has_no_gated_role(D):
    N, E, b0 = ROWS["257"]
    lay = check_case(make_case(O.LAST_OPS, N, E, b0, D, True, 4000 + D), True, {"gated": False, "row": False, "K": len(O.LAST_OPS)})
    assert not any(lay["on"]) and len(lay["stored"]) == 3


@pytest.mark.parametrize("D", [200, 264])
def test_six_candidates_run_on_the_any_layout_kernel(D):
    ops = list(O.LAST_OPS) + ["f_dense_last", "f_sparse_last"]
    N, E, b0 = ROWS["257"]
    lay = check_case(make_case(ops, N, E, b0, D, True, 5000 + D), True, {"K": 6})
    assert len(lay["stored"]) == 5


def test_seven_first_stage_candidates_run_on_the_any_layout_kernel():
    """More than five candidates WITH the gated, row and add roles: the any-layout kernel's form of them."""
    ops = list(FIRST) + ["f_identity", "f_sparse_comp"]
    for rows in ("3+2+4", "257"):
        N, E, b0 = ROWS[rows]
        check_case(make_case(ops, N, E, b0, 200, False, 5500 + N), False, {"K": 7, "gated": True})


def test_compgcn_tanh_tail():
    from mr_gnas_amd import compgcn as C
    z = load_golden("compgcn_small")
    g = G.RelGraph(z["N"], z["src"], z["dst"], device=DEV)
    m = z["in_edges_mask"].bool().to(DEV)
    g.edata.update(etype=z["etype"].to(DEV), norm=z["norm"].to(DEV), in_edges_mask=m, out_edges_mask=~m)
    torch.manual_seed(7)
    layer = C.CompGraphConv(z["Din"], z["Dout"], comp_fn="sub", batchnorm=True, dropout=0.0).to(DEV)
    layer.train()
    runs = []
    for check in (True, False):
        layer.zero_grad(set_to_none=True)
        a = z["n_in"].to(DEV).requires_grad_(True)
        b = z["r_in"].to(DEV).requires_grad_(True)
        with Tap(check) as tap:
            no, ro = layer(g, a, b)
            ((no * z["gn"].to(DEV)).sum() + (ro * z["gr"].to(DEV)).sum()).backward()
            torch.cuda.synchronize()
        assert len(tap.calls) == 1 and tap.calls[0]["layout"]["act"] == 1 and tap.calls[0]["layout"]["K"] == 1
        runs.append((tap.calls[0], a.grad.clone(), b.grad.clone()))
    print(f"tanh tail: worst used fraction of the bound {runs[0][0]['worst']:.3f}")
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert torch.equal(runs[0][0]["written"][0], runs[1][0]["written"][0])


def test_capacity_padding_rows_are_written_as_zeros():
    N, E, b0 = ROWS["257"]
    rows, pad = N + E, 9
    for ops, tied in ((FIRST, False), (O.LAST_OPS, True)):
        case = make_case(ops, N, E, b0, 200, tied, 6000 + len(ops))
        case[0].valid_rows = {rows: torch.tensor([rows - pad], dtype=torch.int32, device=DEV)}
        res, call = run_tapped(case, tied)
        assert call["layout"]["nvalid"] == rows - pad
        n_checked = 0
        for t in call["written"]:
            if t is not None:
                assert not bool(t[rows - pad:].any()), "a padding row of a written gradient is not zero"
                assert bool(t[:rows - pad].any())
                n_checked += 1
        assert n_checked >= 3
        print(f"{len(ops)} candidates, {pad} padding rows: worst used fraction of the bound {call['worst']:.3f}")


def _direct_row_factor_call(D, rows=6):
    """mrg_mix_bwd_apply by hand: candidate 0 gated (recomputed, folded), candidate 1 the row factor."""
    gen = torch.Generator().manual_seed(D)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
    g, s, gate = rnd(rows, D), rnd(rows, D), torch.sigmoid(rnd(rows, D))
    c, rf, rh, uvc = rnd(rows).abs() + 0.1, rnd(rows), rnd(rows), rnd(3, D)
    coef, coef2, w = rnd(2, 4, D), 0.01 * rnd(2, 2, D), torch.tensor([0.6, 0.4], device=DEV)
    dz, gs, rdq = torch.empty(rows, D, device=DEV), torch.empty(rows, D, device=DEV), torch.empty(rows, device=DEV)
    gb = _lib.gated_branch(dict(k=0, s=s, c=c, row_k=1, row_f=rf, row_h=rh, row_uvc=uvc, row_ld=D, b0=2, b1=4), rdq)
    one = (ctypes.c_float * 2)(1.0, 1.0)
    _lib.call("mrg_mix_bwd_apply", (_lib.ptr(g), _lib.ptr_array([gate, s]), _lib.ptr_array([dz, None]), 2, _lib.ptr(coef), _lib.ptr(coef2), _lib.ptr(w),
                                    _lib.ptr_array([None, None]), one, one, (ctypes.c_int64 * 2)(rows, rows), (ctypes.c_int * 2)(2, 0),
                                    _lib.ptr_array([c, None]), _lib.ptr_array([s, None]), _lib.ptr_array([gate, None]), _lib.ptr_array([gs, None]),
                                    (ctypes.c_int * 2)(-1, -1), rows, D, gb, _lib.stream_of(g)))
    torch.cuda.synchronize()
    return dz, gs, rdq


def test_row_factor_with_two_column_steps_is_refused():
    """The row dot is one sum over the lanes of a row: a row-factor candidate at D = 264 (two float4 steps per lane) answers
    MRG_E_SHAPE; the same descriptor at D = 200 runs."""
    dz, gs, rdq = _direct_row_factor_call(200)
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(gs).all()) and bool(torch.isfinite(rdq).all())
    with pytest.raises(_lib.MrgnasError) as e:
        _direct_row_factor_call(264)
    assert "(code -2)" in str(e.value), f"{e.value} is not MRG_E_SHAPE"


# ---- the by-index kernel's bits ------------------------------------------------------------------------------------------------------
# name -> (ops, N, E, b0, D, tied, seed, switches): at most 70 rows; the role layouts of the first stage (default; f_identity's
# gradient a tensor of its own) and a last-stage MixedOp.
GOLDEN_CASES = {
    "first_default": (FIRST, 9, 61, 30, 200, False, 101, {}),
    "first_no_fold_identity": (FIRST, 5, 36, 17, 200, True, 102, {"FOLD_IDENTITY": False}),
    "last": (O.LAST_OPS, 10, 60, 30, 64, True, 103, {}),
}


def golden_tensors(name):
    """{key: tensor} of a golden case on this build: what the gradient store wrote (every candidate's gradient, the gated candidate's
    direct term, the row dot) and the one-dimensional gradients behind it (weights, biases, BatchNorm, gate vectors)."""
    ops, N, E, b0, D, tied, seed, sw = GOLDEN_CASES[name]
    with switched(**sw):
        (out, coef, bufs, grads), call = run_tapped(make_case(ops, N, E, b0, D, tied, seed), tied, check=False)
    res = {}
    for i, t in enumerate(grads):
        if t.dim() <= 1:
            res[f"grad{i}"] = t
    for i, t in enumerate(call["written"]):
        if t is not None:
            res[f"written{i}"] = t
    return {k: v.detach().cpu() for k, v in res.items()}


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_bits_of_the_by_index_kernel(name):
    ref = load_golden("mix_apply_" + name)
    got = golden_tensors(name)
    assert ref.pop("seed") == GOLDEN_CASES[name][6]
    assert set(ref) == set(got), "the fixture holds other tensors than this build produces"
    for k in sorted(ref):
        assert torch.equal(got[k], ref[k]), f"{name}: {k} differs from the recorded bits in {int((got[k] != ref[k]).sum())} entries"
