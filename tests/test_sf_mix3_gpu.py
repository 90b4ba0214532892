"""The three-way score-function search leg on the device: csrc/sf_mix_1n.hip (the four-operand register-tiled sweep with its loss,
gradient and counting epilogues), functional.sf_mix3_bce_all, cell_lp.MixedOp_SF.loss_1n over ['sf_TransE', 'sf_DisMult', 'sf_ConvE'],
supernet.ScoreSearchNetwork(sf_ops=...) under architect.search_epoch, evaluation.mix_ranks / predict_mix with ConvE's hidden rows --
against float64, against the two-way sweep (w2 = 0: bit for bit), against the fixed-genotype losses, against the dense literal
formulation and against the reference's own MixedOp_SF (tests/golden/make_golden_sf_mix3.py).
Tile edges of the sweep: 64 queries, 64 entities, 32 columns per slice; a second column block starts at 28 672, a second row chunk at
8 192.  The helpers of test_sf_mix_gpu.py / test_fused_scorers_gpu.py are imported, not copied."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from mr_gnas_amd import _lib, cell_lp as CL, evaluation as EV, functional as K, graph as G, operations_lp as O, supernet as S
from mr_gnas_amd.architect import Architect, search_epoch
from mr_gnas_amd.sampler import LabelIndex
import l1_ref as L1
import sfmix_ref as MX
import sfmix3_ref as M3
from test_fused_scorers_gpu import R, Side, index_of_dense_labels, int_case, make_index, rel_err, smoothed, tiny_graph
from test_sf_mix_gpu import mix_case, rank_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHTS = [(1.0 / 3, 1.0 / 3, 1.0 / 3), (0.2, 0.3, 0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
NAMES = ("g_ent", "g_sub", "g_rel", "g_hidden", "g_w")


def hidden_rows(B, D, ent, seed):
    """Rows as a ReLU leaves them: non-negative with exact zeros (about half), scaled so that |hidden . ent| <= 7."""
    gen = torch.Generator().manual_seed(1000 + seed)
    h = torch.relu(torch.randn(B, D, generator=gen)).to(DEV)
    x2 = h.double() @ ent.double().T
    h = (min(1.0, 7.0 / max(float(x2.abs().max()), 1e-30)) * h.double()).float()
    assert float((h.double() @ ent.double().T).abs().max()) <= 7.0 and float(h.min()) >= 0
    assert B * D < 16 or bool((h == 0).any())
    return h


def mix3_case(B, N, D, seed):
    """mix_case of test_sf_mix_gpu.py (|gamma - dist| <= 7, |(sub * rel) . ent| <= 7) and hidden_rows: no component saturates."""
    ent, sub_e, relb, gamma = mix_case(B, N, D, seed)
    return ent, sub_e, relb, hidden_rows(B, D, ent, seed), gamma


def weights_of(w):
    return torch.tensor(w, dtype=torch.float32, device=DEV)


def run(fn, ent, sub_e, relb, hidden, w, upstream=3.0):
    e, s, r, h, ww = (t.detach().clone().requires_grad_(True) for t in (ent, sub_e, relb, hidden, w))
    loss = fn(e, s, r, h, ww)
    (upstream * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), e.grad, s.grad, r.grad, h.grad, ww.grad


def dense_p(e, s, r, h, w, gamma):
    """The dense float32 formulation on given hidden rows: sum(w * op(...)) of the literal MixedOp_SF.forward, three [B, N] matrices."""
    return sum(wk * pk for wk, pk in zip(w, (K.transe_scores_all(e, s, r, gamma), K.distmult_scores_all(e, s, r), torch.sigmoid(h @ e.t()))))


def dense_fn(li, subj, rel, gamma, label_smooth):
    return lambda e, s, r, h, w: F.binary_cross_entropy(dense_p(e, s, r, h, w, gamma), li.labels(subj, rel, label_smooth))


def fused_fn(li, subj, rel, gamma, label_smooth, col_chunk=None):
    return lambda e, s, r, h, w: K.sf_mix3_bce_all(e, s, r, h, w, gamma, li, subj, rel, label_smooth, col_chunk)


def check_against_f64(got, ref, what):
    assert got[0].dtype == torch.float32 and got[0].dim() == 0
    l64 = float(ref[0])
    print(f"{what}: loss {float(got[0]):.9g} vs {l64:.9g}; rel_err " + " ".join(f"{n} {rel_err(g, r):.2e}" for n, g, r in zip(NAMES, got[1:], ref[1:])))
    assert abs(float(got[0]) - l64) <= 1e-4 * max(1.0, l64), what
    for name, g, r in zip(NAMES, got[1:], ref[1:]):
        assert g.shape == r.shape and rel_err(g, r) <= 1e-4, f"{what} {name}: {rel_err(g, r):.3e}"


def raw_args(ent, sub_e, relb, li, subj, rel, label_smooth):
    """The operands of the no-autograd entry points: obj, qd, qkey and the two label values."""
    obj, qd = (sub_e + relb).contiguous(), (sub_e * relb).contiguous()
    qkey = (subj.long() * (2 * R) + rel.long()).contiguous()
    return obj, qd, qkey, li.label_values(label_smooth)


# ---- 1. loss and gradients against float64 ---------------------------------------------------------------------------------------------
SHAPES = [(1, 449, 33), (63, 63, 64), (65, 64, 200), (129, 65, 31), (129, 1, 1), (65, 65, 1), (5, 28672 + 65, 4), (5, 28672 + 65, 33)]
# label smoothing 0.1 for N >= 10 only: below, the smoothed labels leave [0, 1] and torch's binary_cross_entropy rejects them
CASES = [(B, N, D, ls) for B, N, D in SHAPES for ls in (0.0, 0.1) if ls == 0.0 or N >= 10]


@pytest.mark.parametrize("B,N,D,label_smooth", CASES)
def test_float64_accuracy_without_saturation(B, N, D, label_smooth):
    li, subj, rel, y01 = make_index(N, B, seed=B + N)
    ent, sub_e, relb, hidden, gamma = mix3_case(B, N, D, seed=D)
    x = M3.scores64(ent, sub_e, relb, hidden, gamma)
    assert all(float(t.abs().max()) <= 7.0 for t in x)
    y = smoothed(y01, li, label_smooth)
    for w in WEIGHTS:
        ww = weights_of(w)
        ref = M3.mix3_loss64(ent, sub_e, relb, hidden, ww, y, gamma)
        check_against_f64(run(dense_fn(li, subj, rel, gamma, label_smooth), ent, sub_e, relb, hidden, ww), ref, f"dense w {w}")   # the inputs are fair
        check_against_f64(run(fused_fn(li, subj, rel, gamma, label_smooth), ent, sub_e, relb, hidden, ww), ref, f"fused w {w}")


# ---- 2. w2 = 0 is the two-way sweep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", [(129, 449, 33), (65, 130, 40)])
def test_a_zero_third_weight_is_the_two_way_sweep_bit_for_bit(B, N, D):
    """p = (w0 p0 + w1 p1) + 0 * p2 adds an exact zero, and the two chains, the epilogue expressions and the order of the float64 sums are
    the two-way kernels': the loss, dl0, dl1 and dw[:2] are the same bits, dl2 is zero.  D = 33 stages scalar, D = 40 float4 rows."""
    li, subj, rel, _ = make_index(N, B, seed=3)
    ent, sub_e, relb, hidden, gamma = mix3_case(B, N, D, seed=11)
    obj, qd, qkey, (v0, v1) = raw_args(ent, sub_e, relb, li, subj, rel, 0.1)
    gscale = torch.full((1,), 3.0 / (B * N), device=DEV)
    for a, b in ((0.3, 0.7), (0.55, 0.25)):
        w2, w3 = weights_of((a, b)), weights_of((a, b, 0.0))
        with torch.no_grad():
            assert torch.equal(K.sf_mix3_bce_mean(obj, qd, hidden, ent, w3, gamma, li, qkey, v0, v1),
                               K.sf_mix_bce_mean(obj, qd, ent, w2, gamma, li, qkey, v0, v1))
            for c0, c1 in ((0, N), (64, N)):                   # c0 > 0 adds to dw: both start from the same values
                dw2, dw3 = torch.full((2,), 0.25, device=DEV), torch.full((3,), 0.25, device=DEV)
                t0, t1, dw2 = K.sf_mix_bce_grad(obj, qd, ent, w2, gamma, li, qkey, v0, v1, c0, c1, gscale, dw=dw2)
                d0, d1, d2, dw3 = K.sf_mix3_bce_grad(obj, qd, hidden, ent, w3, gamma, li, qkey, v0, v1, c0, c1, gscale, dw=dw3)
                torch.cuda.synchronize()
                assert torch.equal(d0, t0) and torch.equal(d1, t1) and torch.equal(dw3[:2], dw2)
                assert bool((d2 == 0).all()) and bool((t0 != 0).any()) and bool((t1 != 0).any())
                assert bool(torch.isfinite(dw3[2])) and (c0 > 0 or float(dw3[2]) != 0)


# ---- 3. degenerate weights -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", [(129, 449, 33), (65, 130, 40)])
def test_degenerate_weights_are_the_fixed_genotype_losses(B, N, D):
    """w = (0, 0, 1) is rows_bce_all("dot") on the hidden rows, (1, 0, 0) transe_bce_all, (0, 1, 0) distmult_bce_all: loss to 1e-6 and
    gradients to 1e-5.  Both shapes have D <= 48, where the "dot" sweep runs its exact-float32 core (test_sf_mix_gpu.py says why that
    matters for this bound)."""
    li, subj, rel, _ = make_index(N, B, seed=3)
    ent, sub_e, relb, hidden, gamma = mix3_case(B, N, D, seed=11)
    fixed = {(0.0, 0.0, 1.0): (lambda e, s, r, h, _w: K.rows_bce_all("dot", None, e, h, li, subj, rel, 0.1), (0, 3)),
             (1.0, 0.0, 0.0): (lambda e, s, r, h, _w: K.transe_bce_all(e, s, r, gamma, li, subj, rel, 0.1), (0, 1, 2)),
             (0.0, 1.0, 0.0): (lambda e, s, r, h, _w: K.distmult_bce_all(e, s, r, li, subj, rel, 0.1), (0, 1, 2))}
    for w, (fn, live) in fixed.items():
        want = run(fn, ent, sub_e, relb, hidden, weights_of(w))
        got = run(fused_fn(li, subj, rel, gamma, 0.1), ent, sub_e, relb, hidden, weights_of(w))
        print(f"D={D} w={w}: loss {float(got[0]):.9g} vs {float(want[0]):.9g}; "
              + " ".join(f"{NAMES[i]} {rel_err(got[1 + i], want[1 + i]):.2e}" for i in live))
        assert abs(float(got[0]) - float(want[0])) <= 1e-6 * float(want[0])
        for i in range(4):
            if i in live:
                assert rel_err(got[1 + i], want[1 + i]) <= 1e-5, f"w {w} {NAMES[i]}: {rel_err(got[1 + i], want[1 + i]):.3e}"
            else:                                              # a component of weight 0 passes no gradient to its own operand
                assert want[1 + i] is None and float(got[1 + i].abs().max()) == 0, f"w {w} {NAMES[i]}"
        assert bool(torch.isfinite(got[5]).all())


# ---- 4. saturation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 53, 200])
def test_drop_in_equality_with_the_dense_formulation_saturation_included(D):
    """Weights whose float32 sums stay at or below 1 ((0.2 + 0.3) + 0.5 and (0.25 + 0.25) + 0.5 are exact), so that the dense formulation's
    p stays inside what torch's binary_cross_entropy accepts where every component saturates at 1."""
    B, N, gamma = 129, 449, 40.0
    li, subj, rel, _ = make_index(N, B, seed=7)
    ent, sub_e, relb = int_case(B, N, D, seed=D)
    gen = torch.Generator().manual_seed(D)
    hidden = torch.randint(0, 3, (B, D), generator=gen).float().to(DEV)          # integer-valued, non-negative, a third zeros
    for w in ((0.2, 0.3, 0.5), (0.25, 0.25, 0.5)):
        ww = weights_of(w)
        dense = run(dense_fn(li, subj, rel, gamma, 0.1), ent, sub_e, relb, hidden, ww)
        fused = run(fused_fn(li, subj, rel, gamma, 0.1), ent, sub_e, relb, hidden, ww)
        print(f"D={D} w={w}: loss fused {float(fused[0]):.9g} dense {float(dense[0]):.9g}; "
              + " ".join(f"{n} {rel_err(g, r):.2e}" for n, g, r in zip(NAMES, fused[1:], dense[1:])))
        assert abs(float(fused[0]) - float(dense[0])) <= 1e-6 * float(dense[0])
        for name, g, r in zip(NAMES, fused[1:], dense[1:]):
            assert rel_err(g, r) <= 1e-5, f"w {w} {name}: {rel_err(g, r):.3e}"
    with torch.no_grad():
        ww = weights_of((0.2, 0.3, 0.5))
        ps = (K.transe_scores_all(ent, sub_e, relb, gamma), K.distmult_scores_all(ent, sub_e, relb), torch.sigmoid(hidden @ ent.t()))
        sat = [(p == 0) | (p == 1) for p in ps]
        assert bool((ps[0] == 1).any()) and all(bool((~s).any()) for s in sat[1:]) and (D < 53 or all(bool(s.any()) for s in sat))
        obj, qd, qkey, (v0, v1) = raw_args(ent, sub_e, relb, li, subj, rel, 0.1)
        one = torch.ones(1, device=DEV)
        *dl, dw = K.sf_mix3_bce_grad(obj, qd, hidden, ent, ww, gamma, li, qkey, v0, v1, 0, N, one)
        assert all(d.shape == (B, N) for d in dl) and dw.shape == (3,)
        for d, s in zip(dl, sat):
            assert bool((d[s] == 0).all())
        assert bool((dl[1][~sat[1]] != 0).any()) and bool((dl[2][~sat[2]] != 0).any()) and (D < 53 or bool((dl[0][~sat[0]] != 0).any()))
        *part, _ = K.sf_mix3_bce_grad(obj, qd, hidden, ent, ww, gamma, li, qkey, v0, v1, 64, 449, one)      # a column range is the same numbers
        assert all(torch.equal(p, d[:, 64:449]) for p, d in zip(part, dl))


# ---- 5. chunking and repeatability -----------------------------------------------------------------------------------------------------
def test_chunking_does_not_matter():
    B, N, D = 129, 449, 33
    li, subj, rel, _ = make_index(N, B, seed=3)
    ent, sub_e, relb, hidden, gamma = mix3_case(B, N, D, seed=11)
    ww = weights_of((0.2, 0.3, 0.5))
    base = run(fused_fn(li, subj, rel, gamma, 0.1, None), ent, sub_e, relb, hidden, ww)
    for col_chunk in (64, 100):
        got = run(fused_fn(li, subj, rel, gamma, 0.1, col_chunk), ent, sub_e, relb, hidden, ww)
        assert torch.equal(got[0], base[0])
        for name, g, r in zip(NAMES, got[1:], base[1:]):
            print(f"col_chunk {col_chunk} {name}: {rel_err(g, r):.2e}")
            assert rel_err(g, r) <= 1e-6, f"col_chunk {col_chunk} {name}: {rel_err(g, r):.3e}"


def test_a_batch_that_crosses_a_row_chunk():
    B, N, D = 8192 + 3, 65, 8
    li, subj, rel, y01 = make_index(N, B, seed=5)
    ent, sub_e, relb, hidden, gamma = mix3_case(B, N, D, seed=13)
    ww = weights_of((0.2, 0.3, 0.5))
    ref = M3.mix3_loss64(ent, sub_e, relb, hidden, ww, smoothed(y01, li, 0.1), gamma)
    check_against_f64(run(fused_fn(li, subj, rel, gamma, 0.1), ent, sub_e, relb, hidden, ww), ref, "fused, two row chunks")


@pytest.mark.parametrize("D", [33, 64])
def test_loss_and_gradients_are_bitwise_repeatable(D):
    B, N = 129, 449
    li, subj, rel, _ = make_index(N, B, seed=9)
    ent, sub_e, relb, hidden, gamma = mix3_case(B, N, D, seed=17)
    ww = weights_of((0.2, 0.3, 0.5))
    a = run(fused_fn(li, subj, rel, gamma, 0.1, 128), ent, sub_e, relb, hidden, ww)
    b = run(fused_fn(li, subj, rel, gamma, 0.1, 128), ent, sub_e, relb, hidden, ww)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 6. memory -------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_stays_below_half_a_batch_by_entity_matrix():
    """test_sf_mix_gpu.py's shape and conditions.  Peak allocation of forward + backward beyond what was there before and the gradients
    left behind: fused at most half of a [B, N] float matrix (three gradient slices and the transpose of one are 32 MiB; 35.8 MiB
    measured against 78.1 MiB), the dense formulation at least two (698.8 MiB measured)."""
    B, N, D, col_chunk, gamma = 1024, 20000, 52, 2048, 20.0
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, 3 * N), rng.integers(0, R, 3 * N), rng.integers(0, N, 3 * N)], 1)
    li = LabelIndex(tri, R, N, DEV)
    subj, rel = torch.from_numpy(tri[:B, 0]).to(DEV), torch.from_numpy(tri[:B, 1]).to(DEV)
    gen = torch.Generator().manual_seed(0)
    ent, sub_e, relb = ((0.3 * torch.randn(n, D, generator=gen)).to(DEV) for n in (N, B, B))
    hidden = (0.3 * torch.relu(torch.randn(B, D, generator=gen))).to(DEV)
    ww = weights_of((0.2, 0.3, 0.5))
    matrix = B * N * 4

    def extra(fn):
        leaves = [t.detach().clone().requires_grad_(True) for t in (ent, sub_e, relb, hidden, ww)]
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn(*leaves)
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        return peak - before - sum(t.grad.numel() * 4 for t in leaves), float(loss.detach())

    fused, lf = extra(fused_fn(li, subj, rel, gamma, 0.1, col_chunk))
    dense, ld = extra(dense_fn(li, subj, rel, gamma, 0.1))
    print(f"peak beyond inputs and gradients: fused {fused / 2 ** 20:.1f} MiB, dense {dense / 2 ** 20:.1f} MiB, [B, N] {matrix / 2 ** 20:.1f} MiB")
    assert abs(lf - ld) <= 1e-4 * max(1.0, ld)
    assert fused <= 0.5 * matrix
    assert dense >= 2 * matrix


# ---- 7. ranks --------------------------------------------------------------------------------------------------------------------------
def rank_case3(Q, N, D):
    """rank_case of test_sf_mix_gpu.py (queries, targets, keys, filter index; query Q // 2 repeats query 0) with hidden rows."""
    c = rank_case(Q, N, D)
    c["hidden"] = hidden_rows(Q, D, c["ent"], Q + N + D)
    if Q > 5:
        c["hidden"][Q // 2] = c["hidden"][0]
    return c


def mix3_ranks(c, w, filtered=True):
    side = (c["side"], c["when"], c["qkey"]) if filtered else ()
    return EV.mix_ranks(c["sub"], c["rel"], c["ent"], w, c["gamma"], c["t"], *side, hidden=c["hidden"]).cpu()


def check_band(c, w, what):
    """Every fused rank lies in [lo, hi] of the float64 probabilities, eps = 4 * max(max|dense float32 - float64|, 1e-7): the factor 4 is
    margin for a second float32 implementation of the same expression (test_sf_mix_gpu.py's band)."""
    ww = weights_of(w)
    Q = c["sub"].shape[0]
    with torch.no_grad():
        p32 = torch.cat([dense_p(c["ent"], c["sub"][i:i + 1024], c["rel"][i:i + 1024], c["hidden"][i:i + 1024], ww, c["gamma"])
                         for i in range(0, Q, 1024)])
    p64 = M3.prob64(c["ent"], c["sub"], c["rel"], c["hidden"], ww, c["gamma"])
    eps = 4.0 * max(float((p32.double() - p64).abs().max()), 1e-7)
    assert eps <= 1e-4                                         # the dense formulation is a fair float32 evaluation: the band means something
    p64, t = p64.cpu(), c["t"].cpu()
    out = {}
    for name, got, ok in (("filtered", mix3_ranks(c, ww), c["allowed"]), ("raw", mix3_ranks(c, ww, False), torch.ones_like(c["allowed"]))):
        lo, hi = MX.mix_rank_band(p64, t, ok, eps)
        print(f"{what} w {w} {name}: eps {eps:.2e}, share of exact bands {float((lo == hi).double().mean()):.3f}, "
              f"widest band {int((hi - lo).max())}, max rank {int(got.max())}")
        assert bool(((got >= lo) & (got <= hi)).all()), f"{what} {name}: {int(((got < lo) | (got > hi)).sum())} of {Q} ranks outside the band"
        assert int(got.min()) >= 1 and int(got.max()) <= c["ent"].shape[0]
        out[name] = got
    return out["filtered"], out["raw"]


@pytest.mark.parametrize("Q,N,D", [(65, 449, 200), (300, 65, 33), (63, 64, 1), (129, 449, 64), (5, 28672 + 65, 33)])
def test_ranks_lie_in_the_float64_band(Q, N, D):
    c = rank_case3(Q, N, D)
    for w in WEIGHTS:
        got, raw = check_band(c, w, f"Q {Q} N {N} D {D}")
        assert int(got[1]) == 1                                      # everything but the target filtered
        assert int(got[2]) == int(raw[2])                            # qkey = -1: unfiltered
        if Q > 5:
            assert int(got[Q // 2]) == int(got[0])                   # the repeated query
    assert int(raw.max()) > 1


def test_more_queries_than_one_sweep_launch():
    c = rank_case3(8192 + 130, 33, 4)
    check_band(c, (0.2, 0.3, 0.5), "two row chunks")


@pytest.mark.parametrize("D", [33, 64])
def test_duplicates_of_the_target_row_tie_exactly(D):
    """Copies of one row at ids 10, 150 and 290: whichever is the target, its probability (one thread per query) equals the sweep's for
    the copies bit for bit, so the rank counts exactly the copies at lower ids."""
    N, Q = 300, 70
    ent, sub_e, relb, hidden, gamma = mix3_case(Q, N, D, seed=D)
    ent[150] = ent[290] = ent[10]
    for w in ((1.0 / 3, 1.0 / 3, 1.0 / 3), (0.2, 0.3, 0.5), (0.0, 0.0, 1.0)):
        ranks = [EV.mix_ranks(sub_e, relb, ent, weights_of(w), gamma, torch.full((Q,), t, dtype=torch.int32, device=DEV), hidden=hidden)
                 for t in (10, 150, 290)]
        assert torch.equal(ranks[1], ranks[0] + 1) and torch.equal(ranks[2], ranks[0] + 2)
        assert int(ranks[0].min()) >= 1 and int(ranks[0].max()) > 1


def test_an_all_zero_table_ranks_by_entity_id():
    N, Q, D = 130, 66, 33
    ent = torch.zeros(N, D, device=DEV)
    gen = torch.Generator().manual_seed(1)
    sub_e, relb = (0.2 * torch.randn(Q, D, generator=gen).to(DEV) for _ in range(2))
    hidden = torch.relu(torch.randn(Q, D, generator=gen)).to(DEV)
    ww = weights_of((0.2, 0.3, 0.5))
    t = (torch.arange(Q, device=DEV) * 2 - 1).clamp(min=0).int()
    assert torch.equal(EV.mix_ranks(sub_e, relb, ent, ww, 5.0, t, hidden=hidden), 1 + t.long())
    # one list for every query: the even ids, always in force -> only the odd lower ids count
    side = Side(torch.tensor([0]), torch.tensor([0, N // 2]), torch.arange(0, N, 2), torch.zeros(N // 2))
    when = torch.full((Q,), -1, dtype=torch.int32, device=DEV)
    got = EV.mix_ranks(sub_e, relb, ent, ww, 5.0, t, side, when, torch.zeros(Q, dtype=torch.int64, device=DEV), hidden=hidden)
    assert torch.equal(got, 1 + (t.long() // 2))


def test_mix_ranks_checks_the_hidden_operand_against_the_weights():
    ent, sub_e, relb, hidden, gamma = mix3_case(65, 130, 40, seed=11)
    t = torch.zeros(65, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        EV.mix_ranks(sub_e, relb, ent, weights_of((0.2, 0.3, 0.5)), gamma, t)
    with pytest.raises(ValueError):
        EV.mix_ranks(sub_e, relb, ent, weights_of((0.5, 0.5)), gamma, t, hidden=hidden)


# ---- 8. the reference's own numbers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_loss_1n_matches_the_reference_mixed_op(tag):
    """Bounds: loss rtol 1e-4; rel_err <= 1e-4 for the entity, subject and relation rows and alpha; for the ConvE parameters the bound
    test_conve_gpu.py's check_sf holds the same scorer to against its reference fixture, |err| <= 5e-4 * max|ref| + 5e-6, which is the
    looser of the two (four of those gradients are sums that cancel to zero in exact arithmetic: test_conve_gpu.py, CANCELLING)."""
    z = load_golden("sf_mix3_small")
    assert float(z[f"{tag}/unsaturated_fraction"]) > 0.5 and float(z[f"{tag}/unsaturated_fraction_conve"]) > 0.5
    gamma, ls = float(z[f"{tag}/gamma"]), float(z[f"{tag}/label_smooth"])
    ent, sub_e, relb = (z[f"{tag}/{k}"].to(DEV).requires_grad_(True) for k in ("ent", "sub", "rel"))
    alpha = z[f"{tag}/alpha"].to(DEV).requires_grad_(True)
    B, N = sub_e.shape[0], ent.shape[0]
    subj, rel = torch.arange(B), torch.zeros(B, dtype=torch.long)
    label01 = z[f"{tag}/label01"].float()
    li = index_of_dense_labels(label01, subj, rel, 1, N)
    subj, rel = subj.to(DEV), rel.to(DEV)
    mixed = CL.MixedOp_SF(gamma, M3.THREE, sf_args=M3.conve_args(*z[f"{tag}/conve_shape"])).to(DEV)
    conve = mixed._ops[2][0]
    prefix = f"{tag}/conve/"
    conve.load_state_dict({k[len(prefix):]: v for k, v in z.items() if k.startswith(prefix)})
    mixed.train()
    w = torch.softmax(alpha, dim=1)
    assert mixed._fused_1n(w[0], ent, sub_e, relb)
    _lib.meter.start(["mrg_sfmix3_bce_fwd", "mrg_sfmix_bce_fwd", "mrg_transe_score_fwd", "mrg_linear_fwd", "mrg_conve_conv_fwd"])
    loss = mixed.loss_1n(w[0], ent, sub_e, relb, li, subj, rel, ls)
    rec = _lib.meter.stop()
    # one sweep, one ConvE feature pass, and no dense score: neither TransE's [B, N] kernel nor a row GEMM (ConvE's dense score product
    # is the forward's only mrg_linear_fwd; its fc layer runs on mrg_conve_fc_fwd)
    assert rec["mrg_sfmix3_bce_fwd"]["launches"] == 1 and rec["mrg_conve_conv_fwd"]["launches"] == 1
    assert not {"mrg_transe_score_fwd", "mrg_linear_fwd", "mrg_sfmix_bce_fwd"} & set(rec)
    loss.backward()
    torch.cuda.synchronize()
    print(f"{tag}: loss {float(loss.detach()):.9g} vs {float(z[f'{tag}/loss']):.9g}")
    torch.testing.assert_close(loss.detach().cpu(), z[f"{tag}/loss"], rtol=1e-4, atol=0)
    for name, got in (("g_ent", ent.grad), ("g_sub", sub_e.grad), ("g_rel", relb.grad), ("g_alpha", alpha.grad)):
        err = rel_err(got.cpu(), z[f"{tag}/{name}"])
        print(f"  {name}: rel_err {err:.2e}")
        assert err <= 1e-4, f"{name}: {err:.3e}"
    for name, p in conve.named_parameters():
        ref = z[f"{tag}/g_conve/{name}"]
        assert p.grad is not None, name
        err, scale = float((p.grad.cpu() - ref).abs().max()), float(ref.abs().max())
        print(f"  conve {name}: err {err:.2e} scale {scale:.2e}")
        assert err <= 5e-4 * scale + 5e-6, f"conve {name}: err {err:.3e} scale {scale:.3e}"
    # other orders of the three run the literal lines
    other = CL.MixedOp_SF(gamma, ['sf_TransE', 'sf_ConvE', 'sf_DisMult'], sf_args=M3.conve_args(*z[f"{tag}/conve_shape"])).to(DEV)
    assert not other._fused_1n(w[0].detach(), ent.detach(), sub_e.detach(), relb.detach())


# ---- 9. the network, the architect and the evaluation pass ------------------------------------------------------------------------------
SF_ARGS = M3.conve_args(64, 8, 8, 3, 4)                          # tiny_graph's D = 64; dropouts 0: the dense and the 1-N step draw nothing


def search_case():
    N, Rg, D, tri, _ = tiny_graph()
    B = 96
    g = G.build_search_graph(N, Rg, tri).to(DEV)
    src, _, _ = g.edges(form="all")
    node_id = torch.arange(N, device=DEV).view(-1, 1)
    li = LabelIndex(tri, Rg, N, DEV)
    subj = torch.from_numpy(np.concatenate([tri[:B // 2, 0], tri[:B // 2, 2]])).to(DEV)
    rel = torch.from_numpy(np.concatenate([tri[:B // 2, 1], tri[:B // 2, 1] + Rg])).to(DEV)
    torch.manual_seed(1)
    net = S.ScoreSearchNetwork(DEV, N, Rg, 2, 1, 2, 2, D, D, 5, 40.0, 0.0, 0.0, sf_ops=M3.THREE, sf_args=SF_ARGS).to(DEV)
    S.xavier_init_(net)
    net.train()
    graph = (g, node_id, src, g.edata["e_type"])
    with torch.no_grad():
        net.rel_wt.mul_(0.05)                                    # moderate logits: no saturation
        ent, rel_emb = net(*graph)
        gamma = float(torch.round(L1.dist64(ent[subj] + rel_emb[rel], ent).median()))      # in the middle of the batch's distances
    for m in net.score_func.modules():
        if hasattr(m, "gamma"):
            m.gamma = gamma
    net.gamma = gamma
    return net, graph, torch.stack((subj, rel), 1), li, tri, N, Rg


def test_score_search_network_loss_matches_the_dense_literal_path():
    net, graph, data, li, _, _, _ = search_case()
    net.label_smooth = 0.1
    alphas = net.arch_parameters()
    assert alphas[4].shape == (1, 3) and net.sf_ops == M3.THREE
    conve = net.score_func.cell_score._ops[0]._ops[2][0]
    assert type(conve) is O.sf_ConvE_op and conve.embed_dim == 64

    def step(labels):
        net.zero_grad(set_to_none=True)
        for a in alphas:
            a.grad = None
        loss = net._loss(*graph, data, labels)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}, [a.grad.clone() for a in alphas]

    loss_d, ref, aref = step(li.labels(data[:, 0], data[:, 1], 0.1))
    _lib.meter.start(["mrg_sfmix3_bce_fwd", "mrg_sfmix3_bce_grad"])
    loss_f, got, agot = step(li)
    rec = _lib.meter.stop()
    assert rec["mrg_sfmix3_bce_fwd"]["launches"] == 1 and rec["mrg_sfmix3_bce_grad"]["launches"] >= 1
    print(f"loss 1-N {loss_f:.9g} dense {loss_d:.9g}")
    assert abs(loss_f - loss_d) <= 1e-4 * max(1.0, loss_d)
    assert sorted(got) == sorted(ref)
    conve_keys = [k for k, _ in net.named_parameters() if k.startswith("score_func.")]
    assert len(conve_keys) == len(list(conve.parameters())) == 10
    assert all(k in got for k in conve_keys)                   # every ConvE parameter receives a gradient through the hidden rows ...
    assert all(float(got[k].abs().max()) > 0 for k in conve_keys if k.endswith(("fc.weight", "conv2d.weight", "bn1.weight", "bn2.weight")))
    for k in conve_keys:                                       # ... the dense path's, to the bound of test 8's ConvE parameters
        err, scale = float((got[k] - ref[k]).abs().max()), float(ref[k].abs().max())
        assert err <= 5e-4 * scale + 5e-6, f"{k}: err {err:.3e} scale {scale:.3e}"
    for i, (a, b) in enumerate(zip(agot, aref)):
        print(f"  alpha {i}: rel_err {rel_err(a, b):.2e} (max abs reference {float(b.abs().max()):.2e})")
        assert rel_err(a, b) <= 1e-4, f"alpha {i}: {rel_err(a, b):.3e}"
    assert agot[4].shape == (1, 3) and float(agot[4].abs().min()) > 0


def test_search_epoch_steps_the_three_way_alpha_and_predict_mix_evaluates():
    net, graph, data, li, tri, N, Rg = search_case()
    args = types.SimpleNamespace(momentum=0.9, weight_decay=3e-4, arch_learning_rate=3e-3, arch_weight_decay=1e-3)
    architect = Architect(DEV, net, args)
    optimizer = torch.optim.SGD(net.parameters(), 0.01, momentum=0.9)
    alphas = net.arch_parameters()
    before = alphas[4].detach().clone()
    step = (*graph, data, li)
    loss, arch_loss = search_epoch(net, architect, optimizer, step, step, 1, 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(arch_loss))
    assert alphas[4].shape == (1, 3) and not torch.equal(alphas[4].detach(), before)
    assert net.show_genotypes()[-1].score_func in M3.THREE and net.show_genotypes()[0].score_func is None
    with torch.no_grad():
        alphas[4].copy_(torch.tensor([[-1.0, 0.0, 1.0]]))
    assert net.show_genotypes()[-1].score_func == 'sf_ConvE'
    # the evaluation pass on the embeddings of one forward
    test = torch.from_numpy(np.concatenate([tri[:150], np.stack([tri[:150, 2], tri[:150, 1] + Rg, tri[:150, 0]], 1)]))
    batches = [test[i:i + 64] for i in range(0, test.shape[0], 64)]
    conve = net.score_func.cell_score._ops[0]._ops[2][0]
    net.eval()
    conve.train()                                              # predict_mix puts the scorer in eval mode for the pass itself
    with torch.no_grad():
        ent, rel_emb = net(*graph)
        w = net.score_weights()[0]
        results, loss_sum = EV.predict_mix(batches, ent, rel_emb, w, net.gamma, li, DEV, conve=conve)
        net.eval()
        mixed = net.score_func.cell_score._ops[0]
        dense = 0.0
        for t in batches:
            s, r = t[:, 0].to(DEV), t[:, 1].to(DEV)
            dense += float(F.binary_cross_entropy(mixed(w, ent, ent[s], rel_emb[r]), li.labels(s, r)))
    print(f"predict_mix {results} loss {loss_sum:.9g} dense {dense:.9g}")
    assert results["count"] == 300 and results["mr"] > results["count"] and {"mrr", "mr", "count"} <= set(results)
    assert abs(loss_sum - dense) <= 1e-4 * max(1.0, dense)


def test_a_default_score_search_network_is_what_it_was():
    torch.manual_seed(1)
    net = S.ScoreSearchNetwork(DEV, 50, 3, 2, 1, 2, 2, 8, 8, 5, 40.0, 0.0, 0.0)
    torch.manual_seed(1)
    plain = S.SearchNetwork(DEV, 50, 3, 2, 1, 2, 2, 8, 8, 5, 40.0, 0.0, 0.0)
    assert sorted(net.state_dict()) == sorted(plain.state_dict())
    assert [a.shape for a in net.arch_parameters()] == [a.shape for a in plain.arch_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(net.arch_parameters(), plain.arch_parameters()))
    assert net.arch_parameters()[4].shape == (1, 2) and net.sf_ops == O.SF_OPS
