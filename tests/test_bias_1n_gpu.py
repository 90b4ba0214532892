"""The "dot" sweeps under a per-entity score bias, logit = q . ent[e] + bias[e], without [B, N] tensors on the device: csrc/bce.hip
(EPI_BCE_BIAS / EPI_BCE_GRAD_BIAS, mrg_cols_sum), csrc/rank.hip (EPI_RANK_BIAS, the target score's bias), csrc/topk.hip (EPI_TOPK_BIAS),
functional.rows_bce_all(bias=), evaluation.query_ranks / query_topk (bias=) and compgcn.CompGCN_ConvE.loss_1n / predict_1n / predict_topk,
against float64, against the dense device path (linear(q, ent, bias, "sigmoid") + F.binary_cross_entropy on LabelIndex.labels) and
against the reference's recorded step (tests/golden/compgcn_conve_1n.npz).  Tolerances are those of test_fused_bce_gpu.py,
test_topk_gpu.py and test_mrr_gpu.py: the bias adds one exact float32 add to those sweeps."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mrr_ref as MR
import topk_ref as TR
from conftest import assert_param_grad, load_golden, sub
from mr_gnas_amd import _lib, compgcn as CG, evaluation as EV, functional as K, graph as G
from mr_gnas_amd.sampler import LabelIndex
from test_fused_bce_gpu import R, make_index, rel_err, smoothed

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("g_ent", "g_q", "g_bias")


def float_case(B, N, D, seed):
    """Random float operands with float64 max |q . ent| <= 7 (the query rows are scaled down where the draw exceeds it) and a bias drawn
    in [-1, 1]: max |x| <= 8."""
    gen = torch.Generator().manual_seed(seed)
    scale = 0.5 if D <= 4 else (0.3 if D <= 64 else 0.15)
    ent = scale * torch.randn(N, D, generator=gen)
    q = scale * torch.randn(B, D, generator=gen) * torch.randn(B, D, generator=gen)
    x = q.double() @ ent.double().t()
    q = (q * min(1.0, 7.0 / float(x.abs().max()))).contiguous()
    bias = 2.0 * torch.rand(N, generator=gen) - 1.0
    return ent.to(DEV), q.to(DEV), bias.to(DEV)


def loss64(ent, q, bias, y):
    """The float64 formula on float64 logits: (loss, g_ent, g_q, g_bias) of 3 * loss."""
    e, s, b = (t.detach().double().requires_grad_(True) for t in (ent, q, bias))
    x = s @ e.t() + b
    assert float(x.detach().abs().max()) <= 8.0
    loss = -(y * F.logsigmoid(x) + (1.0 - y) * F.logsigmoid(-x)).mean()
    (3 * loss).backward()
    return loss.detach(), e.grad, s.grad, b.grad


def run(fn, ent, q, bias, upstream=3.0):
    e, s, b = (t.detach().clone().requires_grad_(True) for t in (ent, q, bias))
    loss = fn(e, s, b)
    (upstream * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), e.grad, s.grad, b.grad


def dense_fn(li, subj, rel, label_smooth):
    return lambda e, s, b: F.binary_cross_entropy(K.linear(s, e, b, "sigmoid"), li.labels(subj, rel, label_smooth))


def fused_fn(li, subj, rel, label_smooth, col_chunk=None):
    return lambda e, s, b: K.rows_bce_all("dot", None, e, s, li, subj, rel, label_smooth, col_chunk, bias=b)


def check_against_f64(got, ref, what):
    assert got[0].dtype == torch.float32 and got[0].dim() == 0
    l64 = float(ref[0])
    print(f"{what}: loss {float(got[0]):.9g} vs {l64:.9g}; " + " ".join(f"{n} {rel_err(g, r):.2e}" for n, g, r in zip(NAMES, got[1:], ref[1:])))
    assert abs(float(got[0]) - l64) <= 1e-4 * max(1.0, l64), what
    for name, g, r in zip(NAMES, got[1:], ref[1:]):
        assert g.shape == r.shape and rel_err(g, r) <= 1e-4, f"{what} {name}: {rel_err(g, r):.3e}"


# every B of {1, 127, 129, 257} and every N of {1, 33, 224, 225, 449} with the split core (D = 52, 64, 200) and with the exact core
# (D = 4: vectorised loads, D = 50: plain loads); N = 28 672 + 33 sweeps a second column block on each core, which gets bias + 28 672
SHAPES = [(1, 449, 52), (127, 33, 64), (129, 224, 200), (257, 225, 52), (129, 1, 64), (127, 449, 200),
          (1, 225, 4), (127, 449, 50), (129, 33, 4), (257, 224, 50), (127, 1, 4), (5, 28672 + 33, 4), (5, 28672 + 33, 52)]
# label smoothing 0.1 needs N >= 10 (below it the smoothed labels leave [0, 1], which the dense path's loss rejects)
CASES = [(B, N, D, ls) for B, N, D in SHAPES for ls in (0.0, 0.1) if ls == 0.0 or N >= 10]


@pytest.mark.parametrize("B,N,D,label_smooth", CASES)
def test_float64_accuracy_without_saturation(B, N, D, label_smooth):
    li, subj, rel, y01 = make_index(N, B, seed=B + N)
    ent, q, bias = float_case(B, N, D, seed=D)
    ref = loss64(ent, q, bias, smoothed(y01, li, label_smooth))
    check_against_f64(run(dense_fn(li, subj, rel, label_smooth), ent, q, bias), ref, "dense")       # the inputs are fair
    check_against_f64(run(fused_fn(li, subj, rel, label_smooth), ent, q, bias), ref, "fused")


def test_a_batch_that_crosses_a_row_chunk():
    B, N, D = 8192 + 5, 33, 4
    li, subj, rel, y01 = make_index(N, B, seed=5)
    ent, q, bias = float_case(B, N, D, seed=13)
    ref = loss64(ent, q, bias, smoothed(y01, li, 0.1))
    check_against_f64(run(fused_fn(li, subj, rel, 0.1), ent, q, bias), ref, "fused, two row chunks")


def int_case(B, N, D, seed):
    """Integer-valued operands (both matrix cores are exact on them) and an integer bias in {-2, ..., 2}.  Query 0 is all 2: against
    entity 5 (all 1) it reaches x = 2 D + bias, against entity 6 (all -1, bias -2) x = -2 D - 2.  From D = 52 on every query ends in
    twenty 2s and entity 7 is 0 but for twenty 1s there: x[:, 7] = 40 + bias[7] > 17, a column whose every cell saturates to p = 1."""
    gen = torch.Generator().manual_seed(seed)
    ent = torch.randint(-1, 2, (N, D), generator=gen).float()
    q = (torch.randint(-1, 2, (B, D), generator=gen) * torch.randint(-1, 3, (B, D), generator=gen)).float()
    bias = torch.randint(-2, 3, (N,), generator=gen).float()
    q[0], ent[5], ent[6], bias[6] = 2.0, 1.0, -1.0, -2.0
    if D >= 52:
        q[:, D - 20:] = 2.0
        ent[7] = 0.0
        ent[7, D - 20:] = 1.0
    return ent.to(DEV), q.to(DEV), bias.to(DEV)


@pytest.mark.parametrize("D", [4, 52, 53, 200])
def test_drop_in_equality_with_the_dense_path_saturation_included(D):
    B, N = 129, 449
    li, subj, rel, y01 = make_index(N, B, seed=7)
    ent, q, bias = int_case(B, N, D, seed=D)
    dense = run(dense_fn(li, subj, rel, 0.1), ent, q, bias)
    fused = run(fused_fn(li, subj, rel, 0.1), ent, q, bias)
    print(f"D={D}: loss fused {float(fused[0]):.9g} dense {float(dense[0]):.9g}; "
          + " ".join(f"{n} {rel_err(g, r):.2e}" for n, g, r in zip(NAMES, fused[1:], dense[1:])))
    assert abs(float(fused[0]) - float(dense[0])) <= 1e-6 * float(dense[0])
    for name, g, r in zip(NAMES, fused[1:], dense[1:]):
        assert rel_err(g, r) <= 1e-5, f"{name}: {rel_err(g, r):.3e}"
    with torch.no_grad():
        p = K.linear(q, ent, bias, "sigmoid")
        sat = (p == 0) | (p == 1)
        if D >= 52:
            assert bool((p == 0).any()) and bool((p == 1).any()) and bool(sat[:, 7].all())
        whole = sat.all(dim=0)
        assert bool((fused[3][whole] == 0).all()) and bool((fused[3][~whole] != 0).any())     # g_bias of a saturated column: exactly 0
        qkey = (subj.long() * (2 * R) + rel.long()).contiguous()
        v0, v1 = li.label_values(0.1)
        one = torch.ones(1, device=DEV)
        dl = K.distmult_bce_dlogit(q, ent, li, qkey, v0, v1, 0, N, one, bias=bias)
        assert dl.shape == (B, N) and bool((dl[sat] == 0).all()) and bool((dl[~sat] != 0).any())
        part = K.distmult_bce_dlogit(q, ent, li, qkey, v0, v1, 224, 449, one, bias=bias)    # a column range is the same numbers
        assert torch.equal(part, dl[:, 224:449])
        plain = K.distmult_bce_dlogit(q, ent, li, qkey, v0, v1, 0, N, one)
        assert not torch.equal(plain, dl)                                                   # the bias is in the logits


def rank_side(li, subj, rel):
    side = EV._LabelSide(li)
    when = torch.full((subj.numel(),), -1, dtype=torch.int32, device=DEV)
    qkey = (subj.long() * side.num_rels + rel.long()).contiguous()
    return side, when, qkey


@pytest.mark.parametrize("D", [4, 50, 52])
def test_a_zero_bias_is_no_bias(D):
    B, N = 129, 449
    li, subj, rel, y01 = make_index(N, B, seed=11)
    ent, q, _ = float_case(B, N, D, seed=D + 1)
    zero = torch.zeros(N, device=DEV)
    got = run(fused_fn(li, subj, rel, 0.1), ent, q, zero)
    with torch.no_grad():
        plain = K.rows_bce_all("dot", None, ent, q, li, subj, rel, 0.1)
        assert torch.equal(got[0], plain)
        qkey = (subj.long() * (2 * R) + rel.long()).contiguous()
        v0, v1 = li.label_values(0.1)
        gscale = torch.full((1,), 3.0 / (B * N), device=DEV)
        colsum = K.distmult_bce_dlogit(q, ent, li, qkey, v0, v1, 0, N, gscale).double().sum(dim=0)
        print(f"D={D}: g_bias vs the unbiased slice's column sums {rel_err(got[3], colsum):.2e}")
        assert rel_err(got[3], colsum) <= 1e-6
        side, when, qk = rank_side(li, subj, rel)
        target = torch.arange(B, device=DEV) % N
        for s in ((None, None, None), (side, when, qk)):
            assert torch.equal(EV.query_ranks(q, ent, target, *s, bias=zero), EV.query_ranks(q, ent, target, *s))
            ids_b, vals_b = EV.query_topk(q, ent, 10, *s, bias=zero)
            ids_p, vals_p = EV.query_topk(q, ent, 10, *s)
            assert torch.equal(ids_b, ids_p) and torch.equal(vals_b, vals_p)


@pytest.mark.parametrize("D", [50, 64])
def test_the_loss_and_the_bias_gradient_are_bitwise_repeatable(D):
    B, N = 257, 449
    li, subj, rel, _ = make_index(N, B, seed=9)
    ent, q, bias = float_case(B, N, D, seed=17)
    a = run(fused_fn(li, subj, rel, 0.1), ent, q, bias)
    b = run(fused_fn(li, subj, rel, 0.1), ent, q, bias)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])


def test_chunking_does_not_matter():
    B, N, D = 129, 449, 52
    li, subj, rel, y01 = make_index(N, B, seed=3)
    ent, q, bias = float_case(B, N, D, seed=11)
    base = run(fused_fn(li, subj, rel, 0.1, None), ent, q, bias)
    for col_chunk in (224, 448, 449):
        got = run(fused_fn(li, subj, rel, 0.1, col_chunk), ent, q, bias)
        assert torch.equal(got[0], base[0])
        for name, g, r in zip(NAMES, got[1:], base[1:]):
            assert rel_err(g, r) <= 1e-6, f"col_chunk {col_chunk} {name}: {rel_err(g, r):.3e}"


def test_the_bias_gradient_is_skipped_when_the_bias_needs_none():
    B, N, D = 33, 225, 52
    li, subj, rel, _ = make_index(N, B, seed=4)
    ent, q, bias = float_case(B, N, D, seed=6)
    e, s = ent.clone().requires_grad_(True), q.clone().requires_grad_(True)
    _lib.meter.start(["mrg_cols_sum", "mrg_rows_bias_bce_dlogit"])
    K.rows_bce_all("dot", None, e, s, li, subj, rel, 0.1, bias=bias).backward()
    got = _lib.meter.stop()
    assert "mrg_cols_sum" not in got and got["mrg_rows_bias_bce_dlogit"]["launches"] == 1


# ---- ranks ------------------------------------------------------------------------------------------------------------------------
def rank_band(q, ent, bias, target, allowed):
    """(lo, hi, exact) [Q] on the CPU: mrr_ref.rank_band on the biased float64 logits, delta = the float32 chain bound of the product
    (3 D 2^-24 max_e sum_c |q_c ent[e, c]|, mrr_ref.delta_q) plus the one rounding of the bias add."""
    q, ent, bias, target = q.double().cpu(), ent.double().cpu(), bias.double().cpu(), target.long().cpu()
    x = q @ ent.t() + bias
    mag = (q.abs() @ ent.abs().t()).max(dim=1).values
    d = (3 * ent.shape[1] * 2.0 ** -24 * mag + 2.0 ** -23 * (mag + float(bias.abs().max()))).unsqueeze(1)
    t = target.unsqueeze(1)
    xt = x.gather(1, t)
    others = allowed & (torch.arange(x.shape[1]).unsqueeze(0) != t)
    return 1 + ((x > xt + d) & others).sum(dim=1), 1 + ((x >= xt - d) & others).sum(dim=1), MR.exact_ranks(x, target, allowed)


RANK_SHAPES = [(1, 449, 52), (127, 33, 64), (129, 224, 200), (257, 225, 52), (129, 1, 64), (1, 225, 4), (127, 449, 50), (129, 33, 4),
               (257, 224, 50), (127, 1, 4)]


@pytest.mark.parametrize("B,N,D", RANK_SHAPES)
def test_ranks_against_float64_raw_and_filtered(B, N, D):
    li, subj, rel, y01 = make_index(N, B, seed=B + N + 1)
    ent, q, bias = float_case(B, N, D, seed=D + 2)
    target = torch.from_numpy(np.random.default_rng(B + D).integers(0, N, B)).to(DEV)
    side, when, qkey = rank_side(li, subj, rel)
    for what, s, allowed in (("raw", (None, None, None), torch.ones(B, N, dtype=torch.bool)), ("filtered", (side, when, qkey), (y01 == 0).cpu())):
        got = EV.query_ranks(q, ent, target, *s, bias=bias).cpu()
        lo, hi, exact = rank_band(q, ent, bias, target, allowed)
        print(f"{what}: {int((got == exact).sum())} of {B} ranks equal the float64 ones, {int((lo == hi).sum())} bands are one rank wide")
        assert got.dtype == torch.int64 and bool(((lo <= got) & (got <= hi)).all()), what
        if N > 1:
            assert int((got == exact).sum()) >= 0.9 * B          # the band is no excuse: nearly every rank is the exact one
    if B >= 127 and N >= 33:                                     # the bias moves ranks: this is not the unbiased sweep
        assert not torch.equal(EV.query_ranks(q, ent, target, bias=bias), EV.query_ranks(q, ent, target))


@pytest.mark.parametrize("D", [50, 64])
def test_a_duplicate_entity_row_ties_wins_or_loses_by_its_bias(D):
    """Entity 250 is a copy of entity 5 (another column block of the sweep).  With equal biases the two tie bit for bit -- the target's
    score is the diagonal accumulator plus bias[target], the add the sweep forms -- and the lower id wins; a larger bias beats the
    target, a smaller one loses.  Moving one entity's bias changes no other comparison, so the ranks differ by exactly that entity."""
    Q, N = 40, 300
    ent, q, bias = float_case(Q, N, D, seed=D + 3)
    ent[250] = ent[5]
    bias[250] = bias[5]
    t5, t250 = (torch.full((Q,), t, device=DEV) for t in (5, 250))

    def ranks(target, who=None, by=0.0):
        b = bias.clone()
        if who is not None:
            b[who] += by
        return EV.query_ranks(q, ent, target, bias=b)

    eq5, eq250 = ranks(t5), ranks(t250)
    assert torch.equal(eq250, eq5 + 1)                             # a tie: entity 5 is in front of 250, 250 is not in front of 5
    assert torch.equal(ranks(t250, 5, 0.5), eq250)                 # the duplicate at the lower id with a larger bias beats the target
    assert torch.equal(ranks(t250, 5, -0.5), eq250 - 1)            # ... with a smaller one it loses
    assert torch.equal(ranks(t5, 250, 0.5), eq5 + 1)               # the duplicate at the higher id with a larger bias beats the target
    assert torch.equal(ranks(t5, 250, -0.5), eq5)                  # ... with a smaller one it loses, as it does in the tie


@pytest.mark.parametrize("D", [4, 52])
def test_with_zero_queries_the_ranks_are_the_ranks_of_the_bias(D):
    Q, N = 130, 449
    gen = torch.Generator().manual_seed(D)
    ent = torch.randn(N, D, generator=gen).to(DEV)
    bias = (torch.randint(-20, 21, (N,), generator=gen).float() / 8).to(DEV)              # many equal values
    target = torch.randint(0, N, (Q,), generator=gen).to(DEV)
    got = EV.query_ranks(torch.zeros(Q, D, device=DEV), ent, target, bias=bias).cpu()
    want = MR.exact_ranks(bias.double().cpu().expand(Q, N), target.cpu(), torch.ones(Q, N, dtype=torch.bool))
    assert torch.equal(got, want) and int(want.max()) > 100


# ---- top-k ------------------------------------------------------------------------------------------------------------------------
def topk_int_case(Q, N, D, seed):
    """Integer operands and a bias of quarters: every logit is exact in float32 on both cores, and many are equal."""
    gen = torch.Generator().manual_seed(seed)
    ent = torch.randint(-1, 2, (N, D), generator=gen).float()
    q = torch.randint(-2, 3, (Q, D), generator=gen).float()
    bias = torch.randint(-8, 9, (N,), generator=gen).float() / 4
    return ent.to(DEV), q.to(DEV), bias.to(DEV)


@pytest.mark.parametrize("Q,N,D,k", [(129, 449, 52, 1), (129, 449, 52, 10), (257, 225, 4, 10), (127, 449, 50, 64), (33, 33, 64, 64),
                                      (5, 28672 + 33, 52, 10), (5, 28672 + 33, 4, 64)])
def test_topk_is_torch_topk_of_the_dense_biased_logits(Q, N, D, k):
    li, subj, rel, y01 = make_index(N, Q, seed=Q + N + 2)
    ent, q, bias = topk_int_case(Q, N, D, seed=D + k)
    side, when, qkey = rank_side(li, subj, rel)
    for what, s, allowed in (("raw", (None, None, None), torch.ones(Q, N, dtype=torch.bool)), ("filtered", (side, when, qkey), (y01 == 0).cpu())):
        ids, vals = EV.query_topk(q, ent, k, *s, bias=bias)
        x64 = q.double().cpu() @ ent.double().cpu().t() + bias.double().cpu()
        want_ids, want_vals = TR.topk64("dot", x64, allowed, k)
        assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), want_ids), what        # ties: the lower id first
        assert torch.equal(vals.double().cpu(), want_vals), what
        dense = K.linear(q, ent, bias, None).masked_fill(~allowed.to(DEV), float("-inf"))   # the dense biased logits, filtered
        m = min(k, N)
        assert torch.equal(vals[:, :m], torch.topk(dense, m, dim=1).values), what
        if what == "filtered":
            assert int((ids[0] >= 0).sum()) == 0                                            # key (0, 0) lists every entity
            assert N >= k + 8 or bool((ids < 0).any())                                      # fewer than k candidates are left
        for j in sorted({0, k // 2, k - 1}):
            have = ids[:, j] >= 0
            ranks = EV.query_ranks(q, ent, ids[:, j].clamp(min=0), *s, bias=bias)
            assert torch.equal(ranks[have], torch.full_like(ranks[have], j + 1)), f"{what} position {j}"


def test_topk_values_are_the_biased_logits_of_float_operands():
    Q, N, D, k = 129, 449, 52, 10
    ent, q, bias = float_case(Q, N, D, seed=31)
    ids, vals = EV.query_topk(q, ent, k, bias=bias)
    x64 = q.double() @ ent.double().t() + bias.double()
    assert rel_err(vals, x64.gather(1, ids)) <= 1e-4
    for j in range(k):
        assert torch.equal(EV.query_ranks(q, ent, ids[:, j], bias=bias), torch.full((Q,), j + 1, device=DEV))


# ---- CompGCN_ConvE on the fixture whose labels come from triples -----------------------------------------------------------------
def compgcn_case(z):
    g = G.RelGraph(z["N"], z["src"], z["dst"], z["etype"], z["norm"], device=DEV)
    m = z["in_edges_mask"].to(DEV)
    g.edata["etype"], g.edata["in_edges_mask"], g.edata["out_edges_mask"] = z["etype"].to(DEV), m, ~m
    g.edata["norm"] = z["norm"].to(DEV)
    net = CG.CompGCN_ConvE(z["nb"], 2 * z["R"], z["N"], z["Din"], [z["Dout"]], comp_fn="sub", dropout=0.0, layer_dropout=[0.0],
                           num_filt=z["F"], hid_drop=0.0, feat_drop=0.0, ker_sz=z["ks"], k_w=z["k_w"], k_h=z["k_h"])
    net.load_state_dict(sub(z, "param0/"))
    li = LabelIndex(z["triples"].numpy(), z["R"], z["N"], DEV)
    return g, net.to(DEV), li, z["subj"].to(DEV), z["rel"].to(DEV)


@pytest.fixture(scope="module")
def fixture_1n():
    return load_golden("compgcn_conve_1n")


def test_compgcn_conve_loss_1n_matches_the_reference(fixture_1n):
    z = fixture_1n
    g, net, li, subj, rel = compgcn_case(z)
    ls = float(z["label_smooth"])
    assert torch.equal(li.labels(subj, rel, ls).cpu(), z["label"])            # LabelIndex rebuilds the reference's smoothed labels
    net.train()
    loss = net.loss_1n(g, subj, rel, li, ls)
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), z["loss"], rtol=1e-4, atol=1e-6)
    assert sorted(n for n, _ in net.named_parameters()) == sorted(sub(z, "gparam/"))
    for n, p in net.named_parameters():
        assert_param_grad(z, n, p.grad, 5e-4, 5e-6, "compgcn_conve_1n")
    assert float(z["gparam/bias"].abs().max()) > 0 and net.bias.grad is not None
    bufs = dict(net.named_buffers())
    for n, ref in sub(z, "buffer/").items():
        torch.testing.assert_close(bufs[n].cpu(), ref, rtol=1e-4, atol=1e-5)


def test_compgcn_conve_loss_1n_is_its_own_dense_loss(fixture_1n):
    z = fixture_1n
    g, net, li, subj, rel = compgcn_case(z)
    other = copy.deepcopy(net)
    net.train()
    other.train()
    loss_f = net.loss_1n(g, subj, rel, li, 0.1)
    loss_f.backward()
    loss_d = F.binary_cross_entropy(other(g, subj, rel), li.labels(subj, rel, 0.1))
    loss_d.backward()
    torch.cuda.synchronize()
    loss_f, loss_d = float(loss_f.detach()), float(loss_d.detach())
    print(f"loss fused {loss_f:.9g} dense {loss_d:.9g}")
    assert abs(loss_f - loss_d) <= 1e-6 * loss_d
    # 1e-5 of the dense gradient's largest entry per parameter.  The parameters in front of a BatchNorm (bn0, fc.bias, W_S.bias,
    # loop_rel) have gradients that are mathematically zero -- 1e-7 of rounding noise in either path -- hence the absolute 1e-6, a fifth
    # of what assert_param_grad allows against the reference.
    ref, seen = dict(other.named_parameters()), 0
    for k, p in net.named_parameters():
        assert (p.grad is None) == (ref[k].grad is None), k
        if p.grad is not None:
            want = ref[k].grad
            err, top = float((p.grad - want).abs().max()), float(want.abs().max())
            print(f"  {k}: max abs error {err:.2e} (max abs dense {top:.2e})")
            assert err <= 1e-5 * top + 1e-6, f"{k}: {err:.3e} against {top:.3e}"
            seen += top > 1e-3
    assert net.bias.grad is not None and float(other.bias.grad.abs().max()) > 1e-3 and seen >= 15
    for (n, a), (_, b) in zip(net.named_buffers(), other.named_buffers()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7, msg=n)


def expected_eval(z):
    """(filtered ranks [B], unsmoothed 0 / 1 labels [B, N]) from the reference's eval-mode predictions: mrg_rank_filtered's rule."""
    y01 = (z["label"] > 0.5)
    t = z["eval_obj"].long()
    allowed = ~y01
    return MR.exact_ranks(z["pred_eval"].double(), t, allowed), y01


def test_predict_1n_and_predict_topk_take_the_model_unchanged(fixture_1n):
    z = fixture_1n
    g, net, li, subj, rel = compgcn_case(z)
    net.train()
    net.loss_1n(g, subj, rel, li, 0.1)                              # the training step whose running statistics pred_eval read
    want, y01 = expected_eval(z)
    assert bool((y01.gather(1, z["eval_obj"].long().unsqueeze(1)) == 1).all()) and int(want.max()) > 1
    triplets = torch.stack((z["subj"], z["rel"], z["eval_obj"]), dim=1).long()
    res, loss = EV.predict_1n([triplets[:4], triplets[4:]], g, net, li, DEV)
    wd = want.double()
    assert res["count"] == want.numel() and res["mr"] == float(wd.sum()) and abs(res["mrr"] - float(wd.reciprocal().sum())) <= 1e-12
    assert all(res[f"hits@{k}"] == int((want <= k).sum()) for k in (1, 3, 10))
    loader = [(t, li.labels(t[:, 0].to(DEV), t[:, 1].to(DEV)).cpu()) for t in (triplets[:4], triplets[4:])]
    res_d, loss_d = EV.predict(loader, g, net, DEV)
    print(f"predict {res_d} {loss_d:.9g}; predict_1n {res} {loss:.9g}")
    assert res == res_d and abs(loss - loss_d) <= 1e-6 * loss_d
    ref_loss = sum(float(F.binary_cross_entropy(z["pred_eval"][a:b], y01[a:b].float())) for a, b in ((0, 4), (4, 7)))
    assert abs(loss - ref_loss) <= 1e-4 * ref_loss
    k = 10
    for label_index, pe in ((None, z["pred_eval"]), (li, z["pred_eval"].masked_fill(y01, -1.0))):
        ids, prob = EV.predict_topk(net, g, subj, rel, k, label_index)
        tv, ti = torch.topk(pe, k, dim=1)
        assert torch.equal(ids.cpu(), ti)
        torch.testing.assert_close(prob.cpu(), tv, rtol=1e-4, atol=5e-5)


def test_loss_1n_launches_the_biased_sweep_and_no_batch_by_entity_product(fixture_1n, monkeypatch):
    z = fixture_1n
    g, net, li, subj, rel = compgcn_case(z)
    net.train()
    _lib.load()
    real, widths = _lib._FN.get("mrg_linear_fwd") or _lib.load().mrg_linear_fwd, []

    def probe(*args):
        widths.append(int(args[7]))                                 # Nout of mrg_linear_fwd(X, W, bias, Y, ws, rows, K, Nout, act, stream)
        return real(*args)

    monkeypatch.setitem(_lib._FN, "mrg_linear_fwd", probe)
    _lib.meter.start(["mrg_rows_bias_bce_fwd", "mrg_distmult_bce_fwd"])
    loss = net.loss_1n(g, subj, rel, li, 0.1)
    got = _lib.meter.stop()
    assert got["mrg_rows_bias_bce_fwd"]["launches"] == 1 and "mrg_distmult_bce_fwd" not in got
    assert widths and z["N"] not in widths, widths                  # the layers' Linears ran, the [B, N] product did not
    del widths[:]
    with torch.no_grad():
        net(g, subj, rel)
    assert z["N"] in widths                                         # the dense forward is what launches it
    assert loss.dim() == 0


def test_peak_memory_stays_far_below_a_batch_by_entity_matrix():
    """Peak allocation of forward + backward beyond what was there before and the gradients left behind: fused at most half a [B, N]
    float matrix, the dense biased path at least two."""
    B, N, D, col_chunk = 1024, 20000, 52, 2048
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, 3 * N), rng.integers(0, R, 3 * N), rng.integers(0, N, 3 * N)], 1)
    li = LabelIndex(tri, R, N, DEV)
    subj, rel = torch.from_numpy(tri[:B, 0]).to(DEV), torch.from_numpy(tri[:B, 1]).to(DEV)
    gen = torch.Generator().manual_seed(0)
    ent, q = ((0.3 * torch.randn(n, D, generator=gen)).to(DEV) for n in (N, B))
    bias = (2.0 * torch.rand(N, generator=gen) - 1.0).to(DEV)
    matrix = B * N * 4

    def extra(fn):
        e, s, b = (t.detach().clone().requires_grad_(True) for t in (ent, q, bias))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn(e, s, b)
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        return peak - before - sum(t.grad.numel() * 4 for t in (e, s, b)), float(loss.detach())

    fused, lf = extra(fused_fn(li, subj, rel, 0.1, col_chunk))
    dense, ld = extra(dense_fn(li, subj, rel, 0.1))
    print(f"peak beyond inputs and gradients: fused {fused / 2 ** 20:.1f} MiB, dense {dense / 2 ** 20:.1f} MiB, [B, N] {matrix / 2 ** 20:.1f} MiB")
    assert abs(lf - ld) <= 1e-4 * max(1.0, ld)
    assert fused <= 0.5 * matrix
    assert dense >= 2 * matrix


def test_graph_capture_replays_the_eager_loss_1n_step(fixture_1n):
    """One loss_1n training step captured once and replayed once equals the eager step: nothing in it synchronises with the host."""
    z = fixture_1n
    g, net_e, li, subj, rel = compgcn_case(z)
    net_g, warm = copy.deepcopy(net_e), copy.deepcopy(net_e)

    def step(net):
        net.train()
        loss = net.loss_1n(g, subj, rel, li, 0.1)
        return [loss.detach()] + list(torch.autograd.grad(loss, list(net.parameters())))       # (every parameter takes part)

    eager = step(net_e)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(warm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(net_g)
    graph.replay()
    torch.cuda.synchronize()
    assert len(eager) == len(outs) and float(eager[0]) > 0
    for a, b in zip(eager, outs):
        torch.testing.assert_close(b, a, rtol=0, atol=0)
    for (n, a), (_, b) in zip(net_e.named_buffers(), net_g.named_buffers()):
        if a.is_floating_point():
            torch.testing.assert_close(b, a, rtol=0, atol=0, msg=n)
