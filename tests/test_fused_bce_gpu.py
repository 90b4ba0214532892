"""The 1-N DistMult loss and evaluation without [B, N] tensors on the device: csrc/bce.hip (EPI_BCE / EPI_BCE_GRAD on both matrix
cores), functional.distmult_bce_all, FixedNetwork.loss_fused and evaluation.predict_fused against float64 and against the dense
device path (LabelIndex.labels + distmult_scores_all + F.binary_cross_entropy)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mr_gnas_amd import _lib, evaluation as EV, functional as K, graph as G, supernet as S
from mr_gnas_amd.sampler import LabelIndex

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 3

README_GENOTYPE = [S.Genotype(alpha_cell=[('pre_sub', 1, 0), ('f_sparse_comp', 2, 1), ('f_sparse_comp', 3, 2), ('a_max', 4, 2),
                                          ('a_max', 5, 3), ('f_sparse_last', 6, 5), ('f_sparse_last', 7, 5)],
                              concat_node=[4, 5, 6, 7], score_func='sf_DisMult')]


def rel_err(got, ref):
    """max abs error over max abs reference (no floor at 1: the gradients of a mean over B * N elements are small)."""
    ref = ref.double()
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def make_index(N, B, seed):
    """Triples over relations [0, R - 1) only, so that every key (s, R - 1) is unknown; key (0, 0) lists every entity; key (1, 0)
    lists entities 223 and 224 where they exist.  The batch: row 0 = (0, 0), row 1 = (1, 0), row 2 = an unknown key, row 3 = row 0
    again (two identical rows), the rest random over all 2R relations.  Returns the index, subj, rel and the dense 0 / 1 labels built
    from the triples on the host."""
    rng = np.random.default_rng(seed)
    T = 3 * N
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, max(R - 1, 1), T), rng.integers(0, N, T)], 1)
    extra = [(0, 0, o) for o in range(N)] + [(min(1, N - 1), 0, o) for o in (223, 224) if o < N]
    tri = np.concatenate([tri, np.asarray(extra, dtype=tri.dtype)])
    subj, rel = rng.integers(0, N, B), rng.integers(0, 2 * R, B)
    fixed = [(0, 0), (min(1, N - 1), 0), (int(rng.integers(0, N)), R - 1), (0, 0)]
    for i, (s, r) in enumerate(fixed[:B]):
        subj[i], rel[i] = s, r
    sr2o = {}
    for s, r, o in tri.tolist():
        sr2o.setdefault((s, r), set()).add(o)
        sr2o.setdefault((o, r + R), set()).add(s)
    y = np.zeros((B, N), dtype=np.float64)
    for i in range(B):
        y[i, sorted(sr2o.get((int(subj[i]), int(rel[i])), ()))] = 1.0
    li = LabelIndex(tri, R, N, DEV)
    return li, torch.from_numpy(subj).to(DEV), torch.from_numpy(rel).to(DEV), torch.from_numpy(y).to(DEV)


def smoothed(y01, li, label_smooth):
    v0, v1 = li.label_values(label_smooth)
    return y01 * (v1 - v0) + v0


def float_case(B, N, D, seed):
    """Random float operands with float64 max |x| <= 7 (the relation rows are scaled down where the draw exceeds it)."""
    gen = torch.Generator().manual_seed(seed)
    scale = 0.5 if D <= 4 else (0.3 if D <= 64 else 0.15)
    ent = (scale * torch.randn(N, D, generator=gen)).to(DEV)
    sub = (scale * torch.randn(B, D, generator=gen)).to(DEV)
    relb = torch.randn(B, D, generator=gen).to(DEV)
    x = (sub.double() * relb.double()) @ ent.double().t()
    relb = (relb * min(1.0, 7.0 / float(x.abs().max()))).contiguous()
    return ent, sub, relb


def loss64(ent, sub, relb, y):
    """The float64 formula on float64 logits: (loss, g_ent, g_sub, g_rel) of 3 * loss."""
    e, s, r = (t.detach().double().requires_grad_(True) for t in (ent, sub, relb))
    x = (s * r) @ e.t()
    assert float(x.detach().abs().max()) <= 8.0
    loss = -(y * F.logsigmoid(x) + (1.0 - y) * F.logsigmoid(-x)).mean()
    (3 * loss).backward()
    return loss.detach(), e.grad, s.grad, r.grad


def run(fn, ent, sub, relb, upstream=3.0):
    e, s, r = (t.detach().clone().requires_grad_(True) for t in (ent, sub, relb))
    loss = fn(e, s, r)
    (upstream * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), e.grad, s.grad, r.grad


def dense_fn(li, subj, rel, label_smooth):
    return lambda e, s, r: F.binary_cross_entropy(K.distmult_scores_all(e, s, r), li.labels(subj, rel, label_smooth))


def fused_fn(li, subj, rel, label_smooth, col_chunk=None):
    return lambda e, s, r: K.distmult_bce_all(e, s, r, li, subj, rel, label_smooth, col_chunk)


def check_against_f64(got, ref, what):
    assert got[0].dtype == torch.float32 and got[0].dim() == 0
    l64 = float(ref[0])
    print(f"{what}: loss {float(got[0]):.9g} vs {l64:.9g}; rel_err g_ent {rel_err(got[1], ref[1]):.2e} g_sub {rel_err(got[2], ref[2]):.2e} "
          f"g_rel {rel_err(got[3], ref[3]):.2e}")
    assert abs(float(got[0]) - l64) <= 1e-4 * max(1.0, l64), what
    for name, g, r in zip(("g_ent", "g_sub", "g_rel"), got[1:], ref[1:]):
        assert rel_err(g, r) <= 1e-4, f"{what} {name}: {rel_err(g, r):.3e}"


# every B of {1, 127, 129, 257} and every N of {1, 33, 224, 225, 449} with the split core (D = 52, 64, 200) and with the exact core
# (D = 4: vectorised loads, D = 50: plain loads); N = 28 672 + 33 sweeps a second column block (csrc/sweep_host.hpp: BCE_COLS) on each
# core, so the partials of two launches are added
SHAPES = [(1, 449, 52), (127, 33, 64), (129, 224, 200), (257, 225, 52), (129, 1, 64), (127, 449, 200),
          (1, 225, 4), (127, 449, 50), (129, 33, 4), (257, 224, 50), (127, 1, 4), (5, 28672 + 33, 4), (5, 28672 + 33, 52)]


# label smoothing 0.1 leaves labels in [0, 1] from N = 10 on (0.9 y + 1 / N: at N = 1 the labels are 1.0 and 1.9, which
# torch's binary_cross_entropy, the dense path's loss, rejects by a device-side assertion): N = 1 runs unsmoothed only
CASES = [(B, N, D, ls) for B, N, D in SHAPES for ls in (0.0, 0.1) if ls == 0.0 or N >= 10]


@pytest.mark.parametrize("B,N,D,label_smooth", CASES)
def test_float64_accuracy_without_saturation(B, N, D, label_smooth):
    li, subj, rel, y01 = make_index(N, B, seed=B + N)
    if B >= 4:
        assert bool((y01[0] == 1).all()) and float(y01[2].sum()) == 0 and torch.equal(y01[0], y01[3])
        assert N <= 224 or (float(y01[1, 223]) == 1 and float(y01[1, 224]) == 1)
    assert torch.equal(li.labels(subj, rel, label_smooth).double(), smoothed(y01, li, label_smooth).float().double())
    ent, sub, relb = float_case(B, N, D, seed=D)
    ref = loss64(ent, sub, relb, smoothed(y01, li, label_smooth))
    check_against_f64(run(dense_fn(li, subj, rel, label_smooth), ent, sub, relb), ref, "dense")       # the inputs are fair
    check_against_f64(run(fused_fn(li, subj, rel, label_smooth), ent, sub, relb), ref, "fused")


def int_case(B, N, D, seed):
    """Integer-valued operands (both matrix cores are exact on them); query 0 against entities 5 / 6 reaches x = +2D / -2D."""
    gen = torch.Generator().manual_seed(seed)
    ent = torch.randint(-1, 2, (N, D), generator=gen).float()
    sub = torch.randint(-1, 2, (B, D), generator=gen).float()
    relb = torch.randint(-1, 3, (B, D), generator=gen).float()
    sub[0], relb[0], ent[5], ent[6] = 1.0, 2.0, 1.0, -1.0
    return ent.to(DEV), sub.to(DEV), relb.to(DEV)


@pytest.mark.parametrize("D", [4, 52, 53, 200])
def test_drop_in_equality_with_the_dense_path_saturation_included(D):
    """Loss and gradients against the dense device path on data where float32 sigmoid saturates to exactly 0 and 1, and the logit
    gradient is exactly 0 wherever the dense path's p is.  D = 4 cannot reach the thresholds with entries in {-1, 0, 1} x
    {-1, 0, 1, 2} (|x| <= 8): it runs the same comparison on the exact core's vectorised loads and asserts its own extremes;
    D = 53 (|x| up to 106) brings the saturated cells to the exact core."""
    B, N = 129, 449
    li, subj, rel, y01 = make_index(N, B, seed=7)
    ent, sub, relb = int_case(B, N, D, seed=D)
    x = (sub.double() * relb.double()) @ ent.double().t()
    if D >= 52:
        assert float(x.max()) >= 17 and float(x.min()) <= -104
    else:
        assert float(x.max()) == 2 * D and float(x.min()) == -2 * D
    dense = run(dense_fn(li, subj, rel, 0.1), ent, sub, relb)
    fused = run(fused_fn(li, subj, rel, 0.1), ent, sub, relb)
    print(f"D={D}: loss fused {float(fused[0]):.9g} dense {float(dense[0]):.9g}; "
          + " ".join(f"{n} {rel_err(g, r):.2e}" for n, g, r in zip(("g_ent", "g_sub", "g_rel"), fused[1:], dense[1:])))
    assert abs(float(fused[0]) - float(dense[0])) <= 1e-6 * float(dense[0])
    for name, g, r in zip(("g_ent", "g_sub", "g_rel"), fused[1:], dense[1:]):
        assert rel_err(g, r) <= 1e-5, f"{name}: {rel_err(g, r):.3e}"
    with torch.no_grad():
        p = K.distmult_scores_all(ent, sub, relb)
        sat = (p == 0) | (p == 1)
        if D >= 52:
            assert bool((p == 0).any()) and bool((p == 1).any())
            assert float(smoothed(y01, li, 0.1)[p == 0].max()) > 0.5              # a cell that costs 100 y
        q = (sub * relb).contiguous()
        qkey = (subj.long() * (2 * R) + rel.long()).contiguous()
        v0, v1 = li.label_values(0.1)
        one = torch.ones(1, device=DEV)
        dl = K.distmult_bce_dlogit(q, ent, li, qkey, v0, v1, 0, N, one)
        assert dl.shape == (B, N) and bool((dl[sat] == 0).all()) and bool((dl[~sat] != 0).any())
        part = K.distmult_bce_dlogit(q, ent, li, qkey, v0, v1, 224, 449, one)       # a column range is the same numbers
        assert torch.equal(part, dl[:, 224:449])


def test_chunking_does_not_matter():
    B, N, D = 129, 449, 52
    li, subj, rel, y01 = make_index(N, B, seed=3)
    ent, sub, relb = float_case(B, N, D, seed=11)
    base = run(fused_fn(li, subj, rel, 0.1, None), ent, sub, relb)
    for col_chunk in (224, 448, 449):
        got = run(fused_fn(li, subj, rel, 0.1, col_chunk), ent, sub, relb)
        assert torch.equal(got[0], base[0])
        for name, g, r in zip(("g_ent", "g_sub", "g_rel"), got[1:], base[1:]):
            assert rel_err(g, r) <= 1e-6, f"col_chunk {col_chunk} {name}: {rel_err(g, r):.3e}"


@pytest.mark.parametrize("B,N,D,col_chunk", [(128, 1250, 52, None), (132, 2300, 52, 1150), (129, 1250, 52, None), (132, 1250, 50, None),
                                             (132, 1250, 52, 1024)])
def test_wide_chunks_and_their_threshold(B, N, D, col_chunk):
    """A chunk of more than 1024 columns forms the query gradient from the transposed slice (B <= 128, or B and D multiples of 4: the
    first two cases, the second with two such chunks adding up); one column fewer, another B or another D keeps the row GEMM."""
    li, subj, rel, y01 = make_index(N, B, seed=21)
    ent, sub, relb = float_case(B, N, D, seed=23)
    ref = loss64(ent, sub, relb, smoothed(y01, li, 0.1))
    check_against_f64(run(fused_fn(li, subj, rel, 0.1, col_chunk), ent, sub, relb), ref, f"fused, col_chunk {col_chunk}")


def test_a_batch_that_crosses_a_row_chunk():
    B, N, D = 8192 + 5, 33, 4
    li, subj, rel, y01 = make_index(N, B, seed=5)
    ent, sub, relb = float_case(B, N, D, seed=13)
    ref = loss64(ent, sub, relb, smoothed(y01, li, 0.1))
    check_against_f64(run(fused_fn(li, subj, rel, 0.1), ent, sub, relb), ref, "fused, two row chunks")


@pytest.mark.parametrize("D", [50, 64])
def test_the_loss_is_bitwise_repeatable(D):
    B, N = 257, 449
    li, subj, rel, _ = make_index(N, B, seed=9)
    ent, sub, relb = float_case(B, N, D, seed=17)
    with torch.no_grad():
        a = fused_fn(li, subj, rel, 0.1)(ent, sub, relb)
        b = fused_fn(li, subj, rel, 0.1)(ent, sub, relb)
    assert torch.equal(a, b)


def test_peak_memory_stays_far_below_a_batch_by_entity_matrix():
    """Peak allocation of forward + backward beyond what was there before and the gradients left behind: fused at most half a [B, N]
    float matrix (the dl slice, the split of the entity rows, the gradient GEMMs' workspaces), dense at least two."""
    B, N, D, col_chunk = 1024, 20000, 52, 2048
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, 3 * N), rng.integers(0, R, 3 * N), rng.integers(0, N, 3 * N)], 1)
    li = LabelIndex(tri, R, N, DEV)
    subj, rel = torch.from_numpy(tri[:B, 0]).to(DEV), torch.from_numpy(tri[:B, 1]).to(DEV)
    gen = torch.Generator().manual_seed(0)
    ent, sub, relb = ((0.3 * torch.randn(n, D, generator=gen)).to(DEV) for n in (N, B, B))
    matrix = B * N * 4

    def extra(fn):
        e, s, r = (t.detach().clone().requires_grad_(True) for t in (ent, sub, relb))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn(e, s, r)
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        return peak - before - sum(t.grad.numel() * 4 for t in (e, s, r)), float(loss.detach())

    fused, lf = extra(fused_fn(li, subj, rel, 0.1, col_chunk))
    dense, ld = extra(dense_fn(li, subj, rel, 0.1))
    print(f"peak beyond inputs and gradients: fused {fused / 2 ** 20:.1f} MiB, dense {dense / 2 ** 20:.1f} MiB, [B, N] {matrix / 2 ** 20:.1f} MiB")
    assert abs(lf - ld) <= 1e-4 * max(1.0, ld)
    assert fused <= 0.5 * matrix
    assert dense >= 2 * matrix


def tiny_graph():
    N, T, Rg, D = 200, 1500, 7, 64
    rng = np.random.default_rng(0)
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, Rg, T), rng.integers(0, N, T)], 1)
    return N, Rg, D, tri, G.build_train_graph(N, Rg, tri).to(DEV)


def test_fixed_network_loss_fused_matches_loss_on_dense_labels():
    N, Rg, D, tri, g = tiny_graph()
    B = 96
    li = LabelIndex(tri, Rg, N, DEV)
    subj = torch.from_numpy(np.concatenate([tri[:B // 2, 0], tri[:B // 2, 2]])).to(DEV)
    rel = torch.from_numpy(np.concatenate([tri[:B // 2, 1], tri[:B // 2, 1] + Rg])).to(DEV)
    torch.manual_seed(1)
    net = S.FixedNetwork(DEV, README_GENOTYPE, N, Rg, D, D, 5, dropout_cell=0.0, drop_aggr=0.0).to(DEV)
    S.xavier_init_(net)
    with torch.no_grad():
        net.rel_wt.mul_(0.05)                                  # moderate logits: no saturation (tests/test_configs_gpu.py, C1)
    net.train()
    loss_d = net._loss(g, subj, rel, li.labels(subj, rel, 0.1))
    loss_d.backward()
    ref = {k: (p.grad.clone() if p.grad is not None else None) for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    loss_f = net.loss_fused(g, subj, rel, li, 0.1)
    loss_f.backward()
    torch.cuda.synchronize()
    loss_f, loss_d = float(loss_f.detach()), float(loss_d.detach())
    print(f"loss fused {loss_f:.9g} dense {loss_d:.9g}")
    assert abs(loss_f - loss_d) <= 1e-4 * max(1.0, loss_d)
    # The operator bound, max abs error over max abs reference, per MODULE: a module's parameters are the columns of one augmented
    # weight ([W | b] acting on [x ; 1]) and their gradients one operator output.  Alone, a bias in front of a BatchNorm has a
    # gradient that is mathematically zero (1e-10 of rounding noise in either path, against 1e-5 in its weight's gradient): there
    # is no reference magnitude to be relative to.
    groups = {}
    for k, p in net.named_parameters():
        assert (p.grad is None) == (ref[k] is None), k
        if p.grad is not None:
            groups.setdefault(k.rsplit(".", 1)[0], []).append((p.grad.reshape(-1), ref[k].reshape(-1)))
    for k, parts in groups.items():
        got, want = torch.cat([a for a, _ in parts]), torch.cat([b for _, b in parts])
        print(f"  {k}: rel_err {rel_err(got, want):.2e} (max abs reference {float(want.abs().max()):.2e})")
        assert float(want.abs().max()) > 0 and rel_err(got, want) <= 1e-4, f"{k}: {rel_err(got, want):.3e}"
    assert len(groups) >= 6
    transe = [README_GENOTYPE[0]._replace(score_func='sf_TransE')]
    other = S.FixedNetwork(DEV, transe, N, Rg, D, D, 5).to(DEV)
    with pytest.raises(_lib.MrgnasError, match="sf_TransE"):
        other.loss_fused(g, subj, rel, li)


class IntegerNet(S.FixedNetwork):
    """The tiny network with prepared integer-valued embeddings after the cells: |x| <= 16, where float32 sigmoid is injective."""

    def embed(self, g):
        return self.int_ent, self.int_rel


def test_predict_fused_matches_predict():
    N, Rg, D, tri, g = tiny_graph()
    li = LabelIndex(tri, Rg, N, DEV)
    net = IntegerNet(DEV, README_GENOTYPE, N, Rg, D, D, 5).to(DEV)
    gen = torch.Generator().manual_seed(2)
    net.int_ent = torch.zeros(N, D)
    net.int_ent[:, :16] = torch.randint(-1, 2, (N, 16), generator=gen).float()
    net.int_ent = net.int_ent.to(DEV)
    net.int_rel = torch.randint(-1, 2, (2 * Rg + 1, D), generator=gen).float().to(DEV)
    test = torch.from_numpy(np.concatenate([tri[:150], np.stack([tri[:150, 2], tri[:150, 1] + Rg, tri[:150, 0]], 1)]))
    x = (net.int_ent[test[:, 0].to(DEV)] * net.int_rel[test[:, 1].to(DEV)]) @ net.int_ent.t()
    assert float(x.abs().max()) <= 16
    bs = 64
    batches = [test[i:i + bs] for i in range(0, test.shape[0], bs)]
    loader = [(t, li.labels(t[:, 0].to(DEV), t[:, 1].to(DEV)).cpu()) for t in batches]
    res_d, loss_d = EV.predict(loader, g, net, DEV)
    res_f, loss_f = EV.predict_fused(loader, g, net, li, DEV)
    res_t, loss_t = EV.predict_fused(batches, g, net, li, DEV)                 # triplets alone
    print(f"predict {res_d} {loss_d:.9g}; predict_fused {res_f} {loss_f:.9g}")
    assert res_d["count"] == test.shape[0] and res_d["mr"] > res_d["count"]   # not everything ranks first
    assert res_f == res_d and res_t == res_d
    assert abs(loss_f - loss_d) <= 1e-6 * loss_d and loss_t == loss_f
