"""No HIP path may depend on what its output and workspace memory held before the call.

Every autograd Function of mr_gnas_amd.functional takes its outputs and workspaces from torch.empty / empty_like / new_empty /
_base._ws, uninitialised.  Several are right only because one kernel writes exactly the elements a later kernel reads: `part` of the
fused a_mean ("only the head rows are written / read"), the chunk reducers' slot partials, split-K partials, per-workgroup column-sum
blocks, capacity-sized launches over plans padded with -1, the running lists of the top-k and rank sweeps, the MixedOp tables.  A
test process starts on freshly mapped, zeroed device memory -- the one content under which a forgotten initialisation or an
unwritten slot comes out right -- and two runs in the same memory state agree with each other.  So every case here runs its
operation, forward and backward, FOUR times under tests/poison.py: allocations zero-filled ("clean"), zero-filled again, filled with
NaN / 0xFF bytes ("nan"), filled with 3e38 / 1e306 / 0x7F bytes ("huge"), and asserts in this order

  1. clean equals clean bit for bit (else "not reproducible, poison comparison void");
  2. every poisoned result is finite where the clean one is;
  3. every poisoned result equals the clean one bit for bit (torch.equal).

No tolerance anywhere: the reference of each comparison is the same code on the same inputs.  Results are every public output: the
outputs, all input and parameter gradients, BatchNorm running statistics, producer column sums, integer outputs (ranks, top-k ids).
Every run is bracketed with _lib.meter: the entry points the case means to test completed a call, no entry point returned an error
(the package has no torch fall-back: an entry point that refuses raises), and the harness filled at least one tensor.

Cases dropped for irreproducibility: none.  One case does not run as shipped: test_nc_network_step.  Its first clean pair differed in
the last bits of the gradient of rel_wt (26 of 30 elements, 3e-7 relative: the first tensor compared; embedding_e and
embedding_e_init receive the same gradient) -- what lies behind `torch.index_select(rel_feat, 0, block.edata[ETYPE])` of
model_nc.Network._forward.  That gather, and the gather of the previous block's node rows, are torch's: their backward is index_add_,
which on the device adds the gradient rows with float atomics in whatever order they arrive.  No kernel of this library is involved
(its own gather, functional.gather, sums in list order).  The case therefore runs under
torch.use_deterministic_algorithms(True, warn_only=True), which gives index_add_ an ordered implementation, and then its clean pair
is equal; every comparison stays bit for bit.  Making the NC networks gather through functional.gather is left for its own change
(it builds a plan per gather per block and wants its own measurement).

Byte workspaces that carry integers (read in csrc/ before the first GPU run; a poisoned byte reads as -1 or 0x7F7F7F7F):
  * mrg_seg_reduce_workspace_bytes (reducers._seg_fwd / _heads_fwd, gcs.fused_gcs): [slots + 1][D] float partials, then the same
    count of int32 arg-max edge ids `ws_arg` (a_max only).  seg_chunk_k stores a slot's pair, seg_hub_k loads the slots
    [hub_first, hub_first + hub_count) of its hub and keeps the id of the larger value; the id ends in `arg` [N, D], which
    seg_bwd_k and segmax_bwd_gx_k only COMPARE with the edge id (a4.x == r).  Never an address.  Poisoned.
  * mrg_linear_relu_segmax_workspace_bytes (fused a_max): [N][Nout] 64-bit keys (float bits << 32 | 0xFFFFFFFF - list position),
    then the split weight.  mrg_linear_relu_segmax_fwd clears the keys with hipMemsetAsync before the GEMM; segmax_finalize_k reads
    eid[0xFFFFFFFF - lo] only where lo != 0, i.e. where the epilogue wrote.  An index, but written (memset) in the same call over the
    whole range that is read.  Poisoned.
  * mrg_distmult_bce / mrg_transe_bce / mrg_sfmix_bce / mrg_sfmix3_bce workspaces: `qlist` [B][2] int32 = begin and end of the
    query's object list, READ AS INDICES into `objs` by the sweeps (gemm_bce_label_words, l1 / mix sweep prologue).  bce_prep_k writes
    every row i < B in the same call before the sweep; every reader guards `row < rows`.  The rest is float64 partials, one per
    workgroup of the walk that both the plan and the launches take from SweepGrid.  Poisoned.
  * mrg_distmult_rank / mrg_transe_rank / mrg_sfmix_rank / mrg_sfmix3_rank workspaces: `qinfo` [Q][4] int32 = target entity, begin,
    end, when: the target indexes `ent` / `bias` (l1_target_k, mix_target_k, rank_bias_tscore_k, all `i < Q`), begin / end index
    `members` / `gone_at`; `counts` [Q] unsigned.  rank_prep_k writes qinfo[i] and counts[i] = 0 for every i < Q first; the sweeps
    clamp a row beyond the launch to rows - 1 or return.  Poisoned.
  * mrg_rows_topk / mrg_transe_topk workspaces: the same qinfo (target -1, never an index), written by topk_prep_k with the running
    lists ids / vals (outputs); `part` [rows][tiles][k] {float value, int id} pairs: topk_select stores a tile list up to and including
    its first padding pair, topk_merge_k stops a list at its first id < 0, so nothing behind the padding is read; ids are compared and
    returned, never an address.  Poisoned.
  * every other workspace reached here holds float or double only: mrg_gemm / mrg_linear_bwd_input[3][_pair] / mrg_dense_filter3
    (the split bf16 planes of a weight), mrg_linear_bwd_weight[3] (per-row-block partial tiles), mrg_gate_bwd, mrg_mix, mrg_zero,
    mrg_seg_std (float64 sums), mrg_conve_fc / mrg_conve_bwd (split-K partials, float64 slabs), the column-sum blocks of the gates,
    dense filters and candidate Linears (float64); mrg_cand_linear_workspace_bytes is 0.
  * not poisoned (poison.SKIP_BYTES_DEFAULT): the workspaces of graph.py and sampler.py, the temporary storage of integer sorts and
    scans whose content is addresses by construction; their builders are pinned bit-exactly against CPU formulations elsewhere.
    Plans are built in the first clean run and cached, so the poisoned runs do not build any."""
import numpy as np
import pytest
import torch

import gcs_ref as GR
import rowgeom_ref as R
from conftest import load_golden, seeded
from poison import SKIP_BYTES_DEFAULT, poisoned

from mr_gnas_amd import _lib, evaluation as EV, functional as K, graph as G, supernet as S, synth
from mr_gnas_amd.sampler import LabelIndex

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 1031                                   # rows: ragged against every rows-per-block of the row-streaming kernels
WIDTHS = (64, 200, 50)                     # four rows per wave; the product's width; the scalar form
RUNS = (("clean", "clean"), ("clean again", "clean"), ("nan", "nan"), ("huge", "huge"))
MIX_FWD = ["mrg_mix_stats_coef", "mrg_mix_fwd"]
MIX_BWD = ["mrg_mix_bwd_reduce", "mrg_mix_bwd_apply"]


# ---- the four runs ----------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Bit for bit: torch.equal, or -- where a result legitimately holds a NaN or an infinity -- equal bit patterns."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if torch.equal(a, b):
        return True
    if not a.dtype.is_floating_point:
        return False
    as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def first_difference(a, b):
    bad = (a != b) | (torch.isnan(a) != torch.isnan(b)) if a.dtype.is_floating_point else (a != b)
    idx = bad.nonzero()
    where = tuple(int(i) for i in idx[0]) if idx.numel() else ()
    return f"{int(bad.sum())} of {a.numel()} elements differ, first at {where}: {a[where].item() if where or a.dim() == 0 else '?'} vs " \
           f"{b[where].item() if where or b.dim() == 0 else '?'}"


def stale_check(monkeypatch, what, run, want, absent=(), skip_bytes=SKIP_BYTES_DEFAULT):
    """run() -> [(name, tensor or None)] four times (RUNS); the three assertions of the module docstring.  want: entry points that must
    have completed a call in every run; absent: entry points that must not have run."""
    results, launched = {}, {}
    for tag, pattern in RUNS:
        with poisoned(monkeypatch, pattern, skip_bytes) as fills:
            _lib.meter.start()
            try:
                res = run()
            finally:                                         # (stop() synchronises the device; the plan builders of graph.py are not the subject)
                rec = {k: v["launches"] for k, v in _lib.meter.stop().items() if not ("plan" in k or "meta_pack" in k or "build" in k)}
            results[tag] = [(n, None if t is None else t.detach().clone()) for n, t in res]
        assert not _lib.meter.refused, f"{what} [{tag}]: an entry point returned an error: {_lib.meter.refused}"
        for name in want:
            assert rec.get(name, 0) >= 1, f"{what} [{tag}]: {name} did not complete a call: {sorted(rec)}"
        for name in absent:
            assert name not in rec, f"{what} [{tag}]: {name} ran: {sorted(rec)}"
        assert fills.tensors > 0, f"{what} [{tag}]: the harness filled nothing: the path no longer allocates through torch.empty & co"
        launched[tag] = rec
    print(f"{what}: {fills}; entry points {sorted(launched['clean'])}")
    clean = results["clean"]
    names = [n for n, _ in clean]
    assert len(set(names)) == len(names), names
    for tag, _ in RUNS[1:]:
        assert [n for n, _ in results[tag]] == names and [t is None for _, t in results[tag]] == [t is None for _, t in clean], (what, tag)
        assert launched[tag] == launched["clean"], f"{what} [{tag}]: other launches than the clean run: {launched[tag]} vs {launched['clean']}"
    for (n, a), (_, b) in zip(clean, results["clean again"]):
        assert a is None or same(a, b), f"{what} {n}: not reproducible, poison comparison void ({first_difference(a, b)})"
    for tag in ("nan", "huge"):
        for (n, a), (_, b) in zip(clean, results[tag]):
            if a is None:
                continue
            if a.dtype.is_floating_point:
                lost = torch.isfinite(a) & ~torch.isfinite(b)
                assert not bool(lost.any()), f"{what} {n} [{tag}]: {int(lost.sum())} of {a.numel()} elements are not finite where the clean run is; " \
                                             f"first at {tuple(int(i) for i in lost.nonzero()[0])}"
        for (n, a), (_, b) in zip(clean, results[tag]):
            assert a is None or same(a, b), f"{what} {n} [{tag}]: differs from the clean run ({first_difference(a, b)})"
    return launched["clean"]


def dev(t):
    return None if t is None else t.to(DEV)


def leaf(t):
    return None if t is None else t.to(DEV).requires_grad_(True)


def grads_of(names, tensors):
    return [("grad " + n, None if t is None else t.grad) for n, t in zip(names, tensors)]


def partials(cs, D):
    """The n partial [2][D] float64 blocks a producer left (a _lib.ColSums): what mrg_mix_stats_coef reads, and nothing else."""
    if cs is None:
        return None
    flat = cs.buf.view(torch.float64)[cs.offset // 8:]
    return flat.as_strided((cs.n, 2 * D), (cs.stride, 1))


def bn_modules(D, n, seed, training=True):
    bns = [torch.nn.BatchNorm1d(D).to(DEV) for _ in range(n)]
    for k, bn in enumerate(bns):
        with torch.no_grad():
            bn.weight.copy_(seeded(f"gam{k}", (D,), seed, 0.1, 1.0)); bn.bias.copy_(seeded(f"bet{k}", (D,), seed, 0.3))
            bn.running_mean.copy_(seeded(f"rm{k}", (D,), seed, 0.2, 0.5 * k)); bn.running_var.copy_(seeded(f"rv{k}", (D,), seed, 0.1, 1.0 + k).abs() + 0.1)
        bn.train(training)
    return bns


def bn_results(bns):
    out = []
    for k, bn in enumerate(bns):
        out += [(f"grad gamma{k}", bn.weight.grad), (f"grad beta{k}", bn.bias.grad), (f"running_mean{k}", bn.running_mean), (f"running_var{k}", bn.running_var)]
    return out


# ---- row GEMM and weight gradient -------------------------------------------------------------------------------------------------
def wgrad_row_blocks(rows, Kin, Nout):
    """The row blocks G of csrc/wgrad_plan.hpp (share 1): one partial tile of the workspace each.  More than one from 65 rows on
    (five 16-row tiles: gsmall = ceil(tiles / 4) >= 2)."""
    TM, TN = (Nout + 31) // 32, (Kin + 1 + 31) // 32
    tiles = (rows + 15) // 16
    ny = -(-TN // (16 if TM <= 4 else 8))
    gmax = max(256 // ny, 32)
    G_ = max(min((tiles + 15) // 16, gmax), min((tiles + 3) // 4, 8), 1)
    tpb = max(-(-tiles // G_), 1)
    return max(-(-rows // (tpb * 16)), 1), TM * 32 * TN * 32 * 4


LINEAR_CASES = [(M, 64, 64, "relu"), (M, 200, 200, None), (M, 50, 50, "sigmoid"), (M, 400, 200, "relu"), (9, 200, 200, "relu"), (9, 64, 64, None),
                (9, 50, 50, None), (4099, 200, 200, None), (64, 64, 64, None), (65, 64, 64, None)]


@pytest.mark.parametrize("rows,Kin,Nout,act", LINEAR_CASES)
def test_row_linear(monkeypatch, rows, Kin, Nout, act):
    """K.linear: mrg_linear_fwd, mrg_linear_bwd_input, mrg_linear_bwd_weight with one partial tile (rows <= 64) and with several."""
    seed = 100 + rows + Kin
    x0, W0, b0, g0 = seeded("x", (rows, Kin), seed), seeded("W", (Nout, Kin), seed, (2.0 / (Kin + Nout)) ** 0.5), seeded("b", (Nout,), seed, 0.1), seeded("g", (rows, Nout), seed)
    blocks, tile = wgrad_row_blocks(rows, Kin, Nout)
    assert int(_lib.load().mrg_linear_bwd_weight_workspace_bytes(rows, Kin, Nout)) == blocks * tile
    assert blocks == {9: 1, 64: 1, 65: 2, M: 8, 4099: 17}[rows]

    def run():
        x, W, b = leaf(x0), leaf(W0), leaf(b0)
        y = K.linear(x, W, b, act)
        y.backward(dev(g0))
        return [("y", y)] + grads_of(("x", "W", "b"), (x, W, b))

    stale_check(monkeypatch, f"linear rows {rows} K {Kin} N {Nout} {act}", run, ["mrg_linear_fwd", "mrg_linear_bwd_input", "mrg_linear_bwd_weight"])


@pytest.mark.parametrize("B,D,N", [(65, 52, 1100), (129, 50, 1031)])
def test_row_linear_wide(monkeypatch, B, D, N):
    """The [B, N] score product (Nout > 1024): the weight gradient as a row GEMM over the transposed operands; at B <= 128 (or whole
    float4 rows) also mrg_act_grad_transpose and the input gradient on the weight-gradient kernel, else the plain input gradient."""
    x0, W0, b0, g0 = seeded("x", (B, D), 7, 0.3), seeded("W", (N, D), 7, 0.3), seeded("b", (N,), 7, 0.1), seeded("g", (B, N), 7)

    def run():
        x, W, b = leaf(x0), leaf(W0), leaf(b0)
        y = K.linear(x, W, b, "sigmoid")
        y.backward(dev(g0))
        return [("y", y)] + grads_of(("x", "W", "b"), (x, W, b))

    transposed = B <= 128 or (B % 4 == 0 and D % 4 == 0)
    rec = stale_check(monkeypatch, f"wide linear B {B} D {D} N {N}", run,
                      ["mrg_linear_fwd"] + (["mrg_act_grad_transpose", "mrg_linear_bwd_weight"] if transposed else ["mrg_linear_bwd_input"]),
                      absent=["mrg_linear_bwd_input"] if transposed else ["mrg_act_grad_transpose", "mrg_linear_bwd_weight"])
    assert rec["mrg_linear_fwd"] == 2, "the wide weight gradient is a second mrg_linear_fwd"


# ---- gates ----------------------------------------------------------------------------------------------------------------------
GATE_NAMES = ["s", "s_in"] + [f"{w}_{x}" for x in ("in", "out", "self") for w in ("W", "b", "a")]


GATE_FORMS = [("comp", True), ("comp", False), ("row", True), ("row", False), ("row sums", True), ("row sums", False), ("last", False)]


@pytest.mark.parametrize("form,has_in", GATE_FORMS, ids=[f + (" s_in" if i else "") for f, i in GATE_FORMS])
@pytest.mark.parametrize("D", WIDTHS)
def test_gates(monkeypatch, D, has_in, form):
    """mrg_gate_fwd / _bwd (f_sparse_comp, f_sparse_last), the row-factor form mrg_gate_row_fwd / _bwd with and without its
    column-sum blocks (the per-workgroup float64 partials a first-stage MixedOp takes its statistics from)."""
    b0, b1 = R.BOUNDS[M]
    seed = 1000 + D
    s0, sin0 = R.rows_input("gate s", M, D, seed), (R.rows_input("gate s_in", M, D, seed) if has_in else None)
    g0, gq0, norm0 = R.rows_input("gate g", M, D, seed), seeded("gate gq", (M,), seed), R.norm_of(b1, seed)
    P0 = R.gate_params(D, 2 * D if has_in else D, seed)

    def run():
        s, s_in, P = leaf(s0), leaf(sin0), [leaf(p) for p in P0]
        extra = []
        if form == "comp":
            out = K.gate_comp(s, s_in, dev(norm0), b0, b1, *P)
            out.backward(dev(g0))
        elif form == "last":
            out = K.gate_last(s, *P[:3])
            out.backward(dev(g0))
        else:
            cand = K.gate_comp_row_factor(s, s_in, dev(norm0), b0, b1, *P, for_epilogue=K.ForEpilogue(stats=form == "row sums"))
            out = cand.y
            assert out.shape == (M,) and (cand.sums is not None) == (form == "row sums"), "the row factor's column sums"
            out.backward(dev(gq0))
            extra = [("sums of s", partials(cand.s_sums, D)), ("sums of s f", partials(cand.sums, D))]
        return [("out", out)] + grads_of(GATE_NAMES, [s, s_in] + P) + extra

    want = {"comp": ["mrg_gate_collapse3", "mrg_gate_fwd", "mrg_gate_bwd", "mrg_gate_param_grad3"], "last": ["mrg_gate_fwd", "mrg_gate_bwd"]}.get(
        form, ["mrg_gate_collapse3", "mrg_gate_row_fwd", "mrg_gate_row_bwd", "mrg_gate_param_grad3"])
    stale_check(monkeypatch, f"gate {form} D {D} s_in {has_in}", run, want)


# ---- dense filters ----------------------------------------------------------------------------------------------------------------
DENSE_OPS = (("f_dense_comp", 0, True, 1.0 / 3.0), ("f_comp", 1, False, 1.0))


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("rows", [M, 9])
@pytest.mark.parametrize("D", WIDTHS)
def test_dense_filters(monkeypatch, D, rows, tied):
    """K.dense_filter_comp for f_dense_comp and f_comp with K1 + K2 tied (s_in is s: the weight halves fold) and untied: the grouped
    forward mrg_dense_filter_fwd3, the dz pass (dz3 / dz), the shared input gradient and the weight3 / per-segment weight gradient."""
    b0, b1 = R.BOUNDS[M] if rows == M else (3, 6)
    seed = 5000 + D
    s0, sin0, g0 = R.rows_input("dense s", rows, D, seed), R.rows_input("dense s_in", rows, D, seed), R.rows_input("dense g", rows, D, seed)
    norm0 = R.norm_of(b1, seed)
    lib = _lib.load()
    grouped = lib.mrg_linear_bwd_input3_workspace_bytes(D, D) > 0 and lib.mrg_linear_bwd_weight3_workspace_bytes(b0, b1, rows, D, 0 if tied else D, D) > 0
    for name, kind, bias, self_scale in DENSE_OPS:
        P0 = R.dense_params(D, seed, bias)

        def run():
            s = leaf(s0)
            s_in = s if tied else leaf(sin0)
            P = [leaf(p) for p in P0]
            out = K.dense_filter_comp(kind, s, s_in, dev(norm0), b0, b1, *P, self_scale)
            out.backward(dev(g0))
            return [("out", out), ("grad s", s.grad), ("grad s_in", None if tied else s_in.grad)] + grads_of([f"p{i}" for i in range(6)], P)

        rec = stale_check(monkeypatch, f"{name} D {D} rows {rows} tied {tied}", run, [])
        assert "mrg_dense_filter_fwd3" in rec or "mrg_dense_filter_fwd" in rec, sorted(rec)
        assert ("mrg_dense_filter_dz3" in rec) == grouped and ("mrg_dense_filter_dz" in rec) == (not grouped), sorted(rec)
        assert ("mrg_linear_bwd_weight3" in rec) == grouped and ("mrg_linear_bwd_weight_share" in rec) == (not grouped), sorted(rec)


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("D", [200, 64])
def test_dense_pair(monkeypatch, D, tied):
    """The dense pair node (f_dense_comp and f_comp of one MixedOp from one read of the operands) with its column-sum blocks, stored
    and gate-only; its backward runs in test_first_stage_mixedop."""
    b0, b1 = R.BOUNDS[M]
    gen = torch.Generator().manual_seed(31 + D)
    s0, sin0 = torch.randn(M, D, generator=gen), torch.randn(M, D, generator=gen)
    norm0 = torch.rand(b1, generator=gen) + 0.1
    W = lambda: torch.randn(D, 2 * D, generator=gen) / (2 * D) ** 0.5
    dense0 = [t for _ in range(3) for t in (W(), 0.1 * torch.randn(D, generator=gen))]
    comp0 = [W() for _ in range(3)]
    assert K.dense_pair_available(D, tied)
    K_ = D if tied else 2 * D
    blocks = [int(_lib.load().mrg_dense_filter3_colsum_blocks(kind, b0, b1, M, D, K_)) for kind in (0, 1)]

    def run():
        s = dev(s0)
        s_in = s if tied else dev(sin0)
        res = []
        with torch.no_grad():
            for gate_only in (False, True):
                d, c = K.dense_filter_pair(s, s_in, dev(norm0), b0, b1, [dev(t) for t in dense0], [dev(t) for t in comp0], gate_only=gate_only,
                                           for_epilogue=K.ForEpilogue(stats=True))
                assert (d.sums is not None) == (blocks[0] > 0) and (c.sums is not None) == (blocks[1] > 0), "which launches have a column-sum form"
                tag = "gate only " if gate_only else "stored "
                res += [(tag + "f_dense_comp", d.y), (tag + "f_comp", c.y), (tag + "c", d.c), (tag + "sums d", partials(d.sums, D)), (tag + "sums c", partials(c.sums, D))]
        return res

    rec = stale_check(monkeypatch, f"dense pair D {D} tied {tied} colsum blocks {blocks}", run, ["mrg_dense_filter_fwd3"])
    print(f"dense pair D {D} tied {tied}: column-sum blocks {blocks}, {rec}")


# ---- MixedOp and cell zero ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kn", [2, 5])
@pytest.mark.parametrize("D", WIDTHS)
def test_mixed_epilogue(monkeypatch, D, Kn):
    """K.mixed_epilogue in training mode with K = 2 and K = 5 stored candidates (the second of five absent, an addend with five): the
    coef / sums / red tables of mrg_mix_workspace_bytes, the statistics, combine, reduce and apply kernels."""
    seed = 8000 + D + Kn
    present = [not (Kn >= 3 and k == 1) for k in range(Kn)]
    ys0 = [seeded(f"y{k}", (M, D), seed, 1.0 + 0.5 * k, 0.5 * k) if p else None for k, p in enumerate(present)]
    w0, g0 = torch.softmax(seeded("w", (Kn,), seed), 0), R.rows_input("mix g", M, D, seed)
    add0 = R.rows_input("mix addend", M, D, seed) if Kn == 5 else None

    def run():
        bns = bn_modules(D, Kn, seed)
        ys, w, addend = [leaf(y) for y in ys0], leaf(w0), leaf(add0)
        out = K.mixed_epilogue(ys, bns, w, addend=addend, act="relu")
        out.backward(dev(g0))
        return [("out", out)] + grads_of([f"y{k}" for k in range(Kn)] + ["w", "addend"], ys + [w, addend]) + bn_results(bns)

    stale_check(monkeypatch, f"mixed epilogue D {D} K {Kn}", run, MIX_FWD + MIX_BWD + ["mrg_mix_finalize_bwd"])


def first_stage(N, E, Rn, D, tied, seed):
    """A first-stage MixedOp of the supernet over every first-stage operator (five candidates: zero, identity, the row-factor gate
    and the dense pair among them) on a random relation graph: the inputs of test_producer_stats_gpu.first_stage."""
    from mr_gnas_amd import operations_lp as O
    gen = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    et = torch.randint(0, 2 * Rn, (E,), generator=gen)
    g = G.RelGraph(N, src.numpy(), dst.numpy(), et.numpy(), (torch.rand(E, generator=gen) + 0.1).numpy().astype(np.float32), device=DEV)
    h0 = torch.randn(E + N, D, generator=gen)
    hin0 = h0 if tied else torch.randn(E + N, D, generator=gen)
    w0 = torch.softmax(torch.randn(len(O.FIRST_OPS), generator=gen), 0)
    gout = torch.randn(E + N, D, generator=gen)
    torch.manual_seed(seed)
    mixed = S.MixedOp(D, 0.0, O.FIRST_OPS).to(DEV)
    S.xavier_init_(mixed)
    for p in mixed.parameters():
        if p.dim() == 1:
            p.data.add_(0.1 * torch.randn(p.shape, generator=gen).to(DEV))
    return g, mixed, h0, hin0, w0, gout


SWITCHES = {"shipped": {}, "statistics pass": {"PRODUCER_STATS": False}, "stored f_dense_comp": {"GATED_RECOMPUTE": False},
            "stored f_sparse_comp": {"ROW_FACTOR": False}, "side streams": {"FORK_MIN_ROWS": 0}}


@pytest.mark.parametrize("switches", list(SWITCHES))
@pytest.mark.parametrize("D,tied", [(200, False), (200, True), (64, False)])
def test_first_stage_mixedop(monkeypatch, D, tied, switches):
    """The supernet's first-stage MixedOp (K = 5) forward and backward at 1031 rows: producer statistics on (the gates' and dense
    filters' column-sum blocks feed mrg_mix_stats_coef) and off, the recompute forms GATED_RECOMPUTE and ROW_FACTOR on and off, the
    dense pair's backward, and the candidates on side streams."""
    for name, value in SWITCHES[switches].items():
        monkeypatch.setattr(K.switches, name, value)
    N, E = 300, M - 300
    g, mixed, h0, hin0, w0, gout = first_stage(N, E, 4, D, tied, 11 * N + E + D + int(tied))
    state0 = {k: v.clone() for k, v in mixed.state_dict().items()}
    pnames = [n for n, _ in mixed.named_parameters()]

    def run():
        mixed.load_state_dict(state0)
        mixed.zero_grad(set_to_none=True)
        h = leaf(h0)
        hin = h if tied else leaf(hin0)
        w = leaf(w0)
        out = mixed(w, g, h, hin)
        assert "MixedEpilogue" in type(out.grad_fn).__name__
        coef = out.grad_fn.saved_tensors[1]
        out.backward(dev(gout))
        return ([("out", out), ("coef", coef), ("grad h", h.grad), ("grad h_in", None if tied else hin.grad), ("grad w", w.grad)]
                + [("grad " + n, p.grad) for n, p in zip(pnames, mixed.parameters())] + [("buffer " + n, b) for n, b in mixed.named_buffers()])

    rec = stale_check(monkeypatch, f"first-stage MixedOp D {D} tied {tied} {switches}", run, MIX_FWD + MIX_BWD)
    if switches in ("shipped", "side streams"):
        assert "mrg_gate_row_fwd" in rec and "mrg_dense_filter_fwd3" in rec, sorted(rec)
    if switches == "stored f_sparse_comp":
        assert "mrg_gate_fwd" in rec and "mrg_gate_row_fwd" not in rec, sorted(rec)


KINDS = ("mult", "sub", "add")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("D", WIDTHS)
def test_cell_zero(monkeypatch, D, training):
    """K.cell_zero_mixed over the three compose kinds with LazyRows operands (mrg_zero_*, the per-block partials of
    mrg_zero_workspace_bytes), table gradients through mrg_span_gcs."""
    seed = 9000 + D
    gen = torch.Generator().manual_seed(seed)
    N, Rn = 600, 7
    ent0, rel0 = seeded("ent", (N, D), seed), seeded("rel", (Rn, D), seed)
    ei, ri = torch.randint(0, N, (M,), generator=gen), torch.randint(0, Rn, (M,), generator=gen)
    w0, g0 = torch.softmax(seeded("w", (3,), seed), 0), R.rows_input("zero g", M, D, seed)
    gp_e, gp_r = K.GatherPlan(ei.to(DEV), N), K.GatherPlan(ri.to(DEV), Rn)

    def run():
        bns = bn_modules(D, 3, seed, training)
        ent, rel, w = leaf(ent0), leaf(rel0), leaf(w0)
        out = K.cell_zero_mixed(KINDS, K.LazyRows(ent, gp_e), K.LazyRows(rel, gp_r), bns, w)
        out.backward(dev(g0))
        return [("out", out)] + grads_of(("ent", "rel", "w"), (ent, rel, w)) + bn_results(bns)

    stale_check(monkeypatch, f"cell zero D {D} training {training}", run,
                (["mrg_zero_stats_coef"] if training else []) + ["mrg_zero_fwd", "mrg_zero_bwd_reduce", "mrg_zero_bwd_apply"])


# ---- reducers ---------------------------------------------------------------------------------------------------------------------
def hub_block(D, seed):
    """test_nc_gpu.std_block: 300 destinations, a hub of 9 000 in-edges (chunk slots and the hub kernel run), 40 destinations without
    in-edges, 60 of in-degree 1, the rest 2..12, the edge list shuffled.  Returns the Block, the relation graph over the same edges
    (sources folded onto the 300 nodes), messages [E, D], rows [E + N, D] and an upstream gradient [N, D]."""
    gen = torch.Generator().manual_seed(seed)
    n_dst, n_src = 300, 500
    deg = torch.randint(2, 13, (n_dst,), generator=gen)
    deg[0], deg[1:41], deg[41:101] = 9000, 0, 1
    dst = torch.repeat_interleave(torch.arange(n_dst), deg)
    dst = dst[torch.randperm(dst.numel(), generator=gen)]
    E = int(dst.numel())
    src = torch.randint(0, n_src, (E,), generator=gen)
    blk = G.Block(torch.arange(n_src), torch.arange(n_dst), src, dst, torch.arange(E)).to(DEV)
    rel = G.RelGraph(n_dst, src % n_dst, dst, device=DEV)
    x = torch.randn(E + n_dst, D, generator=gen) * 2 + 0.5
    return blk, rel, x, torch.randn(n_dst, D, generator=gen), E, n_dst


@pytest.mark.parametrize("kind", ["sum", "mean", "max"])
@pytest.mark.parametrize("D", WIDTHS)
def test_segment_reducers(monkeypatch, D, kind):
    """K.seg_reduce on the relation graph and on the block, with self rows: the chunk reducer with slot partials and the hub kernel
    (max), the span kernel (sum, mean), the ordered backward."""
    blk, rel, x0, g0, E, N = hub_block(D, 7000 + D)
    assert blk.plan()["n_hubs"] >= 1 and blk.plan()["n_slots"] > 2 and rel.plan()["n_hubs"] >= 1

    def run():
        res = []
        for tag, graph in (("rel ", rel), ("block ", blk)):
            msg, selfr = leaf(x0[:E]), leaf(x0[E:])
            out = K.seg_reduce(kind, msg, selfr, graph)
            out.backward(dev(g0))
            res += [(tag + "out", out), (tag + "grad msg", msg.grad), (tag + "grad self", selfr.grad)]
        return res

    stale_check(monkeypatch, f"seg_reduce {kind} D {D}", run, [("mrg_seg_reduce_fwd" if kind == "max" else "mrg_span_gcs"), "mrg_seg_reduce_bwd_ordered"])


AGG_FORMS = {
    # form: (kind, switches, entry points where the fused forms take the width, entry points where they do not)
    "a_max fused": ("max", {"FUSED_AMAX_MIN_ROWS": 0}, ["mrg_linear_relu_segmax_fwd", "mrg_segmax_bwd_input", "mrg_linear_bwd_weight"],
                    ["mrg_linear_fwd", "mrg_seg_reduce_fwd", "mrg_linear_bwd_input"]),
    "a_max fused dense bwd": ("max", {"FUSED_AMAX_MIN_ROWS": 0, "SPARSE_AMAX_BWD": False},
                              ["mrg_linear_relu_segmax_fwd", "mrg_seg_reduce_bwd_ordered", "mrg_linear_bwd_input"], ["mrg_seg_reduce_fwd"]),
    "a_max two launches": ("max", {"FUSED_AMAX": False}, ["mrg_linear_fwd", "mrg_seg_reduce_fwd", "mrg_seg_reduce_bwd_ordered", "mrg_linear_bwd_input"], None),
    "a_mean heads": ("mean", {"FUSED_AMAX_MIN_ROWS": 0}, ["mrg_linear_relu_segsum_fwd", "mrg_seg_reduce_heads_fwd", "mrg_seg_reduce_bwd_ordered"],
                     ["mrg_linear_fwd", "mrg_span_gcs"]),
    "a_mean span": ("mean", {"FUSED_AMEAN": False}, ["mrg_linear_fwd", "mrg_span_gcs", "mrg_seg_reduce_bwd_ordered"], None),
}


@pytest.mark.parametrize("form", list(AGG_FORMS))
@pytest.mark.parametrize("D", WIDTHS)
def test_linear_relu_aggregate(monkeypatch, D, form):
    """a_max and a_mean as one node (Linear + ReLU + reduce + self rows) on the hub graph: a_max fused (one GEMM with the segmented-max
    epilogue over the 64-bit keys, then the sparse input gradient mrg_segmax_bwd_input) and as two launches; a_mean through the fused
    heads path -- mrg_linear_relu_segsum_fwd leaves run sums at the HEAD rows of `part`, mrg_seg_reduce_heads_fwd reads the rows it
    takes for heads -- with relu_bits in the backward, and through the span path."""
    kind, switches, fused_want, plain_want = AGG_FORMS[form]
    for name, value in switches.items():
        monkeypatch.setattr(K.switches, name, value)
    blk, rel, x0, g0, E, N = hub_block(D, 7100 + D)
    W0, b0 = seeded("aW", (D, D), D, (1.0 / D) ** 0.5), seeded("ab", (D,), D, 0.1)
    fused = K._fused_agg_ws(N, D) > 0 or plain_want is None

    def run():
        x, W, b = leaf(x0), leaf(W0), leaf(b0)
        out = K.linear_relu_aggregate(kind, x, W, b, rel)
        out.backward(dev(g0))
        return [("out", out)] + grads_of(("x", "W", "b"), (x, W, b))

    rec = stale_check(monkeypatch, f"{form} D {D}", run, (fused_want if fused else plain_want) + ["mrg_linear_bwd_weight"])
    assert D % 4 or fused, "the fused forms take every float4 width above 48"


@pytest.mark.parametrize("D", [64, 200])
def test_amax_closes_a_gradient_chain(monkeypatch, D):
    """Three readers of one state: a_max (fused) closes the gradient fan-in chain with mrg_segmax_bwd_input_chain -- the running sum of
    a materialised a_mean gradient, a_sum's gathered gradient and the self rows in its own store -- and, with the chain off, the fan-in
    sum is mrg_sum_rows_gather over a gathered term and self rows."""
    monkeypatch.setattr(K.switches, "FUSED_AMAX_MIN_ROWS", 0)
    blk, rel, x0, g0, E, N = hub_block(D, 7200 + D)
    Ws = [seeded(f"W{i}", (D, D), D, (1.0 / D) ** 0.5) for i in range(2)]
    bs = [seeded(f"b{i}", (D,), D, 0.1) for i in range(2)]
    calls = []
    real = _lib.call

    def spy(name, args, **kw):
        calls.append((name, len(args)))
        return real(name, args, **kw)

    monkeypatch.setattr(K.reducers, "call", spy)
    for chain in (True, False):
        monkeypatch.setattr(K.switches, "FANIN_CHAIN", chain)

        def run():
            x = leaf(x0)
            P = [leaf(t) for t in Ws + bs]
            fan = K.Fan(x * 1.0, 3)
            out = (K.linear_relu_aggregate("max", fan.take(), P[0], P[2], rel) + K.linear_relu_aggregate("mean", fan.take(), P[1], P[3], rel)
                   + K.aggregate_rows("sum", fan.take(), rel))
            out.backward(dev(g0))
            return [("out", out)] + grads_of(("x", "W0", "W1", "b0", "b1"), [x] + P)

        del calls[:]
        rec = stale_check(monkeypatch, f"three readers D {D} chain {chain}", run, ["mrg_linear_relu_segmax_fwd", "mrg_segmax_bwd_input", "mrg_linear_relu_segsum_fwd"])
        chained = [n for n, nargs in calls if n == "mrg_segmax_bwd_input" and nargs == 16]
        print(f"three readers D {D} chain {chain}: {sorted(rec)}; chained a_max launches {len(chained)}")
        if chain:
            assert len(chained) == len(RUNS), "a_max did not close the chain (mrg_segmax_bwd_input_chain)"
        else:
            assert not chained and "mrg_sum_rows_gather" in rec, sorted(rec)


@pytest.mark.parametrize("kind", ["sum", "mean", "max", "std"])
@pytest.mark.parametrize("D", WIDTHS)
def test_block_aggregators(monkeypatch, D, kind):
    """The node-classification aggregators on the block (no self rows): aggregate_std with its float64 slot partials, a_sum on the
    span kernel, a_mean / a_max through linear_relu_aggregate_nc (the partial forms: the fused heads path as a sum, the fused a_max)."""
    monkeypatch.setattr(K.switches, "FUSED_AMAX_MIN_ROWS", 0)
    blk, rel, x0, g0, E, N = hub_block(D, 7300 + D)
    W0, b0 = seeded("aW", (D, D), D, (1.0 / D) ** 0.5), seeded("ab", (D,), D, 0.1)

    def run():
        x, W, b = leaf(x0[:E]), leaf(W0), leaf(b0)
        if kind in ("std", "sum"):
            out = K.aggregate_nc(kind, x, blk)
        else:
            out = K.linear_relu_aggregate_nc(kind, x, W, b, blk)
        out.backward(dev(g0))
        return [("out", out), ("grad x", x.grad)] + ([] if kind in ("std", "sum") else grads_of(("W", "b"), (W, b)))

    fused = K._fused_agg_ws(N, D) > 0
    want = {"std": ["mrg_seg_std_fwd", "mrg_seg_std_bwd"], "sum": ["mrg_span_gcs", "mrg_seg_reduce_bwd_ordered"],
            "max": ["mrg_linear_relu_segmax_fwd"] if fused else ["mrg_linear_fwd", "mrg_seg_reduce_fwd"],
            "mean": ["mrg_linear_relu_segsum_fwd", "mrg_seg_reduce_heads_fwd"] if fused else ["mrg_linear_fwd", "mrg_span_gcs"]}[kind]
    stale_check(monkeypatch, f"block {kind} D {D}", run, want)


@pytest.mark.parametrize("mode", GR.MODES)
@pytest.mark.parametrize("D", WIDTHS)
def test_fused_gcs(monkeypatch, D, mode):
    """mrg_fused_gcs in its six modes (and mrg_span_gcs in the four elementwise ones) on gcs_ref.mixed: a 9 000-element hub split
    into chunk slots, empty segments, lists of 1, 64, 65 and 128 elements."""
    c = GR.mixed(D)
    needs_y = mode not in ("copy", "negs")
    seg = c["seg"].to(DEV).int()
    plan, sp = G.dst_csr_plan(seg, c["nseg"]), G.span_plan(seg, c["nseg"])
    assert plan["n_hubs"] >= 1

    def run():
        X, Y = dev(c["X"]), (dev(c["Y"]) if needs_y else None)
        xi, yi, scal = c["xi"].to(DEV).int(), (c["yi"].to(DEV).int() if needs_y else None), dev(c["scal"])
        res = [("fused", K.fused_gcs(mode, X, xi, Y, yi, scal, plan, c["nseg"]))]
        if mode in GR.SPAN_MODES:
            res.append(("span", K.span_gcs(mode, X, Y, G.span_meta(sp, xi, yi, scal), sp)))
        return res

    stale_check(monkeypatch, f"fused_gcs {mode} D {D}", run, ["mrg_fused_gcs"] + (["mrg_span_gcs"] if mode in GR.SPAN_MODES else []))


# ---- compose, gather, fan-in, ccorr ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_compose_gather_and_fan_in(monkeypatch, D):
    """gather_compose with LazyRows operands (table gradients: span sums), K.gather_rows, plain compose, and a fan-in sum of three
    readers of one tensor."""
    seed = 3000 + D
    gen = torch.Generator().manual_seed(seed)
    N, Rn = 515, 5
    ent0, rel0, g0 = seeded("ent", (N, D), seed), seeded("rel", (Rn, D), seed), R.rows_input("compose g", M, D, seed)
    ei, ri = torch.randint(0, N, (M,), generator=gen), torch.randint(0, Rn, (M,), generator=gen)
    gp_e, gp_r = K.GatherPlan(ei.to(DEV), N), K.GatherPlan(ri.to(DEV), Rn)

    def run():
        res = [("gather", K.gather_rows(dev(ent0), ei.to(DEV).int()))]
        for kind in KINDS:
            e, r = leaf(ent0), leaf(rel0)
            out = K.compose(kind, K.LazyRows(e, gp_e), K.LazyRows(r, gp_r))
            out.backward(dev(g0))
            s, h = leaf(ent0[ei]), leaf(rel0[ri])
            fan = K.Fan(s * 1.0, 3)
            plain = K.compose(kind, fan.take(), h) + K.compose("mult", fan.take(), fan.take())
            plain.backward(dev(g0))
            res += [(kind + " lazy out", out), (kind + " grad ent", e.grad), (kind + " grad rel", r.grad), (kind + " plain out", plain),
                    (kind + " grad s", s.grad), (kind + " grad hr", h.grad)]
        return res

    stale_check(monkeypatch, f"compose / gather / fan-in D {D}", run, ["mrg_gather_compose_fwd", "mrg_span_gcs", "mrg_compose_fwd", "mrg_compose_bwd", "mrg_sum_buffers"])


@pytest.mark.parametrize("path", ["rows", "matrix"])
@pytest.mark.parametrize("D", WIDTHS)
def test_ccorr(monkeypatch, D, path):
    """ccorr of [M, D] rows with one shared row in both paths (switches.CCORR_PATH): the per-row kernel on expanded rows, and the
    circulant on the row GEMM where the width admits it (a multiple of 4 above 48)."""
    monkeypatch.setattr(K.switches, "CCORR_PATH", path)
    a0, b0, g0 = seeded("a", (M, D), D, 0.5), seeded("b", (1, D), D, 0.5), seeded("g", (M, D), D)
    matrix = path == "matrix" and D % 4 == 0 and D > 48

    def run():
        res = []
        for tag, swap in (("shared b ", False), ("shared a ", True)):
            a, b = leaf(a0), leaf(b0)
            out = K.ccorr(b, a) if swap else K.ccorr(a, b)
            out.backward(dev(g0))
            res += [(tag + "out", out), (tag + "grad a", a.grad), (tag + "grad b", b.grad)]
        return res

    stale_check(monkeypatch, f"ccorr {path} D {D}", run, ["mrg_ccorr_matrix", "mrg_ccorr_matrix_grad", "mrg_linear_fwd"] if matrix else ["mrg_ccorr_rows"],
                absent=["mrg_ccorr_rows"] if matrix else ["mrg_ccorr_matrix"])


# ---- candidate Linears ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [57, 4099])
def test_candidate_linears(monkeypatch, rows):
    """The grouped candidate Linears of a node-classification MixedOp at D = 64: forward with its per-workgroup column-sum blocks,
    the grouped input gradient, the weight gradients."""
    D, n = 64, 3
    gen = torch.Generator().manual_seed(rows)
    xs0 = [torch.randn(rows, D, generator=gen) * 1.5 + 0.25 for _ in range(n)]
    gs0 = [torch.randn(rows, D, generator=gen) for _ in range(n)]
    Ws0 = [torch.randn(D, D, generator=gen) / D ** 0.5 for _ in range(n)]
    bs0 = [0.3 * torch.randn(D, generator=gen) for _ in range(n)]
    assert int(_lib.load().mrg_cand_linear_colsum_blocks(rows, D)) > 0

    def run():
        lins = []
        for W, b in zip(Ws0, bs0):
            lin = torch.nn.Linear(D, D).to(DEV)
            with torch.no_grad():
                lin.weight.copy_(W); lin.bias.copy_(b)
            lins.append(lin)
        xs = [leaf(x) for x in xs0]
        cands = K.candidate_linears(xs, lins, for_epilogue=K.ForEpilogue(stats=True))
        assert all(c.kind == "stored" and c.sums is not None for c in cands)
        torch.autograd.backward([c.y for c in cands], [dev(g) for g in gs0])
        res = []
        for k, (c, x, lin) in enumerate(zip(cands, xs, lins)):
            res += [(f"y{k}", c.y), (f"sums{k}", partials(c.sums, D)), (f"grad x{k}", x.grad), (f"grad W{k}", lin.weight.grad), (f"grad b{k}", lin.bias.grad)]
        return res

    stale_check(monkeypatch, f"candidate linears rows {rows}", run, ["mrg_cand_linear_fwd", "mrg_cand_linear_bwd_input", "mrg_linear_bwd_weight"])


# ---- ConvE ------------------------------------------------------------------------------------------------------------------------
CONVE_CASES = [(0, True, 65), (0, False, 65), (1, True, 65), (1, False, 65), (0, True, 300)]


@pytest.mark.parametrize("layout,training,B", CONVE_CASES, ids=[f"{'stacked' if l == 0 else 'interleaved'}-{'train' if t else 'eval'}-B{b}" for l, t, b in CONVE_CASES])
def test_conve(monkeypatch, layout, training, B):
    """The ConvE feature path, no dropout: D = 32 as a 16 x 4 stacked or an 8 x 8 interleaved image, F = 33 filters (across the
    32-filter chunk), ks = 3, B = 65 (across the 64-row tile; stacked K = 924: a split-K fc with S > 1 partial blocks) and B = 300
    (the weight-gradient slabs cover two images per range)."""
    D, F, ks = 32, 33, 3
    Hi, Wi = (16, 4) if layout == 0 else (8, 8)
    Kfc = F * (Hi - ks + 1) * (Wi - ks + 1)
    lib = _lib.load()
    S_ = int(lib.mrg_conve_fc_workspace_bytes(B, Kfc, D)) // (B * D * 4)
    assert Kfc == (924 if layout == 0 else 1188) and (S_ > 1 or B != 65), f"fc splits {S_}"
    slabs = (int(lib.mrg_conve_bwd_workspace_bytes(B, D, F, ks)) - (B * 2 * D * 4 + 15) // 16 * 16 - B * 16) // (F * (ks * ks + 1) * 8)
    assert slabs == (B if B == 65 else 150), slabs
    torch.manual_seed(5)
    mods = [torch.nn.BatchNorm2d(1), torch.nn.Conv2d(1, F, ks), torch.nn.BatchNorm2d(F), torch.nn.Linear(Kfc, D)]
    with torch.no_grad():
        for m in (mods[0], mods[2]):
            m.weight.add_(0.1 * torch.randn_like(m.weight)); m.bias.add_(0.1 * torch.randn_like(m.bias))
            m.running_mean.add_(0.1 * torch.randn_like(m.running_mean)); m.running_var.add_(0.2 * torch.rand_like(m.running_var))
    state0 = [{k: v.clone() for k, v in m.state_dict().items()} for m in mods]
    sub0, rel0, g0 = seeded("sub", (B, D), B), seeded("rel", (B, D), B), seeded("gh", (B, D), B)
    mods = [m.to(DEV) for m in mods]

    def run():
        for m, st in zip(mods, state0):
            m.load_state_dict(st)
            m.zero_grad(set_to_none=True)
            m.train(training)
        sub, rel = leaf(sub0), leaf(rel0)
        h = K.conve_features(sub, rel, layout, (Hi, Wi), mods[0], mods[1], mods[2], None, mods[3], None)
        h.backward(dev(g0))
        res = [("h", h), ("grad sub", sub.grad), ("grad rel", rel.grad)]
        for i, m in enumerate(mods):
            res += [(f"grad m{i}.{n}", p.grad) for n, p in m.named_parameters()] + [(f"m{i}.{n}", b) for n, b in m.named_buffers() if "running" in n]
        return res

    stale_check(monkeypatch, f"conve layout {layout} training {training} B {B}", run,
                ["mrg_conve_bn0_fwd", "mrg_conve_conv_fwd", "mrg_conve_bn1_fwd", "mrg_conve_fc_fwd", "mrg_conve_fc_bwd", "mrg_conve_bn1_bwd",
                 "mrg_conve_conv_bwd", "mrg_conve_finish_bwd"])


# ---- 1-N losses and sweeps --------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = [(129, 449, 52), (5, 28672 + 65, 33), (8192 + 3, 33, 33)]      # tile edges; a second column block; a second row chunk
NREL = 3


def label_index(N, B, seed):
    """A LabelIndex over random triples with a key that lists every entity, an unknown key and a repeated query (the index of
    test_fused_scorers_gpu.make_index), and a batch of B queries with targets."""
    rng = np.random.default_rng(seed)
    T = 3 * N
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, NREL - 1, T), rng.integers(0, N, T)], 1)
    tri = np.concatenate([tri, np.asarray([(0, 0, o) for o in range(N)], dtype=tri.dtype)])
    subj, rel, tgt = rng.integers(0, N, B), rng.integers(0, 2 * NREL, B), rng.integers(0, N, B)
    for i, (s, r) in enumerate([(0, 0), (min(1, N - 1), 0), (int(rng.integers(0, N)), NREL - 1), (0, 0)][:B]):
        subj[i], rel[i] = s, r
    li = LabelIndex(tri, NREL, N, DEV)
    return li, torch.from_numpy(subj).to(DEV), torch.from_numpy(rel).to(DEV), torch.from_numpy(tgt).to(DEV)


@pytest.mark.parametrize("scorer", ["distmult", "rows with bias", "transe", "two-way mix", "three-way mix"])
@pytest.mark.parametrize("B,N,D", SWEEP_SHAPES)
def test_one_to_n_sweeps(monkeypatch, B, N, D, scorer):
    """Per scorer the 1-N loss with its gradients, the filtered ranks and (DistMult, rows with bias, TransE) the filtered top-k: the
    per-workgroup loss partials, the qlist / qinfo tables, the counts, and the running lists that a second column block merges into."""
    li, subj, rel, tgt = label_index(N, B, B + N)
    seed = B + N + D
    ent0, sub0, rel0 = seeded("ent", (N, D), seed, 0.3), seeded("sub", (B, D), seed, 0.3), seeded("relrows", (B, D), seed, 0.5)
    hid0, bias0 = seeded("hidden", (B, D), seed, 0.3), seeded("bias", (N,), seed, 0.2)
    gamma, k = 4.0, min(10, N)
    side = EV._LabelSide(li)
    when = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    qkey = (subj.long() * side.num_rels + rel.long()).contiguous()

    def run():
        ent, sub, relr, hid, bias = leaf(ent0), leaf(sub0), leaf(rel0), leaf(hid0), leaf(bias0)
        w = leaf(torch.tensor([0.3, 0.7] if scorer == "two-way mix" else [0.2, 0.3, 0.5]))
        res, used = [], [ent, sub, relr]
        if scorer == "distmult":
            loss = K.distmult_bce_all(ent, sub, relr, li, subj, rel, 0.1)
            q, kind, bias_ = (sub * relr).detach(), "dot", None
        elif scorer == "rows with bias":
            q = (sub * relr)
            loss = K.dot_bce_all(ent, q, li, subj, rel, 0.1, bias=bias)
            q, kind, bias_ = q.detach(), "dot", bias.detach()
            used.append(bias)
        elif scorer == "transe":
            loss = K.transe_bce_all(ent, sub, relr, gamma, li, subj, rel, 0.1)
            q, kind, bias_ = (sub + relr).detach(), "l1", None
        elif scorer == "two-way mix":
            loss = K.sf_mix_bce_all(ent, sub, relr, w, gamma, li, subj, rel, 0.1)
            used.append(w)
        else:
            loss = K.sf_mix3_bce_all(ent, sub, relr, hid, w, gamma, li, subj, rel, 0.1)
            used += [hid, w]
        (3.0 * loss).backward()
        res = [("loss", loss)] + [(f"grad {i}", t.grad) for i, t in enumerate(used)]
        with torch.no_grad():
            if scorer in ("two-way mix", "three-way mix"):
                hidden = hid.detach() if scorer == "three-way mix" else None
                res += [("ranks", EV.mix_ranks(sub.detach(), relr.detach(), ent.detach(), w.detach(), gamma, tgt, side, when, qkey, hidden=hidden)),
                        ("raw ranks", EV.mix_ranks(sub.detach(), relr.detach(), ent.detach(), w.detach(), gamma, tgt, hidden=hidden))]
            else:
                res += [("ranks", EV.query_ranks(q, ent.detach(), tgt, side, when, qkey, kind=kind, bias=bias_)),
                        ("raw ranks", EV.query_ranks(q, ent.detach(), tgt, kind=kind, bias=bias_))]
                ids, vals = EV.query_topk(q, ent.detach(), k, side, when, qkey, kind=kind, bias=bias_)
                res += [("top-k ids", ids), ("top-k values", vals)]
        return res

    want = {"distmult": ["mrg_distmult_bce_fwd", "mrg_distmult_bce_dlogit", "mrg_rows_rank", "mrg_rows_topk"],
            "rows with bias": ["mrg_rows_bias_bce_fwd", "mrg_rows_bias_bce_dlogit", "mrg_rows_bias_rank", "mrg_rows_bias_topk"],
            "transe": ["mrg_transe_bce_fwd", "mrg_transe_bce_dlogit", "mrg_transe_rank", "mrg_transe_topk"],
            "two-way mix": ["mrg_sfmix_bce_fwd", "mrg_sfmix_bce_grad", "mrg_sfmix_rank"],
            "three-way mix": ["mrg_sfmix3_bce_fwd", "mrg_sfmix3_bce_grad", "mrg_sfmix3_rank"]}[scorer]
    stale_check(monkeypatch, f"{scorer} B {B} N {N} D {D}", run, want)


# ---- end to end, eager ----------------------------------------------------------------------------------------------------------------
def net_results(net, outs, alphas=()):
    res = list(outs) + [("grad " + n, p.grad) for n, p in net.named_parameters()] + [("buffer " + n, b) for n, b in net.named_buffers()]
    return res + [(f"grad alpha{i}", a.grad) for i, a in enumerate(alphas)]


def reset(net, state0, alphas=()):
    net.load_state_dict(state0)
    net.zero_grad(set_to_none=True)
    for a in alphas:
        a.grad = None
    net.train()


@pytest.mark.parametrize("case", ["supernet_tiny", "supernet_d24"])
def test_search_network_step(monkeypatch, case):
    """SearchNetwork forward, get_loss, backward on the golden step graphs: outputs, loss, parameter and alpha gradients, buffers."""
    from test_nets_gpu import load_net_state
    z = load_golden(case)
    n = z["node_id"].numel()
    g = G.RelGraph(n, z["src"], z["dst"], z["edge_type"], z["norm"], device=DEV)
    net = S.SearchNetwork(DEV, z["Nall"], z["R"], z["layers"], 1, 2, 2, z["D"], z["D0"], z["nbase"], 9.0, 0.0, 0.0).to(DEV)
    load_net_state(net, z)
    net.load_alpha([z[f"alpha/{i}"].to(DEV) for i in range(5)])
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    alphas = net.arch_parameters()[:4]

    def run():
        reset(net, state0, net.arch_parameters())
        ent, rel = net(g, z["node_id"].to(DEV), z["src_in"].to(DEV), z["edge_type"].to(DEV))
        loss = net.get_loss(g, ent, rel, z["data"].to(DEV), z["labels"].to(DEV))
        loss.backward()
        return net_results(net, [("ent", ent), ("rel", rel), ("loss", loss)], alphas)

    stale_check(monkeypatch, case, run, MIX_FWD + MIX_BWD + ["mrg_zero_fwd"])


def test_fixed_network_step(monkeypatch):
    """FixedNetwork (the README genotype) on fixednet_tiny: predictions, loss, every gradient."""
    from conftest import sub
    from test_nets_gpu import README_GENOTYPE
    z = load_golden("fixednet_tiny")
    g = G.RelGraph(z["N"], z["src"], z["dst"], z["etype"], z["norm"], device=DEV)
    net = S.FixedNetwork(DEV, README_GENOTYPE, z["N"], z["R"], z["D"], z["D0"], z["nbase"], score_args={"gamma": 9.0}).to(DEV)
    net.load_state_dict({**sub(z, "param/"), **sub(z, "buffer/")})
    state0 = {k: v.clone() for k, v in net.state_dict().items()}

    def run():
        reset(net, state0)
        pred = net(g, z["subj"].to(DEV), z["rel"].to(DEV))
        loss = torch.nn.functional.binary_cross_entropy(pred, z["label"].to(DEV))
        loss.backward()
        return net_results(net, [("pred", pred), ("loss", loss)])

    rec = stale_check(monkeypatch, "fixednet_tiny", run, ["mrg_mix_fwd"])
    assert any(k.startswith("mrg_gate") for k in rec) and any("seg" in k for k in rec), sorted(rec)


def test_nc_network_step(monkeypatch):
    """The node-classification Network on nc_fixednet_small/n1: logits, loss, gradients, running statistics.  model_nc gathers the
    node and relation rows with torch.index_select (see the module docstring): this case runs with torch's deterministic algorithms
    on, so that those gathers' backward is an ordered sum and the clean pair can be compared at all."""
    from test_nc_cpu import fixture_blocks, make_net
    z, tag = load_golden("nc_fixednet_small"), "n1"
    net = make_net(z, tag, DEV)
    blocks = [b.to(DEV) for b in fixture_blocks(z, tag + "/blocks/")]
    trip, seeds, labels = z[tag + "/trip_index"].to(DEV), z[tag + "/seeds"].long().to(DEV), z[tag + "/labels"].to(DEV)
    state0 = {k: v.clone() for k, v in net.state_dict().items()}

    def run():
        reset(net, state0)
        logits = net(trip, blocks)
        loss = net._criterion(logits, labels[seeds])
        loss.backward()
        return net_results(net, [("logits", logits), ("loss", loss)])

    import torch.utils.deterministic as TD
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(), TD.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    TD.fill_uninitialized_memory = False          # (torch would fill every torch.empty itself, the integer ones included: the fills are poison.py's)
    try:
        stale_check(monkeypatch, "nc_fixednet_small/n1", run, ["mrg_linear_fwd", "mrg_mix_fwd"])
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
        TD.fill_uninitialized_memory = before[2]


def test_supernet_step_d200_with_hubs_and_side_streams(monkeypatch):
    """The class of step test_c3_wn18rr_supernet_step_matches_float64_oracle runs, small: a D = 200 two-layer supernet over 300 nodes,
    4 relations, 3 000 triples, one node the object of 400 extra triples (its in-degree is several chunks of the plans: chunk slots,
    hub kernels, split spans), FORK_MIN_ROWS = 0 so that candidates and direction segments run on side streams -- an allocation
    recycled across streams is the other way stale memory gets in."""
    monkeypatch.setattr(K.switches, "FORK_MIN_ROWS", 0)
    monkeypatch.setattr(K.switches, "FUSED_AMAX_MIN_ROWS", 0)
    N, Rn, T, D = 300, 4, 3000, 200
    rng = np.random.default_rng(3)
    tri = synth.synth_kg(N, Rn, T - 400, 3)
    hub = np.stack([rng.integers(0, N, 400), rng.integers(0, Rn, 400), np.full(400, 17)], 1)
    tri = np.concatenate([tri, hub]).astype(np.int64)
    samples, labels = synth.negative_sampling(tri, N, 2, np.random.default_rng(4))
    g = G.build_search_graph(N, Rn, tri).to(DEV)
    src, dst, _ = g.edges(form="all")
    deg = torch.bincount(dst.cpu(), minlength=N)
    assert int(deg.max()) > 2 * G.CHUNK_EDGES and g.plan()["n_hubs"] >= 1, "the plans must split the hub"
    node_id, edge_type = torch.arange(N, device=DEV).view(-1, 1), g.edata["e_type"]
    samples_t, labels_t = torch.from_numpy(samples).to(DEV), torch.from_numpy(labels).to(DEV)
    torch.manual_seed(0)
    net = S.SearchNetwork(DEV, N, Rn, 2, 1, 2, 2, D, 100, 2 * Rn + 1, 40.0, 0.0, 0.0).to(DEV)
    S.xavier_init_(net)
    with torch.no_grad():
        for _, p in net.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    alphas = net.arch_parameters()[:4]

    def run():
        reset(net, state0, net.arch_parameters())
        ent, rel = net(g, node_id, src, edge_type)
        loss = net.get_loss(g, ent, rel, samples_t, labels_t)
        loss.backward()
        return net_results(net, [("ent", ent), ("rel", rel), ("loss", loss)], alphas)

    rec = stale_check(monkeypatch, "supernet D 200 with a hub, side streams", run,
                      MIX_FWD + MIX_BWD + ["mrg_zero_fwd", "mrg_gate_row_fwd", "mrg_dense_filter_fwd3", "mrg_linear_relu_segmax_fwd", "mrg_segmax_bwd_input"])
    assert len(K._SIDE_STREAMS) > 0, "no side stream was ever opened"
    print(f"supernet D 200: {sum(rec.values())} launches of {len(rec)} entry points")
