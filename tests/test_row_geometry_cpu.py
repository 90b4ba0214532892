"""The row-geometry matrix without a GPU: (1) csrc/row_geom.hpp, compiled with the host compiler, over the width list of
tests/rowgeom_ref.py -- all ten <VEC, LPR, KMAX> classes, both live-step counts of the KMAX = 4 classes and the first refused
width of each placement are reached by the widths test_row_geometry_gpu.py runs; (2) every restatement of rowgeom_ref, evaluated
in float32, against the project's CPU statement of the same operation (oracle.ops, nn.BatchNorm1d + ReLU + weighted sum) at two
widths, to the tolerance the operator tests hold the kernels to, and a_std in float64 against test_nc_gpu.std_ref64 -- the
reference of the GPU matrix is pinned here; (3) the input conditioning reaches the margins it promises."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import rowgeom_ref as R
from conftest import seeded
from oracle import graph as OG, ops as OO
from test_nc_cpu import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (64, 193)                                              # a float4 width and a scalar one


def test_width_list_reaches_every_class_and_refusal_edge(tmp_path):
    """tools/row_geom_check.cpp walks row_geom over D = 1 .. 1100 on aligned and unaligned bases, prints the class of every listed
    (width, placement) and fails unless the list reaches all ten classes, three and four live steps of A64k4 and S64k4, and the
    first refused widths 1028, 257 and 260u.  The classes it prints are the ones rowgeom_ref.class_of names the GPU cases by."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "row_geom_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mr-gnas_amd", "csrc"),
                            os.path.join(ROOT, "tools", "row_geom_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr[-2000:]
    args = [R.arg_of(D, u) for D, u in R.CONFIGS] + ["!" + R.arg_of(D, u) for D, u in R.REFUSAL_EDGES + R.REFUSED]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    assert "10 classes, 0 never reached, 0 live-step cases missing, 0 refusal edges missing, 0 bad geometries" in run.stdout, run.stdout[-2000:]
    seen = dict(re.findall(r"^(\d+u?): (\w+) live \d$", run.stdout, re.M))
    live = dict(re.findall(r"^(\d+u?): \w+ live (\d)$", run.stdout, re.M))
    assert len(seen) == len(R.CONFIGS)
    for D, u in R.CONFIGS:
        assert seen[R.arg_of(D, u)] == R.class_of(D, u) and int(live[R.arg_of(D, u)]) == R.geom(D, u)[3], (D, u)
    assert {R.class_of(D, u) for D, u in R.CONFIGS} == set(R.CLASSES)
    assert all(R.geom(D, u) is None for D, u in R.REFUSED + R.REFUSAL_EDGES)
    assert run.stdout.count(": refused\n") == len(R.REFUSED) + len(R.REFUSAL_EDGES)


def test_mix_limits_follow_the_host_checks():
    """The three LDS checks by hand at the widths where they bind: D = 1024 (A64k4) takes eight candidates forward and ONE backward
    (4 * 1024 + 4 * 3 * 1024 floats are exactly 64 KB); 512 (A64k2) five (the [K][6][D] apply table); the scalar classes all eight."""
    assert R.mix_limits(1024, False) == (8, 1) and R.mix_limits(772, False) == (8, 1) and R.mix_limits(516, False) == (8, 1)
    assert R.mix_limits(512, False) == (8, 5) and R.mix_limits(260, False) == (8, 8) and R.mix_limits(256, True) == (8, 8)
    assert R.mix_limits(1024, False, R.ZERO_MAXK) == (3, 1) and R.mix_limits(512, False, R.ZERO_MAXK) == (3, 3)
    for D, u in R.CONFIGS:
        fwd, bwd = R.mix_limits(D, u)
        assert 1 <= bwd <= fwd <= R.MIX_MAXK


# ---- the restatements in float32 against the project's CPU statements -----------------------------------------------------------------
def _graph(M, seed):
    """An oracle graph of E = M - N edges in the reference's layout ((b0, b1) = (E / 2, E)) and the [M, D] row bounds."""
    N = 11
    E = M - N
    gen = torch.Generator().manual_seed(seed)
    og = OG.OGraph(N, torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen), torch.zeros(E, dtype=torch.long),
                   R.norm_of(E, seed))
    return og, E // 2, E


def _both(fn_ref, fn_own, leaves, gout, what):
    """Output and every gradient of the two statements agree to close()."""
    a = [t.clone().requires_grad_(True) for t in leaves]
    b = [t.clone().requires_grad_(True) for t in leaves]
    ra, rb = fn_ref(*a), fn_own(*b)
    close(rb, ra.detach(), what + " out")
    for i, (ga, gb) in enumerate(zip(torch.autograd.grad(ra, a, gout), torch.autograd.grad(rb, b, gout))):
        close(gb, ga, f"{what} grad {i}", rtol=3e-4, atol=1e-4)


@pytest.mark.parametrize("D", WIDTHS)
def test_gate_and_dense_restatements_are_the_oracle_operators(D):
    M = 51
    og, b0, b1 = _graph(M, D)
    s, s_in, gout = seeded("s", (M, D), D), seeded("s_in", (M, D), D), seeded("g", (M, D), D)
    P = R.gate_params(D, 2 * D, D)
    names = [f"{n}_{x}.{w}" for x in ("in", "out", "self") for n, w in (("W", "weight"), ("W", "bias"), ("a", "weight"))]
    _both(lambda s, s_in, *p: OO.f_sparse_comp(og, dict(zip(names, p)), s, s_in),
          lambda s, s_in, *p: R.gate_comp(s, s_in, og.norm, b0, b1, p), [s, s_in] + P, gout, "f_sparse_comp")
    # the row factor times the rows is the operator
    _both(lambda s, s_in, *p: OO.f_sparse_comp(og, dict(zip(names, p)), s, s_in),
          lambda s, s_in, *p: s * R.gate_row_factor(s, s_in, og.norm, b0, b1, p).view(-1, 1), [s, s_in] + P, gout, "row factor")
    W, b, a = R.gate_params(D, D, D + 1, (True, False, False))[:3]
    _both(lambda s, W, b, a: OO.f_sparse_last(og, {"W.weight": W, "W.bias": b, "a.weight": a}, s, s),
          lambda s, W, b, a: R.gate_last(s, W, b, a), [s, W, b, a], gout, "f_sparse_last")
    for kind, name, bias, self_scale in ((0, "f_dense_comp", True, 1.0 / 3.0), (1, "f_comp", False, 1.0)):
        Pd = R.dense_params(D, D, bias)
        keys = [f"W_{x}.{w}" for x in ("in", "out", "self") for w in ("weight", "bias")]
        live = [i for i, t in enumerate(Pd) if t is not None]
        full = lambda p: [p[live.index(i)] if i in live else None for i in range(6)]
        _both(lambda s, s_in, *p: OO.OPS[name](og, {k: v for k, v in zip(keys, full(p)) if v is not None}, s, s_in),
              lambda s, s_in, *p: R.dense_filter(kind, s, s_in, og.norm, b0, b1, full(p), self_scale), [s, s_in] + [Pd[i] for i in live], gout, name)
    for kind in ("mult", "sub", "add"):
        _both(lambda s, h: OO.OPS["pre_" + kind](og, {}, s, h), lambda s, h: R.compose(kind, s, h), [s, s_in], gout, "pre_" + kind)


@pytest.mark.parametrize("D", WIDTHS)
def test_reducer_restatements_are_the_oracle_reducers_and_std_ref64(D):
    from test_nc_gpu import std_ref64
    from mr_gnas_amd import graph as G
    src, dst, n_src, n = R.reducer_block(D)
    E = int(dst.numel())
    msg, selfr, gout = seeded("msg", (E, D), D), seeded("self", (n, D), D), seeded("g", (n, D), D)
    R.condition_max(msg, dst, n)
    for kind, fn in (("sum", OG.seg_sum), ("mean", OG.seg_mean), ("max", OG.seg_max)):
        _both(lambda m, sr: fn(m, dst, n) + sr, lambda m, sr: R.seg_reduce(kind, m, sr, dst, n), [msg, selfr], gout, "seg " + kind)
    blk = G.Block(torch.arange(n_src), torch.arange(n), src, dst, torch.arange(E))
    x64, ref = std_ref64(msg, blk)
    (gref,) = torch.autograd.grad(ref, x64, gout.double())
    # std_ref64 is a float64 statement, and E[x^2] - E[x]^2 evaluated in float32 loses a destination whose messages nearly agree
    # (5.9e-4 on this block's gradient): the restatement is held to it in float64, where the two are the same numbers
    m = msg.double().requires_grad_(True)
    own = R.seg_std(m, dst, n)
    assert float((own.detach() - ref.detach()).abs().max()) <= 1e-12 and float((torch.autograd.grad(own, m, gout.double())[0] - gref).abs().max()) <= 1e-9


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("D", WIDTHS)
def test_mixed_restatement_is_batchnorm_relu_weighted_sum(D, training):
    rows, K_ = 37, 3
    ys = [seeded(f"y{k}", (rows, D), D, 1.0 + k, 0.5 * k) for k in range(K_)]
    ys[1] = None
    bns = [torch.nn.BatchNorm1d(D) for _ in range(K_)]
    for k, bn in enumerate(bns):
        with torch.no_grad():
            bn.weight.copy_(seeded(f"gam{k}", (D,), D, 0.1, 1.0)); bn.bias.copy_(seeded(f"bet{k}", (D,), D, 0.3))
            bn.running_mean.copy_(seeded(f"rm{k}", (D,), D, 0.1)); bn.running_var.copy_(seeded(f"rv{k}", (D,), D, 0.1, 1.0).abs())
        bn.train(training)
    rm0, rv0 = [bn.running_mean.clone() for bn in bns], [bn.running_var.clone() for bn in bns]
    w, addend, gout = torch.softmax(seeded("w", (K_,), D), 0), seeded("add", (rows, D), D), seeded("g", (rows, D), D)
    for act, fn in (("relu", torch.relu), ("tanh", torch.tanh)):
        for bn, m, v in zip(bns, rm0, rv0):
            with torch.no_grad():
                bn.running_mean.copy_(m); bn.running_var.copy_(v)
        leaves = [y for y in ys if y is not None] + [w, addend]
        a = [t.clone().requires_grad_(True) for t in leaves]
        b = [t.clone().requires_grad_(True) for t in leaves]
        ref = a[3] + sum(a[2][k] * fn(bn(a[[0, None, 1][k]] if ys[k] is not None else torch.zeros(rows, D))) for k, bn in enumerate(bns))
        own = R.mixed([b[0], None, b[1]], [bn.weight for bn in bns], [bn.bias for bn in bns], b[2], b[3], act, training, rm0, rv0)
        close(own, ref.detach(), f"mixed {act} out")
        pa, pb = [p for bn in bns for p in (bn.weight, bn.bias)], [p for bn in bns for p in (bn.weight, bn.bias)]
        for i, (ga, gb) in enumerate(zip(torch.autograd.grad(ref, a + pa, gout), torch.autograd.grad(own, b + pb, gout))):
            close(gb, ga, f"mixed {act} grad {i}", rtol=3e-4, atol=1e-4)
        if training:
            for k in (0, 2):
                m, v = R.running_stats(ys[k], rm0[k], rv0[k])
                torch.testing.assert_close(m, bns[k].running_mean, rtol=1e-4, atol=1e-5)
                torch.testing.assert_close(v, bns[k].running_var, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("D", WIDTHS)
def test_cell_zero_restatement_is_the_mixed_one_over_the_compose_candidates(D):
    rows, N, Rn = 37, 20, 5
    gen = torch.Generator().manual_seed(D)
    ent, rel = seeded("ent", (N, D), D), seeded("rel", (Rn, D), D)
    ei, ri = torch.randint(0, N, (rows,), generator=gen), torch.randint(0, Rn, (rows,), generator=gen)
    gam, bet = [seeded(f"gam{k}", (D,), D, 0.1, 1.0) for k in range(3)], [seeded(f"bet{k}", (D,), D, 0.3) for k in range(3)]
    w, gout = torch.softmax(seeded("w", (3,), D), 0), seeded("g", (rows, D), D)
    kinds = ("mult", "sub", "add")
    ref_fn = lambda e, r: sum(w[k] * torch.relu(torch.nn.functional.batch_norm(OO.OPS["pre_" + kd](None, {}, e[ei], r[ri]), None, None, gam[k], bet[k], training=True))
                              for k, kd in enumerate(kinds))
    _both(ref_fn, lambda e, r: R.cell_zero(kinds, e, r, ei, ri, gam, bet, w), [ent, rel], gout, "cell zero")


# ---- the conditioning -------------------------------------------------------------------------------------------------------------------
def test_conditioning_reaches_its_margins():
    D, rows = 68, 200
    ys = [seeded(f"y{k}", (rows, D), 3, 1.0 + k) for k in range(2)]
    gam, bet = [seeded(f"gam{k}", (D,), 3, 0.1, 1.0).double() for k in range(2)], [seeded(f"bet{k}", (D,), 3, 0.3).double() for k in range(2)]
    args_of = lambda ts: [R.bn_arg(t.double(), gam[k], bet[k], True, None, None) for k, t in enumerate(ts)]
    before = min(R.relu_margin(z) for z in args_of(ys))
    after = R.condition_relu(ys, args_of, lambda k, bad: (k, bad), seed=3)
    assert before < R.RELU_MARGIN <= after and all(t.dtype == torch.float32 for t in ys)
    src, dst, n_src, n = R.reducer_block(5)
    msg = torch.round(seeded("msg", (int(dst.numel()), 4), 5) * 4) / 4        # quarter steps: ties everywhere
    assert R.max_gap(msg.double(), dst, n) == 0.0
    R.condition_max(msg, dst, n)
    assert R.max_gap(msg.double(), dst, n) >= R.MAX_GAP
