"""The "dot" sweeps under a per-entity score bias (csrc/bce.hip, rank.hip, topk.hip: mrg_rows_bias_*, mrg_cols_sum; functional.rows_bce_all,
evaluation.query_ranks / query_topk with bias=; compgcn.CompGCN_ConvE.loss_1n) without a GPU: the entry points exist and the ABI number
stays, the old workspace queries answer what they answered, argument errors come back before any launch, nothing falls back to the
CPU, the module gains the scorer protocol without a new state_dict key, and the new kernel instances use no scratch memory."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import load_golden, sub
from mr_gnas_amd import _lib, compgcn as CG, evaluation as EV, functional as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
NEW = ("mrg_rows_bias_bce_fwd", "mrg_rows_bias_bce_dlogit", "mrg_rows_bias_rank", "mrg_rows_bias_topk", "mrg_cols_sum")
E_NULLPTR, E_SHAPE, E_WORKSPACE = -1, -2, -4


def test_the_entry_points_are_declared_and_the_abi_stays():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 23 and lib.mrg_abi_version() == 23


def test_the_old_workspace_queries_answer_what_they_answered():
    """The biased entry points share their twins' workspaces, and the twins' plans did not move.  The numbers were read from the
    library built at the parent commit (same compiler, on the CPU: the queries launch nothing)."""
    lib = _lib.load()
    shapes = [(8, 100, 64), (1024, 14541, 200), (257, 449, 50), (8197, 33, 4), (5, 28705, 52), (256, 1000000, 256)]
    parent = {"mrg_distmult_bce_workspace_bytes": [86784, 18183680, 2816, 66816, 11011840, 44114176],
              "mrg_distmult_rank_workspace_bytes": [140288, 21112064, 110080, 459776, 11148800, 1537169664],
              "mrg_rows_topk_workspace_bytes": [87296, 23512320, 66304, 786944, 11061760, 46665984]}
    for name, want in parent.items():
        extra = (10,) if "topk" in name else ()
        assert [getattr(lib, name)(*s, *extra) for s in shapes] == want, name


def _fwd(lib, q=P(256), ent=P(256), bias=P(256), qkey=P(256), keys=P(256), rowptr=P(256), objs=P(256), U=3, B=8, N=100, D=64,
         loss=P(256), ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_rows_bias_bce_fwd(q, ent, bias, qkey, keys, rowptr, objs, U, 0.0, 1.0, B, N, D, loss, ws, ws_bytes, None)


def _dlogit(lib, q=P(256), ent=P(256), bias=P(256), qkey=P(256), keys=P(256), rowptr=P(256), objs=P(256), U=3, B=8, N=100, D=64, c0=0,
            c1=100, gscale=P(256), dl=P(256), ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_rows_bias_bce_dlogit(q, ent, bias, qkey, keys, rowptr, objs, U, 0.0, 1.0, B, N, D, c0, c1, gscale, dl, ws, ws_bytes,
                                        None)


def _rank(lib, q=P(256), ent=P(256), bias=P(256), t_idx=P(256), qkey=P(256), when=P(256), keys=P(256), rowptr=P(256), members=P(256),
          gone_at=P(256), U=3, B=8, N=100, D=64, ranks=P(256), ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_rows_bias_rank(q, ent, bias, t_idx, qkey, when, keys, rowptr, members, gone_at, U, B, N, D, ranks, ws, ws_bytes, None)


def _topk(lib, q=P(256), ent=P(256), bias=P(256), qkey=P(256), when=P(256), keys=P(256), rowptr=P(256), members=P(256), gone_at=P(256),
          U=3, B=8, N=100, D=64, k=10, ids=P(256), vals=P(256), ws=P(256), ws_bytes=1 << 40):
    return lib.mrg_rows_bias_topk(q, ent, bias, qkey, when, keys, rowptr, members, gone_at, U, B, N, D, k, ids, vals, ws, ws_bytes, None)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    needs = {_fwd: lib.mrg_distmult_bce_workspace_bytes(8, 100, 64), _dlogit: lib.mrg_distmult_bce_workspace_bytes(8, 100, 64),
             _rank: lib.mrg_distmult_rank_workspace_bytes(8, 100, 64), _topk: lib.mrg_rows_topk_workspace_bytes(8, 100, 64, 10)}
    required = {_fwd: ("q", "ent", "bias", "loss"), _dlogit: ("q", "ent", "bias", "gscale", "dl"), _rank: ("q", "ent", "bias", "t_idx", "ranks"),
                _topk: ("q", "ent", "bias", "ids", "vals")}
    for fn, n in needs.items():
        for name in required[fn]:                                         # the bias is required: no NULL-means-none in these entry points
            assert fn(lib, **{name: None}) == E_NULLPTR, (fn.__name__, name)
        assert fn(lib, D=0) == E_SHAPE and fn(lib, D=1028) == E_SHAPE and fn(lib, D=257) == E_SHAPE and fn(lib, N=0) == E_SHAPE
        assert fn(lib, B=-1) == E_SHAPE and fn(lib, U=-1) == E_SHAPE and fn(lib, bias=None, D=0) == E_SHAPE
        assert n > 0 and fn(lib, ws=None) == E_WORKSPACE and fn(lib, ws_bytes=n - 1) == E_WORKSPACE
        assert fn(lib, B=0, q=None, ent=None, bias=None, ws=None, ws_bytes=0) == 0       # nothing to do, nothing launched
    assert _dlogit(lib, c0=-1) == E_SHAPE and _dlogit(lib, c0=10, c1=10) == E_SHAPE and _dlogit(lib, c1=101) == E_SHAPE
    assert _topk(lib, k=0) == E_SHAPE and _topk(lib, k=65) == E_SHAPE
    cols = lib.mrg_cols_sum
    assert cols(P(256), -1, 4, 4, P(256), None) == E_SHAPE and cols(P(256), 4, -1, 4, P(256), None) == E_SHAPE
    assert cols(P(256), 4, 8, 7, P(256), None) == E_SHAPE                                 # a leading dimension below the width
    assert cols(None, 4, 8, 8, P(256), None) == E_NULLPTR and cols(P(256), 4, 8, 8, None, None) == E_NULLPTR
    assert cols(None, 4, 0, 0, None, None) == 0


class _Index:
    """What the Python-side checks read of a sampler.LabelIndex before they reach a device."""
    num_ent, num_rel = 12, 3

    def label_values(self, label_smooth=0.0):
        return 0.0, 1.0


def test_python_side_errors_come_before_any_device_check():
    q, ent, bias = torch.zeros(4, 8), torch.zeros(12, 8), torch.zeros(12)
    subj = rel = torch.zeros(4, dtype=torch.long)
    target = torch.zeros(4, dtype=torch.long)
    # a bias is defined for "dot" scorers only: ValueError on CPU tensors, i.e. before the device is looked at
    with pytest.raises(ValueError, match='"dot" scorers only'):
        K.rows_bce_all("l1", 40.0, ent, q, _Index(), subj, rel, bias=bias)
    with pytest.raises(ValueError, match='"dot" scorers only'):
        EV.query_ranks(q, ent, target, kind="l1", bias=bias)
    with pytest.raises(ValueError, match='"dot" scorers only'):
        EV.query_topk(q, ent, 3, kind="l1", bias=bias)
    # a bias of the wrong length, or not a vector
    for bad in (torch.zeros(11), torch.zeros(12, 1)):
        with pytest.raises(ValueError, match="bias"):
            K.rows_bce_all("dot", None, ent, q, _Index(), subj, rel, bias=bad)
        with pytest.raises(ValueError, match="bias"):
            K.dot_bce_all(ent, q, _Index(), subj, rel, bias=bad)
        with pytest.raises(ValueError, match="bias"):
            EV.query_ranks(q, ent, target, bias=bad)
        with pytest.raises(ValueError, match="bias"):
            EV.query_topk(q, ent, 3, bias=bad)
    # a well-formed call on CPU tensors: no CPU fallback
    with pytest.raises(_lib.MrgnasError):
        K.rows_bce_all("dot", None, ent, q, _Index(), subj, rel, bias=bias)
    with pytest.raises(_lib.MrgnasError):
        EV.query_ranks(q, ent, target, bias=bias)
    with pytest.raises(_lib.MrgnasError):
        EV.query_topk(q, ent, 3, bias=bias)


def _net(z):
    net = CG.CompGCN_ConvE(z["nb"], 2 * z["R"], z["N"], z["Din"], [z["Dout"]], comp_fn="sub", dropout=0.0, layer_dropout=[0.0],
                           num_filt=z["F"], hid_drop=0.0, feat_drop=0.0, ker_sz=z["ks"], k_w=z["k_w"], k_h=z["k_h"])
    net.load_state_dict(sub(z, "param0/"))
    return net


def test_compgcn_conve_follows_the_scorer_protocol_without_new_state():
    z = load_golden("compgcn_conve_1n")
    net = _net(z)
    assert sorted(net.state_dict()) == sorted(sub(z, "param0/"))                      # the reference's keys, nothing added
    assert sorted(n for n, _ in net.named_parameters()) == sorted(sub(z, "gparam/"))
    assert callable(net.embed) and callable(net.query) and callable(net.loss_1n)
    assert net.score_kind == "dot" and net.score_func is net and net.score_bias is net.bias
    assert sum(1 for _ in net.modules()) == sum(1 for _ in _net(z).modules()) and net not in list(net.children())
    # the fixture is what its generator promises: distinct keys, both directions, labels that LabelIndex can rebuild from the triples
    keys = {(int(s), int(r)) for s, r in zip(z["subj"], z["rel"])}
    assert len(keys) == z["subj"].numel() and int((z["rel"] >= z["R"]).sum()) >= 1 and int((z["rel"] < z["R"]).sum()) >= 1
    known = {}
    for s, r, o in z["triples"].tolist():
        known.setdefault((s, r), set()).add(o)
        known.setdefault((o, r + z["R"]), set()).add(s)
    y = torch.zeros(len(keys), z["N"])
    for i, (s, r) in enumerate(zip(z["subj"].tolist(), z["rel"].tolist())):
        y[i, sorted(known[(s, r)])] = 1.0
    ls = float(z["label_smooth"])
    assert torch.equal((1.0 - ls) * y + (1.0 / z["N"]), z["label"])
    assert all(torch.unique(row).numel() == z["N"] for row in z["pred_eval"])         # no ties in the expected ranks


def test_loss_1n_has_no_cpu_fallback():
    z = load_golden("compgcn_conve_1n")
    net = _net(z)
    with pytest.raises(_lib.MrgnasError, match="no CPU"):
        net.loss_1n(None, z["subj"], z["rel"], _Index())
    with pytest.raises(_lib.MrgnasError, match="no CPU"):
        net.query(torch.zeros(7, z["Dout"]), torch.zeros(7, z["Dout"]))


def test_the_biased_kernel_instances_use_no_scratch():
    """Every instance the bias adds -- the four epilogue kinds 14-17 on both cores, the column sums and the target-score add -- compiles
    for gfx950 without scratch memory and without register spills to it (the resource-usage remarks, as
    test_host_cpu.py::test_async_fill_kernels_do_not_spill reads them)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mr-gnas_amd", "csrc")
    seen = set()
    for unit in ("bce.hip", "rank.hip", "topk.hip"):
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                              "--cuda-device-only", "-c", os.path.join(csrc, unit), "-o", os.devnull],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        name = None
        for line in out.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                continue
            new = name and (re.search(r"rowgemm_(x3s_k|k)I.*Li1[4-7]ELb[01]E", name) or "cols_sum_k" in name or "rank_bias_tscore_k" in name)
            m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
            if m and new:
                assert int(m.group(2)) == 0, f"{name}: {m.group(1)} {m.group(2)}"
                seen.add(name)
    kinds = {(re.search(r"rowgemm_(x3s_k|k)I", n).group(1), int(re.search(r"Li(1[4-7])ELb", n).group(1))) for n in seen if "rowgemm" in n}
    assert kinds == {(core, epi) for core in ("x3s_k", "k") for epi in (14, 15, 16, 17)}, kinds
    assert len(seen) == 4 * 3 + 2, sorted(seen)             # per kind: the split core, the exact core with vectorised and with plain loads
