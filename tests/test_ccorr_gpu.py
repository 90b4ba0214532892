"""Standalone circular correlation on the MI355X (csrc/ccorr.hip, functional/ccorr.py): ccorr(a, b)[k] = sum_j a[j] b[(j + k) % D]
(reference utils/utils.py:285-301, models/operations_lp.py:58-68) and its gradients against float64, on both paths (the per-row
kernel and a shared row's circulant on the row GEMM), bit-reproducibility, graph capture, input handling and pre_corr_op inside a
MixedOp."""
import importlib

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DS = [1, 7, 10, 100, 200, 256, 300, 512]
NS = [0, 1, 33, 4097]


def ref_fft(a, b):
    """float64 on the host: irfft(conj(rfft(a)) * rfft(b), n=D) -- the reference's definition on today's torch.fft."""
    D = a.shape[-1]
    if a.numel() == 0 or b.numel() == 0:                    # (the host FFT refuses an empty batch)
        return ref_direct(a, b)
    return torch.fft.irfft(torch.conj(torch.fft.rfft(a, dim=-1)) * torch.fft.rfft(b, dim=-1), n=D, dim=-1)


def ref_direct(a, b):
    """float64 on the host: the double sum c[k] = sum_j a[j] b[(j + k) % D]."""
    D = a.shape[-1]
    idx = (torch.arange(D)[None, :] + torch.arange(D)[:, None]) % D        # idx[k, j] = (j + k) % D
    return (a.unsqueeze(-2) * b[..., idx]).sum(-1)


def shapes(N, D):
    return {
        "rows": ((N, D), (N, D)),
        "shared_b": ((N, D), (1, D)),
        "shared_b_1d": ((N, D), (D,)),
        "shared_a": ((1, D), (N, D)),
        "outer": ((N, 1, D), (1, 2, D)),
    }


def rows_of(shape):
    n = 1
    for s in shape[:-1]:
        n *= s
    return n


def max_err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max()) if ref.numel() else 0.0


def scale(ref):
    return float(ref.abs().max()) if ref.numel() else 0.0


def run_case(sa, sb, seed, check=True):
    from mr_gnas_amd import functional as K
    gen = torch.Generator().manual_seed(seed)
    a64 = torch.randn(*sa, generator=gen, dtype=torch.float64)
    b64 = torch.randn(*sb, generator=gen, dtype=torch.float64)
    a64.requires_grad_(check)
    b64.requires_grad_(check)
    full = tuple(torch.broadcast_shapes(sa[:-1], sb[:-1])) + (sa[-1],)
    g64 = torch.randn(full, generator=gen, dtype=torch.float64)
    if check:
        ref = ref_fft(a64, b64)
        ref.backward(g64)
    a = a64.detach().float().to(DEV).requires_grad_(True)
    b = b64.detach().float().to(DEV).requires_grad_(True)
    out = K.ccorr(a, b)
    out.backward(g64.float().to(DEV))
    torch.cuda.synchronize()
    assert tuple(out.shape) == full and out.dtype == torch.float32
    assert a.grad.shape == a.shape and b.grad.shape == b.shape
    if check:
        N = rows_of(full)
        r = ref.detach()
        assert max_err(out, r) <= 1e-5 * scale(r), ("forward", sa, sb)
        for name, got, want, n in (("da", a.grad, a64.grad, rows_of(sa)), ("db", b.grad, b64.grad, rows_of(sb))):
            tol = 1e-4 if n < N else 1e-5                  # the gradient of a shared row sums over all rows
            assert max_err(got, want) <= tol * scale(want), (name, sa, sb, max_err(got, want), scale(want))
    return out, a.grad, b.grad


def test_references_agree():
    gen = torch.Generator().manual_seed(1)
    for D in DS:
        a = torch.randn(5, D, generator=gen, dtype=torch.float64)
        b = torch.randn(5, D, generator=gen, dtype=torch.float64)
        d, f = ref_direct(a, b), ref_fft(a, b)
        assert float((d - f).abs().max()) <= 1e-10 * max(1.0, float(d.abs().max())), D


@pytest.mark.parametrize("D", DS)
def test_forward_and_gradients_vs_float64(D):
    for N in NS:
        for i, (sa, sb) in enumerate(shapes(N, D).values()):
            run_case(sa, sb, seed=1000 * D + 10 * N + i)


@pytest.mark.parametrize("N", [70_000, 544_230])
def test_paths_agree(monkeypatch, N):
    from mr_gnas_amd.functional import switches as SW
    D = 200
    for sa, sb in (((N, D), (1, D)), ((1, D), (N, D))):
        res = {}
        for path in ("rows", "matrix"):
            monkeypatch.setattr(SW, "CCORR_PATH", path)
            res[path] = run_case(sa, sb, seed=N, check=N <= 70_000)
        for k, (x, y) in enumerate(zip(res["rows"], res["matrix"])):
            shared = k > 0 and rows_of((sa, sb)[k - 1]) == 1
            tol = 1e-4 if shared else 1e-5
            x, y = x.detach(), y.detach()
            assert float((x - y).abs().max()) <= tol * float(x.abs().max()), (k, sa, sb)


def _step(a, b):
    from mr_gnas_amd import functional as K
    a = a.detach().requires_grad_(True)                     # a leaf with a's strides and dtype
    b = b.detach().requires_grad_(True)
    out = K.ccorr(a, b)
    out.backward(torch.cos(out.detach()))
    return out.detach(), a.grad, b.grad


@pytest.mark.parametrize("path", ["rows", "matrix"])
def test_bit_reproducible(monkeypatch, path):
    from mr_gnas_amd.functional import switches as SW
    monkeypatch.setattr(SW, "CCORR_PATH", path)
    gen = torch.Generator(device=DEV).manual_seed(3)
    N, D = 70_000, 200
    a = torch.randn(N, D, device=DEV, generator=gen)
    for b in (torch.randn(N, D, device=DEV, generator=gen), torch.randn(1, D, device=DEV, generator=gen)):
        first, second = _step(a, b), _step(a, b)
        for x, y in zip(first, second):
            assert torch.equal(x, y)
        first, second = _step(b, a), _step(b, a)
        for x, y in zip(first, second):
            assert torch.equal(x, y)


@pytest.mark.parametrize("shared", [False, True])
def test_capturable(shared):
    from mr_gnas_amd import functional as K
    C = importlib.import_module("mr_gnas_amd.functional.ccorr")     # the package re-exports the function under the same name
    gen = torch.Generator(device=DEV).manual_seed(4)
    N, D = max(C.MATRIX_MIN_ROWS, 8192), 200
    a = torch.randn(N, D, device=DEV, generator=gen)
    b = torch.randn(1 if shared else N, D, device=DEV, generator=gen)
    eager = K.ccorr(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.ccorr(a, b)                                       # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.ccorr(a, b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_noncontiguous_and_other_dtypes():
    gen = torch.Generator(device=DEV).manual_seed(5)
    N, D = 1000, 100
    base_a = torch.randn(D, 2 * N, device=DEV, generator=gen)
    base_b = torch.randn(N, D, device=DEV, generator=gen, dtype=torch.float64)
    cases = [
        (base_a.t()[::2], base_b),                          # strided rows, float64
        (base_a.t()[:N].half(), base_b.t().contiguous().t()[:, :]),
        (base_a[:, :N].t(), base_b[:1]),                    # a shared float64 row
    ]
    for a, b in cases:
        assert not (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype == torch.float32)
        got = _step(a, b)
        want = _step(a.float().contiguous(), b.float().contiguous())
        assert got[0].dtype == torch.float32 and torch.equal(got[0], want[0])
        assert torch.equal(got[1].float(), want[1].to(got[1].dtype).float())
        assert torch.equal(got[2].float(), want[2].to(got[2].dtype).float())


def test_pre_corr_op_in_a_mixed_op(monkeypatch):
    """MixedOp(["pre_corr", "pre_sub"]) against a float64 restatement of reference models/cell_lp.py:25-33
    (BatchNorm -> ReLU -> w * . -> sum): pre_corr_op is not a _PreOp, so it takes the generic fused path."""
    from mr_gnas_amd import cell_lp as CL, operations_lp as OPS
    monkeypatch.setitem(OPS.MIXED_OPS, "pre_corr", lambda args: OPS.pre_corr_op())
    N, D = 5000, 200
    gen = torch.Generator().manual_seed(6)
    h64 = torch.randn(N, D, generator=gen, dtype=torch.float64)
    hr64 = torch.randn(N, D, generator=gen, dtype=torch.float64)
    w64 = torch.rand(2, generator=gen, dtype=torch.float64)
    gamma = 1 + 0.1 * torch.randn(2, D, generator=gen, dtype=torch.float64)
    beta = 0.1 * torch.randn(2, D, generator=gen, dtype=torch.float64)
    gout = torch.randn(N, D, generator=gen, dtype=torch.float64)

    mop = CL.MixedOp(D, 0.0, ["pre_corr", "pre_sub"]).to(DEV)
    with torch.no_grad():
        for k in range(2):
            mop._ops[k][1].weight.copy_(gamma[k])
            mop._ops[k][1].bias.copy_(beta[k])
    h = h64.float().to(DEV).requires_grad_(True)
    hr = hr64.float().to(DEV).requires_grad_(True)
    w = w64.float().to(DEV).requires_grad_(True)
    out = mop(w, None, h, hr)
    out.backward(gout.float().to(DEV))
    torch.cuda.synchronize()

    ph, phr, pw = (t.clone().requires_grad_(True) for t in (h64, hr64, w64))
    pg, pb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ys = [ref_fft(ph, phr), ph - phr]
    ref = 0
    for k, y in enumerate(ys):
        mu = y.mean(0)
        var = y.var(0, unbiased=False)
        ref = ref + pw[k] * torch.relu((y - mu) / torch.sqrt(var + 1e-5) * pg[k] + pb[k])
    ref.backward(gout)

    torch.testing.assert_close(out.detach().double().cpu(), ref.detach(), rtol=1e-4, atol=2e-5)
    bns = [mop._ops[k][1] for k in range(2)]
    pairs = [(h.grad, ph.grad), (hr.grad, phr.grad), (w.grad, pw.grad)]
    pairs += [(torch.stack([bn.weight.grad for bn in bns]), pg.grad), (torch.stack([bn.bias.grad for bn in bns]), pb.grad)]
    for got, want in pairs:
        assert max_err(got, want) <= 5e-4 * scale(want), (max_err(got, want), scale(want))


def test_pre_corr_op_forward():
    """pre_corr_op()(g, src_emb, hr) = ccorr(src_emb, hr.expand_as(src_emb)) (reference models/operations_lp.py:63-68), through its
    lazy handle when handles are on, with a relation row broadcast over the rows."""
    from mr_gnas_amd import functional as K, lazy as LZ, operations_lp as OPS
    gen = torch.Generator(device=DEV).manual_seed(7)
    h = torch.randn(3000, 200, device=DEV, generator=gen)
    for hr in (torch.randn(3000, 200, device=DEV, generator=gen), torch.randn(1, 200, device=DEV, generator=gen)):
        got = LZ.real(OPS.pre_corr_op()(None, h, hr))
        assert torch.equal(got, K.ccorr(h, hr.expand_as(h)))
        assert tuple(got.shape) == tuple(h.shape)
