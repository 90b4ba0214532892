"""Standalone circular correlation ccorr(a, b) and its gradients (csrc/ccorr.hip; reference utils/utils.py:285-301,
models/operations_lp.py:58-68).

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h): every Function enqueues HIP kernels of
libmrgnas_hip.so on torch's current stream through ctypes; every call site states the algorithmic bytes / flops of the launch.

    ccorr(a, b)[k] = sum_j a[j] * b[(j + k) % D]       (= irfft(conj(rfft(a)) * rfft(b), n=D))
    dL/da = ccorr(g, b),   dL/db = cconv(a, g),   cconv(x, y)[m] = sum_j x[j] * y[(m - j) % D]

Two paths:
  rows    mrg_ccorr_rows: O(D^2) multiply-adds per pair of rows on the f32 vector pipe, forward and both gradients;
  matrix  one operand is a single row shared by every row of the other: ccorr(a, b) = a @ H(b)^T, H[k, j] = b[(j + k) % D], or
          ccorr(a, b) = b @ T(a)^T, T[k, m] = a[(m - k) % D] -- mrg_ccorr_matrix builds the D x D circulant, ``linear`` (the split-core
          row GEMM) multiplies, and linear's weight gradient is folded back onto the shared row by mrg_ccorr_matrix_grad.
"""
import torch

from .. import _lib
from .. import lazy as LZ
from .._lib import call, f32c, ptr, require_hip, stream_of
from . import switches as SW
from .row_linear import linear

CORR, CONV = 0, 1              # MRG_CCORR / MRG_CCONV
SHARED_B, SHARED_A = 0, 1      # MRG_CCORR_H / MRG_CCORR_T
MAX_D = 512                    # MRG_CCORR_MAX_D

# Below this many rows a shared-row product stays on the per-row kernel (the operand expanded): both forms are launch-bound there and
# the matrix path pays the circulant build and the GEMM's split-weight pass.  Measured with tools/ccorr_bench.py.
MATRIX_MIN_ROWS = 32768


def matrix_ok(D):
    """Widths the matrix path takes: those the row GEMM runs on its split core (K % 4 == 0, K > 48)."""
    return D % 4 == 0 and D > 48


def _rows(mode, x, y):
    N, D = x.shape
    out = torch.empty(N, D, dtype=torch.float32, device=x.device)
    call("mrg_ccorr_rows", (mode, ptr(x), ptr(y), ptr(out), N, D, stream_of(x)), nbytes=12 * N * D, flops=2 * N * D * D)
    return out


class _CCorrRows(torch.autograd.Function):
    """out[i] = ccorr(a[i], b[i]) over [N, D] rows."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _rows(CORR, a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = f32c(g)
        require_hip(g)
        da = _rows(CORR, g, b) if ctx.needs_input_grad[0] else None
        db = _rows(CONV, a, g) if ctx.needs_input_grad[1] else None
        return da, db


class _Circulant(torch.autograd.Function):
    """The D x D matrix of a shared row r: H(r) (SHARED_B) or T(r) (SHARED_A); backward folds the matrix gradient onto r."""

    @staticmethod
    def forward(ctx, r, mode):
        D = r.shape[0]
        W = torch.empty(D, D, dtype=torch.float32, device=r.device)
        call("mrg_ccorr_matrix", (mode, ptr(r), ptr(W), D, stream_of(r)), nbytes=4 * (D * D + D))
        ctx.mode = mode
        return W

    @staticmethod
    def backward(ctx, gW):
        gW = f32c(gW)
        require_hip(gW)
        D = gW.shape[0]
        gr = torch.empty(D, dtype=torch.float32, device=gW.device)
        call("mrg_ccorr_matrix_grad", (ctx.mode, ptr(gW), ptr(gr), D, stream_of(gW)), nbytes=4 * (D * D + D), flops=D * D)
        return gr, None


def _real(x):
    if isinstance(x, torch.Tensor) and not isinstance(x, LZ.Lazy):
        return x
    from .compose_gather import LazyRows
    if isinstance(x, LazyRows):
        return x.materialize()
    return LZ.real(x)


def _use_matrix(N, D):
    if not matrix_ok(D) or N == 0:
        return False
    if SW.CCORR_PATH is not None:
        return SW.CCORR_PATH == "matrix"
    return N >= MATRIX_MIN_ROWS


def ccorr(a, b):
    """Circular correlation of the rows of a [..., D] and b [..., D] (leading dims broadcast as in torch), float32 [..., D].

    Equal row counts run on the per-row kernel; a single row of one operand against N rows of the other on the matrix path from
    MATRIX_MIN_ROWS rows on (``switches.CCORR_PATH`` forces either); any other broadcast runs on expanded rows and its gradients are
    summed back to the operands' shapes."""
    a, b = _real(a), _real(b)
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.dim() == 0 or b.dim() == 0:
        raise _lib.MrgnasError("ccorr: operands must be tensors of shape [..., D]")
    D = a.shape[-1]
    if b.shape[-1] != D:
        raise _lib.MrgnasError(f"ccorr: row widths differ ({D} vs {b.shape[-1]})")
    if not 1 <= D <= MAX_D:
        raise _lib.MrgnasError(f"ccorr: row width {D} outside 1 .. {MAX_D}")
    a, b = f32c(a), f32c(b)
    require_hip(a, b)
    la, lb = tuple(a.shape[:-1]), tuple(b.shape[:-1])
    try:
        lead = tuple(torch.broadcast_shapes(la, lb))
    except RuntimeError as e:
        raise _lib.MrgnasError(f"ccorr: shapes {tuple(a.shape)} and {tuple(b.shape)} do not broadcast") from e
    N = 1
    for n in lead:
        N *= n
    Na, Nb = a.numel() // D, b.numel() // D
    full = lead + (D,)
    if la == lead and lb == lead:
        return _CCorrRows.apply(a.reshape(N, D), b.reshape(N, D)).reshape(full)
    if la == lead and Nb == 1 and _use_matrix(N, D):
        return linear(a.reshape(N, D), _Circulant.apply(b.reshape(D), SHARED_B)).reshape(full)
    if lb == lead and Na == 1 and _use_matrix(N, D):
        return linear(b.reshape(N, D), _Circulant.apply(a.reshape(D), SHARED_A)).reshape(full)
    # any other broadcast: both operands as [N, D] rows; autograd's expand sums each gradient back (sum_to_size)
    ae = a if la == lead else a.expand(full)
    be = b if lb == lead else b.expand(full)
    return _CCorrRows.apply(ae.reshape(N, D).contiguous(), be.reshape(N, D).contiguous()).reshape(full)
