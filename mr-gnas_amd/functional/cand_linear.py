"""The candidate Linears of one node-classification MixedOp in one launch (csrc/cand_linear.hip; reference models/cell.py:17-31).

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h): every Function enqueues HIP kernels of
libmrgnas_hip.so on torch's current stream through ctypes; every call site states the algorithmic bytes / flops of the launch.

Every candidate of the reference's NC MixedOp is ``[op, Linear(D, D), BatchNorm1d, ReLU]``.  ``candidate_linears`` runs the Linears
of up to four candidates as one grouped launch (forward: ``mrg_cand_linear_fwd``, which also leaves the BatchNorm column sums of its
outputs; input gradient: ``mrg_cand_linear_bwd_input``) and hands ``Candidate("stored", y_k, sums=...)`` to the MixedOp epilogue.
Weight and bias gradients stay on ``mrg_linear_bwd_weight``, one launch per candidate.  A shape the grouped kernel does not cover
(``mrg_cand_linear_colsum_blocks(rows, D) == 0``: D % 4 != 0 or D outside 16..128), an operand that is not 16-byte aligned, or
``switches.CAND_LINEAR_GROUP`` off runs ``linear`` per candidate."""
import torch

from .. import _lib
from .._lib import call, f32c, ptr, ptr_array, require_hip, stream_of
from . import switches as SW
from ._base import _ws, _ws_bytes
from .candidates import Candidate, wants_stats
from .row_linear import linear

GROUP_MAX = 4              # members of one launch (csrc/cand_linear.hip: CAND_MAX)


def _blocks(rows, D):
    return _ws_bytes("mrg_cand_linear_colsum_blocks", rows, D)


def grouped_ok(rows, D, tensors):
    """Does the grouped kernel take this shape and these operands?"""
    return rows > 0 and _blocks(rows, D) > 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


class _CandLinears(torch.autograd.Function):
    """(y_0 .. y_{n-1}) = (x_k W_k^T + b_k) for n <= 4 members in one launch.  box: None, or a list that receives the members'
    _lib.ColSums (the column sums of y_k, formed by the launch)."""

    @staticmethod
    def forward(ctx, box, n, *tensors):
        xs = [f32c(t) for t in tensors[:n]]
        Ws = [f32c(t) for t in tensors[n:2 * n]]
        bs = [f32c(t) for t in tensors[2 * n:3 * n]]
        require_hip(*xs, *Ws, *bs)
        rows, D = xs[0].shape
        for x, W in zip(xs, Ws):
            if tuple(x.shape) != (rows, D) or tuple(W.shape) != (D, D):
                raise _lib.MrgnasError(f"candidate linears: members of [{rows}, {D}] rows with [{D}, {D}] weights expected, got "
                                       f"{tuple(x.shape)} and {tuple(W.shape)}")
        dev, st = xs[0].device, stream_of(xs[0])
        ys = [torch.empty(rows, D, dtype=torch.float32, device=dev) for _ in range(n)]
        ws = _ws(_ws_bytes("mrg_cand_linear_workspace_bytes", n, D), xs[0])
        blocks = _blocks(rows, D) if box is not None else 0
        sums = torch.empty(n * blocks * 2 * D * 8, dtype=torch.uint8, device=dev) if blocks else None
        call("mrg_cand_linear_fwd", (n, ptr_array(xs), ptr_array(Ws), ptr_array(bs), ptr_array(ys), ptr(ws), rows, D, st, ptr(sums), blocks),
             nbytes=4 * rows * D * 2 * n + 4 * n * D * D, flops=2 * rows * D * D * n)
        if blocks:
            box.extend(_lib.ColSums(sums, k * blocks * 2 * D * 8, blocks, 2 * D, rows) for k in range(n))
        ctx.n, ctx.has_b = n, [b is not None for b in bs]
        ctx.save_for_backward(*xs, *Ws)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        n = ctx.n
        saved = ctx.saved_tensors
        xs, Ws = saved[:n], saved[n:]
        gys = [f32c(g) for g in gys]
        require_hip(*gys)
        rows, D = xs[0].shape
        st = stream_of(xs[0])
        gxs, gWs, gbs = [None] * n, [None] * n, [None] * n
        need_x = [k for k in range(n) if ctx.needs_input_grad[2 + k]]
        if need_x:
            for k in need_x:
                gxs[k] = torch.empty_like(xs[k])
            m = len(need_x)
            ws = _ws(_ws_bytes("mrg_cand_linear_workspace_bytes", m, D), xs[0])
            call("mrg_cand_linear_bwd_input", (m, ptr_array([gys[k] for k in need_x]), ptr_array([Ws[k] for k in need_x]),
                                               ptr_array([gxs[k] for k in need_x]), ptr(ws), rows, D, st),
                 nbytes=4 * rows * D * 2 * m + 4 * m * D * D, flops=2 * rows * D * D * m)
        for k in range(n):
            need_b = ctx.has_b[k] and ctx.needs_input_grad[2 + 2 * n + k]
            if not (ctx.needs_input_grad[2 + n + k] or need_b):
                continue
            gWs[k] = torch.empty_like(Ws[k])
            gbs[k] = torch.empty(D, dtype=torch.float32, device=xs[k].device) if ctx.has_b[k] else None
            ws = _ws(_ws_bytes("mrg_linear_bwd_weight_workspace_bytes", rows, D, D), xs[k])
            call("mrg_linear_bwd_weight", (ptr(gys[k]), ptr(xs[k]), None, ptr(gWs[k]), ptr(gbs[k]), ptr(ws), rows, D, 0, D, st),
                 nbytes=4 * rows * 2 * D + 4 * D * D, flops=2 * rows * D * D)
        return (None, None, *gxs, *gWs, *gbs)


class _BiasRows(torch.autograd.Function):
    """The Linear of an f_zero candidate: Linear(0 * x) = bias on every row, stored as [rows, D].  The weight's gradient is a zero
    tensor (the reference's x^T g with x = 0), not None: SGD with weight decay treats the two differently."""

    @staticmethod
    def forward(ctx, W, b, rows):
        ctx.save_for_backward(W)
        return b.detach().to(torch.float32).expand(rows, b.shape[0]).contiguous()

    @staticmethod
    def backward(ctx, g):
        (W,) = ctx.saved_tensors
        return torch.zeros_like(W), g.sum(0), None


def constant_candidate(lin, rows):
    """The candidate of an operator whose output is zero on every row (f_zero): the Linear's bias, [rows, D]."""
    if lin.bias is None:
        raise _lib.MrgnasError("constant candidate: the Linear has no bias (the candidate would be absent)")
    return Candidate("stored", _BiasRows.apply(lin.weight, lin.bias, rows))


def candidate_linears(xs, linears, for_epilogue=None):
    """[Candidate("stored", Linear_k(xs[k]))] for the candidates of one MixedOp: xs[k] is the k-th operator's output [rows, D] (all
    of the same rows), or None for an operator whose output is zero (f_zero: the candidate is the Linear's bias on every row).
    The candidates carry their BatchNorm column sums exactly when wants_stats(for_epilogue) and the grouped kernel ran."""
    live = [k for k, x in enumerate(xs) if x is not None]
    if not live:
        raise _lib.MrgnasError("candidate linears: at least one operator output is needed to know the row count")
    rows, D = xs[live[0]].shape
    out = [None] * len(xs)
    for k, x in enumerate(xs):
        if x is None:
            out[k] = constant_candidate(linears[k], rows)
    operands = [t for k in live for t in (xs[k], linears[k].weight, linears[k].bias)]
    if not (SW.CAND_LINEAR_GROUP and grouped_ok(rows, D, operands) and all(x.dtype == torch.float32 and x.is_contiguous() for x in (xs[k] for k in live))):
        for k in live:
            out[k] = Candidate("stored", linear(xs[k], linears[k].weight, linears[k].bias))
        return out
    for i in range(0, len(live), GROUP_MAX):
        part = live[i:i + GROUP_MAX]
        box = [] if wants_stats(for_epilogue) else None
        ys = _CandLinears.apply(box, len(part), *[xs[k] for k in part], *[linears[k].weight for k in part], *[linears[k].bias for k in part])
        for j, k in enumerate(part):
            out[k] = Candidate("stored", ys[j], sums=box[j] if box else None)
    return out
