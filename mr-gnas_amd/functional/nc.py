"""Node-classification aggregators on a block (graph.Block: E edge rows in, n_dst destination rows out, NO self rows): a_std
(csrc/segstd.hip) and the forms of a_sum / a_mean / a_max without the residual self rows (reference models/operations.py:109-190).

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h).  The reducers without self rows are the
existing entry points called with ``self_rows = NULL``: a_sum is ``seg_reduce`` (span kernel), a_max / a_mean are
``linear_relu_partial`` (the fused ReLU(Linear) + segmented max / run-sum GEMM where the shape takes it), a_mean scaled by the
inverse in-degree."""
import torch

from .. import _lib
from .._lib import call, f32c, ptr, require_hip, stream_of
from ._base import _chunk_plan_args
from .reducers import ORDERED_BWD_MIN_BYTES, linear_relu_partial, seg_reduce


class _SegStd(torch.autograd.Function):
    """out[v] = sqrt(relu(mean(x^2) - mean(x)^2) + 1e-5) over v's in-edge rows of msg [E, D]; 0 without in-edges."""

    @staticmethod
    def forward(ctx, msg, graph):
        msg = f32c(msg)
        require_hip(msg)
        E, N, D = graph.num_edges(), graph.number_of_nodes(), msg.shape[1]
        if msg.shape[0] != E:
            raise _lib.MrgnasError(f"a_std: message rows {msg.shape[0]} != number of edges {E}")
        p = graph.plan()
        out, mean, coef = (torch.empty(N, D, dtype=torch.float32, device=msg.device) for _ in range(3))
        plan_args, ws = _chunk_plan_args(p, D, msg, "mrg_seg_std_workspace_bytes")
        call("mrg_seg_std_fwd", (ptr(msg), ptr(p["eid"]), *plan_args, ptr(p["in_degree"]), ptr(out), ptr(mean), ptr(coef), ptr(ws), N, D,
                                 stream_of(msg)), nbytes=4 * E * D + 4 * E + 12 * N * D)
        ctx.graph = graph
        ctx.save_for_backward(msg, mean, coef)
        return out

    @staticmethod
    def backward(ctx, g):
        msg, mean, coef = ctx.saved_tensors
        graph = ctx.graph
        g = f32c(g)
        E, N, D = msg.shape[0], graph.number_of_nodes(), msg.shape[1]
        gmsg = torch.empty(E, D, dtype=torch.float32, device=msg.device)
        big = 12 * N * D > ORDERED_BWD_MIN_BYTES             # the three gathered [N, D] tables beyond the caches: walk by destination
        order = graph.plan()["eid"] if big else None
        call("mrg_seg_std_bwd", (ptr(g), ptr(msg), ptr(graph.i32("dst")), ptr(mean), ptr(coef), ptr(order), ptr(gmsg), E, N, D,
                                 stream_of(msg)), nbytes=8 * E * D + 4 * E + 12 * N * D)
        return gmsg, None


def aggregate_std(msg, block):
    """a_std (reference models/operations.py:168-190) on HIP: [E, D] edge rows -> [n_dst, D]."""
    return _SegStd.apply(msg, block)


def inv_in_degree(block):
    """1 / max(in-degree, 1) per destination as [n_dst, 1] float32 (a_mean's scale), cached on the block."""
    deg = block.plan()["in_degree"] if block.device.type == "cuda" else block.in_degrees()
    from ..graph import cached_on
    return cached_on(block, "_nc_inv_deg", (deg,), None, lambda: (1.0 / deg.clamp(min=1).float()).view(-1, 1))


def aggregate_nc(kind, msg, block):
    """a_sum ("sum") / a_std ("std") of the node-classification task: the reduction of the E edge rows, no self rows."""
    if kind == "std":
        return aggregate_std(msg, block)
    if kind != "sum":
        raise _lib.MrgnasError(f"aggregate_nc: unknown reduction {kind!r}")
    return seg_reduce("sum", msg, None, block)


def linear_relu_aggregate_nc(kind, x, W, b, block):
    """a_max ("max") / a_mean ("mean") of the node-classification task: reduce_{e -> v} ReLU(x_e W^T + b) over the E edge rows of x,
    no self rows; 0 for a destination without in-edges."""
    if kind == "max":
        return linear_relu_partial("max", x, W, b, block)[0]
    if kind == "mean":
        return linear_relu_partial("sum", x, W, b, block)[0] * inv_in_degree(block)
    raise _lib.MrgnasError(f"linear_relu_aggregate_nc: unknown reduction {kind!r}")
