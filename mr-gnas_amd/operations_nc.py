"""Drop-in operator zoo for MR-GNAS node classification, MI355X-native.

Importable in place of the reference's ``models/operations.py``: the same registry ``MIXED_OPS`` (``name -> constructor(args
dict)``, 13 entries), the same op-name lists in the same order (the order defines the alpha columns; ``a_std`` is in none of them
and is reachable through a genotype only), the same class names, ``forward(g, src_emb, src_emb_in)`` signatures and parameter
names, plus the unregistered ``pre_corr_op``.  ``g`` is a ``mr_gnas_amd.graph.Block`` (sampler.full_neighbor_blocks).

Rows: the compose ops and the first-stage filters work on the E edge rows of a block; the aggregators turn them into n_dst
destination rows WITHOUT self rows (unlike the link-prediction aggregators of operations_lp); the last-stage filters work on
whatever rows they are given.  HIP operands run on the kernels of libmrgnas_hip.so through ``functional``; CPU operands run the
torch formulation.  Unlike operations_lp this module installs no lazy indexing: importing it leaves ``torch.Tensor`` untouched.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as K

MIXED_OPS = {
    'pre_mult': lambda args: pre_mult_op(),
    'pre_sub': lambda args: pre_sub_op(),
    'pre_add': lambda args: pre_add_op(),
    'f_zero': lambda args: f_zero_op(),
    'f_identity': lambda args: f_identity_op(),
    'f_dense': lambda args: f_dense_op(args),
    'f_sparse': lambda args: f_sparse_op(args),
    'f_dense_last': lambda args: f_dense_op_last(args),
    'f_sparse_last': lambda args: f_sparse_op_last(args),
    'a_max': lambda args: a_max_op(args),
    'a_mean': lambda args: a_mean_op(args),
    'a_sum': lambda args: a_sum_op(args),
    'a_std': lambda args: a_std_op(args),
}
PRE_OPS = ['pre_mult', 'pre_sub', 'pre_add']
FIRST_OPS = ['f_zero', 'f_identity', 'f_dense', 'f_sparse']
MIDDLE_OPS = ['a_max', 'a_sum', 'a_mean']
LAST_OPS = ['f_zero', 'f_identity', 'f_dense_last', 'f_sparse_last']

AGGREGATORS = ('a_max', 'a_mean', 'a_sum', 'a_std')     # edge rows in, destination rows out
PAIRED = ('pre_mult', 'pre_sub', 'pre_add', 'pre_corr', 'f_dense', 'f_sparse')   # read both operands row by row
EPS = 1e-5


def _same_rows(name, a, b):
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{name}: operands have {a.shape[0]} and {b.shape[0]} rows (edge rows and destination rows mixed)")


def _edge_rows(name, g, x):
    if x.shape[0] != g.num_edges():
        raise ValueError(f"{name}: expects the block's {g.num_edges()} edge rows, got {x.shape[0]} rows")


# ---- compose -----------------------------------------------------------------------------
class _PreOp(nn.Module):
    kind = None

    def forward(self, g, src_emb, hr):
        _same_rows(type(self).__name__, src_emb, hr)
        if src_emb.is_cuda:
            return K.compose(self.kind, src_emb, hr)
        return {'mult': torch.mul, 'sub': torch.sub, 'add': torch.add}[self.kind](src_emb, hr)


class pre_mult_op(_PreOp):
    kind = 'mult'


class pre_sub_op(_PreOp):
    kind = 'sub'


class pre_add_op(_PreOp):
    kind = 'add'


class pre_corr_op(nn.Module):
    """ccorr(src_emb, hr) (registered by neither task's registry)."""

    def forward(self, g, src_emb, hr):
        hr = hr.expand_as(src_emb)
        if src_emb.is_cuda:
            return K.ccorr(src_emb, hr)
        D = src_emb.shape[-1]
        return torch.fft.irfft(torch.conj(torch.fft.rfft(src_emb, dim=-1)) * torch.fft.rfft(hr, dim=-1), n=D, dim=-1)


# ---- identity / zero ---------------------------------------------------------------------
class f_identity_op(nn.Module):
    def forward(self, g, src_emb, src_emb_in):
        return src_emb


class f_zero_op(nn.Module):
    def forward(self, g, src_emb, src_emb_in):
        return 0 * src_emb


# ---- aggregators: E edge rows -> n_dst destination rows, no self rows ----------------------
def _torch_reduce(kind, m, g):
    """The reduction on the torch side (CPU operands): DGL's update_all(copy_edge, reduce) on a block."""
    _, dst = g.edges()
    n, D = g.number_of_nodes(), m.shape[1]
    deg = torch.zeros(n, dtype=m.dtype, device=m.device).index_add_(0, dst, torch.ones_like(dst, dtype=m.dtype)).view(-1, 1)
    s = torch.zeros(n, D, dtype=m.dtype, device=m.device).index_add(0, dst, m)
    if kind == 'sum':
        return s
    if kind == 'mean':
        return s / deg.clamp(min=1)
    if kind == 'max':
        h = torch.zeros(n, D, dtype=m.dtype, device=m.device).scatter_reduce(0, dst.view(-1, 1).expand_as(m), m, 'amax',
                                                                                include_self=False)
        return torch.where(deg > 0, h, torch.zeros_like(h))
    q = torch.zeros(n, D, dtype=m.dtype, device=m.device).index_add(0, dst, m * m)
    mean = s / deg.clamp(min=1)
    std = torch.sqrt(torch.relu(q / deg.clamp(min=1) - mean * mean) + EPS)
    return torch.where(deg > 0, std, torch.zeros_like(std))


class _LinReluAgg(nn.Module):
    kind = None

    def __init__(self, args):
        super().__init__()
        feature_dim = args.get('feature_dim', 100)
        self.linear = nn.Linear(feature_dim, feature_dim)

    def forward(self, block, src_emb, src_emb_in):
        _edge_rows(type(self).__name__, block, src_emb)
        if src_emb.is_cuda:
            return K.linear_relu_aggregate_nc(self.kind, src_emb, self.linear.weight, self.linear.bias, block)
        return _torch_reduce(self.kind, F.relu(self.linear(src_emb)), block)


class a_max_op(_LinReluAgg):
    kind = 'max'


class a_mean_op(_LinReluAgg):
    kind = 'mean'


class _PlainAgg(nn.Module):
    kind = None

    def __init__(self, args):
        super().__init__()

    def forward(self, block, src_emb, src_emb_in):
        _edge_rows(type(self).__name__, block, src_emb)
        if src_emb.is_cuda:
            return K.aggregate_nc(self.kind, src_emb, block)
        return _torch_reduce(self.kind, src_emb, block)


class a_sum_op(_PlainAgg):
    kind = 'sum'


class a_std_op(_PlainAgg):
    kind = 'std'


# ---- feature filters -----------------------------------------------------------------------
class f_dense_op(nn.Module):
    def __init__(self, args):
        super().__init__()
        self._feature_dim = args.get('feature_dim', 100)
        self.W = nn.Linear(2 * self._feature_dim, self._feature_dim, bias=True)

    def forward(self, g, src_emb, src_emb_in):
        _same_rows('f_dense_op', src_emb, src_emb_in)
        if src_emb.is_cuda:
            return K.dense_filter_single(src_emb, src_emb_in, self.W.weight, self.W.bias)
        return torch.sigmoid(self.W(torch.cat([src_emb, src_emb_in], dim=1))) * src_emb


class f_sparse_op(nn.Module):
    def __init__(self, args):
        super().__init__()
        self._feature_dim = args.get('feature_dim', 100)
        self.W = nn.Linear(2 * self._feature_dim, self._feature_dim, bias=True)
        self.a = nn.Linear(self._feature_dim, 1, bias=False)

    def forward(self, g, src_emb, src_emb_in):
        _same_rows('f_sparse_op', src_emb, src_emb_in)
        if src_emb.is_cuda:
            none3 = [None, None, None]
            return K._Gate.apply(src_emb, src_emb_in, None, 0, 0, 1.0, *none3, *none3, self.W.weight, self.W.bias, self.a.weight)
        return torch.sigmoid(self.a(self.W(torch.cat([src_emb, src_emb_in], dim=1)))) * src_emb


class f_dense_op_last(nn.Module):
    def __init__(self, args):
        super().__init__()
        self._feature_dim = args.get('feature_dim', 100)
        self.W = nn.Linear(self._feature_dim, self._feature_dim, bias=True)

    def forward(self, g, src_emb, src_emb_in):
        if src_emb.is_cuda:
            return K.dense_filter_single(src_emb, None, self.W.weight, self.W.bias)
        return torch.sigmoid(self.W(src_emb)) * src_emb


class f_sparse_op_last(nn.Module):
    def __init__(self, args):
        super().__init__()
        self._feature_dim = args.get('feature_dim', 100)
        self.W = nn.Linear(self._feature_dim, self._feature_dim, bias=True)
        self.a = nn.Linear(self._feature_dim, 1, bias=False)

    def forward(self, g, src_emb, src_emb_in):
        if src_emb.is_cuda:
            return K.gate_last(src_emb, self.W.weight, self.W.bias, self.a.weight)
        return torch.sigmoid(self.a(self.W(src_emb))) * src_emb
