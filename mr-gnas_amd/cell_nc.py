"""Drop-in search cell for MR-GNAS node classification, MI355X-native.

Importable in place of the reference's ``models/cell.py``: ``MixedOp``, ``Cell_Zero``, ``Cell_First``, ``Cell_Middle``, ``Cell_Last``
and ``Cell`` with the reference's constructor signatures and ``state_dict`` keys (``..._ops.{i}._ops.{k}.{1,2}.*``: a candidate is
the ModuleList ``[op, Linear, BatchNorm1d, ReLU]``).  ``g`` is a ``mr_gnas_amd.graph.Block``.

Row kinds are fixed by the wiring: the zero and the first stage work on the block's E edge rows, the middle stage (the aggregators)
takes them to the n_dst destination rows, the last stage and the concat work on destination rows.  The ``h_in`` the last stage
receives is the zero stage's output on EDGE rows; no ``LAST_OPS`` operator reads it (as in the reference).

The NC MixedOp is not the link-prediction one: every candidate carries its own ``Linear(D, D)`` between the operator and the
BatchNorm, and so ``f_zero`` is not zero -- ``Linear(0 * x)`` is the bias on every row, BatchNorm in training mode turns a constant
column into ``beta``, the candidate contributes ``w_k * ReLU(beta_k)`` to every row and its running statistics move
(``running_mean -> bias``, ``running_var -> 0``).  Here the branch is a stored candidate of ``bias`` rows
(``functional.constant_candidate``); its ``Linear.weight.grad`` is a zero tensor, as in the reference.

What runs where, for float32 HIP operands: the operators on ``operations_nc`` (HIP kernels), the candidates' Linears of one MixedOp
as ONE grouped launch that also forms their BatchNorm sums (``functional.candidate_linears``), BatchNorm + ReLU + the weighted sum
-- and the sum over the MixedOps that feed one state, through ``addend`` -- on the MixedOp epilogue, the concat Linear on the row
GEMM and its BatchNorm + ReLU on the one-branch epilogue.  CPU operands run the torch formulation.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as K
from .model_nc import _bn_relu, _hip_ok, _one
from .operations_nc import FIRST_OPS, LAST_OPS, MIDDLE_OPS, MIXED_OPS, PRE_OPS


class MixedOp(nn.Module):

    def __init__(self, feature_dim, operations):
        super(MixedOp, self).__init__()
        self._feature_dim = feature_dim
        self._operations = operations
        self._args = {'feature_dim': self._feature_dim}
        self._ops = nn.ModuleList([nn.ModuleList([MIXED_OPS[op_name](self._args),
                                                  nn.Linear(self._feature_dim, self._feature_dim, bias=True),
                                                  nn.BatchNorm1d(self._feature_dim),
                                                  nn.ReLU()])
                                   for op_name in self._operations])

    def forward(self, weights, g, h, h_in, addend=None):
        """sum_k weights[k] * ReLU(BatchNorm_k(Linear_k(op_k(g, h, h_in))))  (+ addend: the MixedOps summed into the same state)."""
        if _hip_ok(h, self) and weights.is_cuda:
            return self._forward_hip(weights, g, h, h_in, addend)
        output = sum(w * self.op_forward(op, g, h, h_in) for w, op in zip(weights, self._ops))
        return output if addend is None else addend + output

    def op_forward(self, op, g, h, h_in):
        nh = op[0](g, h, h_in)
        for i in range(1, len(op)):
            nh = op[i](nh.float())
        return nh

    def _forward_hip(self, weights, g, h, h_in, addend):
        training = self._ops[0][2].training
        xs = [None if name == 'f_zero' else op[0](g, h, h_in) for name, op in zip(self._operations, self._ops)]
        rows = next((x.shape[0] for x in xs if x is not None), h.shape[0])
        if training and rows == 1:                         # what F.batch_norm raises for BatchNorm1d on one row
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {(rows, self._feature_dim)}")
        if all(x is None for x in xs):
            cands = [K.constant_candidate(op[1], rows) for op in self._ops]
        else:
            cands = K.candidate_linears(xs, [op[1] for op in self._ops], K.ForEpilogue(stats=training))
        return K.mixed_epilogue_prepare(cands, [op[2] for op in self._ops])(weights, addend)


def _summed(ops, weights, offset, g, states, h_in):
    """The sum of the MixedOps ops[offset + j] over states[j], accumulated through the epilogue's addend."""
    s = None
    for j, h in enumerate(states):
        s = ops[offset + j](weights[offset + j], g, h, h_in, addend=s)
    return s


class Cell_Zero(nn.Module):

    def __init__(self, nodes, feature_dim):
        super(Cell_Zero, self).__init__()
        self._feature_dim = feature_dim
        self._ops = nn.ModuleList()
        self._ops.append(MixedOp(feature_dim, operations=PRE_OPS))

    def forward(self, g, h, hr, weights):
        return self._ops[0](weights[0], g, h, hr)


class Cell_First(nn.Module):

    def __init__(self, nodes, feature_dim):
        super(Cell_First, self).__init__()
        self._nodes = nodes
        self._feature_dim = feature_dim
        self._ops = nn.ModuleList()
        for i in range(nodes):
            for j in range(i + 1):
                self._ops.append(MixedOp(feature_dim, operations=FIRST_OPS))

    def forward(self, g, states, h_in, weights):
        offset = 0
        for i in range(self._nodes):
            s = _summed(self._ops, weights, offset, g, states, h_in)
            offset += len(states)
            states.append(s)
        return states[1:]


class Cell_Middle(nn.Module):

    def __init__(self, nodes, feature_dim):
        super(Cell_Middle, self).__init__()
        self._nodes = nodes
        self._feature_dim = feature_dim
        self._ops = nn.ModuleList()
        for i in range(nodes):
            self._ops.append(MixedOp(feature_dim, operations=MIDDLE_OPS))

    def forward(self, g, states, h_in, weights):
        return [self._ops[i](weights[i], g, states[i], h_in) for i in range(self._nodes)]


class Cell_Last(nn.Module):

    def __init__(self, in_nodes, nodes, feature_dim):
        super(Cell_Last, self).__init__()
        self._in_nodes = in_nodes
        self._nodes = nodes
        self._feature_dim = feature_dim
        self._ops = nn.ModuleList()
        for i in range(nodes):
            for j in range(i + in_nodes):
                self._ops.append(MixedOp(feature_dim, operations=LAST_OPS))

    def forward(self, g, states, h_in, weights):
        offset = 0
        for i in range(self._nodes):
            s = _summed(self._ops, weights, offset, g, states, h_in)
            offset += len(states)
            states.append(s)
        return states


class Cell(nn.Module):

    def __init__(self, nb_zero_nodes, nb_first_nodes, nb_last_nodes, feature_dim, dropout=0.0):
        super(Cell, self).__init__()
        self._nb_zero_nodes = nb_zero_nodes
        self._nb_first_nodes = nb_first_nodes
        self._nb_last_nodes = nb_last_nodes
        self._feature_dim = feature_dim
        self._dropout = dropout
        self.cell_zero = Cell_Zero(nb_zero_nodes, feature_dim)
        self.cell_first = Cell_First(nb_first_nodes, feature_dim)
        self.cell_middle = Cell_Middle(nb_first_nodes, feature_dim)
        self.cell_last = Cell_Last(nb_first_nodes, nb_last_nodes, feature_dim)
        self.concat_weights = nn.Linear((nb_first_nodes + nb_last_nodes) * feature_dim, feature_dim)
        self.batchnorm_h = nn.BatchNorm1d(feature_dim)
        self.activate = nn.ReLU()
        _one(self)

    def forward(self, g, src_emb, hr, weights_zero, weights_first, weights_middle, weights_last):
        h_in = self.cell_zero(g, src_emb, hr, weights_zero)                   # edge rows
        states = self.cell_first(g, [h_in], h_in, weights_first)              # edge rows
        states = self.cell_middle(g, states, h_in, weights_middle)            # edge rows -> destination rows
        states = self.cell_last(g, states, h_in, weights_last)                # destination rows (h_in: edge rows, unread)
        x = torch.cat(states, dim=1)
        if _hip_ok(x, self.concat_weights) and _hip_ok(x, self.batchnorm_h):
            h = _bn_relu(K.module_linear(self.concat_weights, x), self.batchnorm_h, self._one)
        else:
            h = self.activate(self.batchnorm_h(self.concat_weights(x)))
        return F.dropout(h, self._dropout, training=self.training)
