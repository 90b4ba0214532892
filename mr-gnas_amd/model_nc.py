"""Drop-in fixed-genotype network for MR-GNAS node classification, MI355X-native.

Importable in place of the reference's ``models/model.py``: ``OpModule``, ``Cell``, ``MLPClassifier``, ``mean_aggre`` and
``Network`` with the reference's constructor signatures and ``state_dict`` keys, so its checkpoints load.  ``Network.forward(trip_index,
blocks)`` takes the blocks of ``sampler.full_neighbor_blocks`` (DGL's ``MultiLayerFullNeighborSampler(layers, return_eids=True)``)
and returns the logits of the last block's destination nodes.

What runs where, for float32 HIP operands: the cell operators on ``operations_nc`` (HIP kernels), every OpModule / concat Linear on
the row GEMM, every BatchNorm + ReLU on the one-branch MixedOp epilogue (as the ConvE scorer's BN2).  The embedding lookups, the
relation basis product (once per relation type, then gathered per edge: the reference forms it per edge, same values within
rounding), the classifier and the loss stay on torch.  Between layers, the reference's host-side relabel loop (O(n_dst * E)) is
replaced by the next block's local source index: the same row numbers, since block i + 1's source nodes are block i's
destination nodes in order.

A genotype whose wiring mixes edge rows and destination rows (a concat, a sum or a paired operator over both kinds, an aggregator
over destination rows, a cell whose output is not on destination rows) raises ValueError when the cell is built, before any launch.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as K
from .graph import EID, ETYPE
from .operations_nc import AGGREGATORS, MIXED_OPS, PAIRED, _torch_reduce


def _hip_ok(x, module):
    return (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()
            and not any(m._forward_hooks or m._forward_pre_hooks for m in module.modules()))


def _bn_relu(h, bn, one):
    """ReLU(BatchNorm1d(h)) on the one-branch MixedOp epilogue (statistics, running-statistics update and gradients on HIP)."""
    if bn.training and h.shape[0] == 1:                # what F.batch_norm raises for BatchNorm1d on one row
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(h.shape)}")
    return K.mixed_epilogue([h], [bn], one if one.device == h.device else one.to(h.device))


def _one(module):
    module.register_buffer("_one", torch.ones(1), persistent=False)      # the one-branch epilogue's weight (not in state_dict)


class OpModule(nn.Module):

    def __init__(self, args, operation_name):
        super(OpModule, self).__init__()
        self.args = args
        self._feature_dim = args.feature_dim
        self.op = MIXED_OPS[operation_name]({'feature_dim': self._feature_dim})
        self.linear = nn.Linear(self._feature_dim, self._feature_dim, bias=True)
        self.batchnorm_h = nn.BatchNorm1d(self._feature_dim)
        self.activate = nn.ReLU()
        _one(self)

    def forward(self, g, h, h_in):
        h = self.op(g, h, h_in)
        if _hip_ok(h, self):
            if self.args.op_norm:
                return _bn_relu(K.linear(h, self.linear.weight, self.linear.bias), self.batchnorm_h, self._one)
            return K.linear(h, self.linear.weight, self.linear.bias, "relu")
        h = self.linear(h)
        if self.args.op_norm:
            h = self.batchnorm_h(h)
        return self.activate(h)


def row_kinds(genotype):
    """Which rows ("edge" or "dst") every state of a cell lives on, from the genotype's wiring alone; ValueError where the wiring
    mixes the two kinds.  State 0 is the source embedding and state 1 the pre op's output (both on edge rows)."""
    nb = len(set(edge[1] for edge in genotype.alpha_cell))
    concat = list(range(1, 1 + nb)) if genotype.concat_node is None else genotype.concat_node
    ops = {}
    for (name, center, pre) in genotype.alpha_cell:
        ops.setdefault((center - 1, pre), name)                      # only the first op of a (center, pre) pair is used

    def out_kind(name, kin, kin2, where):
        if name in AGGREGATORS:
            if kin != "edge":
                raise ValueError(f"genotype: {name} at {where} reduces destination rows (it needs the block's edge rows)")
            return "dst"
        if name in PAIRED and kin != kin2:
            raise ValueError(f"genotype: {name} at {where} reads {kin} rows and {kin2} rows together")
        return kin

    if (0, 0) not in ops:
        raise ValueError("genotype: node 1 has no operator on node 0")
    kinds = ["edge", None]
    kinds[1] = out_kind(ops[(0, 0)], "edge", "edge", "node 1")
    for n in range(1, nb):
        hs = [out_kind(ops[(n, i)], kinds[i], kinds[1], f"node {n + 1} <- {i}") for i in range(n + 1) if (n, i) in ops]
        if len(set(hs)) > 1:
            raise ValueError(f"genotype: node {n + 1} sums edge rows and destination rows")
        kinds.append(hs[0] if hs else None)
    cat = [kinds[i] for i in concat]
    if None in cat:
        raise ValueError("genotype: the concat reads a node without operators")
    if len(set(cat)) > 1:
        raise ValueError(f"genotype: the concat over nodes {concat} mixes edge rows and destination rows")
    if cat[0] != "dst":
        raise ValueError("genotype: the cell's output is on edge rows; a node-classification cell ends on destination rows")
    return kinds


class Cell(nn.Module):

    def __init__(self, args, genotype):
        super(Cell, self).__init__()
        self.args = args
        self._genotype = genotype
        self._nb_nodes = len(set([edge[1] for edge in genotype.alpha_cell]))
        self._feature_dim = args.feature_dim
        self._concat_node = list(range(1, 1 + self._nb_nodes)) if genotype.concat_node is None else genotype.concat_node
        self._row_kinds = row_kinds(genotype)
        self.batchnorm_h = nn.BatchNorm1d(self._feature_dim)
        self.activate = nn.ReLU()
        _one(self)
        self._compile()

    def _compile(self):
        nb_nodes = self._nb_nodes
        self._ops = nn.ModuleList([nn.ModuleList([nn.ModuleList() for i in range(n)]) for n in range(1, 1 + nb_nodes)])
        for (op_name, center_node, pre_node) in self._genotype.alpha_cell:
            center_node -= 1
            self._ops[center_node][pre_node].append(OpModule(self.args, op_name))
        self.concat = nn.Linear(len(self._concat_node) * self._feature_dim, self._feature_dim)

    def forward(self, g, src_emb, hr):
        zero_out = self._ops[0][0][0](g, src_emb, hr)
        states = [src_emb, zero_out]
        for n in range(1, self._nb_nodes):
            hs = []
            for i in range(n + 1):
                if len(self._ops[n][i]) > 0:
                    hs.append(self._ops[n][i][0](g, states[i], zero_out))
            states.append(sum(hs))
        x = torch.cat([states[idx] for idx in self._concat_node], dim=1)
        if _hip_ok(x, self.concat) and _hip_ok(x, self.batchnorm_h):
            return _bn_relu(K.module_linear(self.concat, x), self.batchnorm_h, self._one)
        return self.activate(self.batchnorm_h(self.concat(x)))


class MLPClassifier(nn.Module):

    def __init__(self, input_dim, output_dim, L=2):  # L = nb_hidden_layers
        super().__init__()
        list_FC_layers = [nn.Linear(input_dim // 2 ** l, input_dim // 2 ** (l + 1), bias=True) for l in range(L)]
        list_FC_layers.append(nn.Linear(input_dim // 2 ** L, output_dim, bias=True))
        self.FC_layers = nn.ModuleList(list_FC_layers)
        self.L = L

    def forward(self, x):
        y = x
        for l in range(self.L):
            y = F.relu(self.FC_layers[l](y))
        return self.FC_layers[self.L](y)


class mean_aggre(nn.Module):
    """Unused by Network (as in the reference); kept for its parameters (state_dict) and as a standalone a_mean."""

    def __init__(self, feature_dim):
        super(mean_aggre, self).__init__()
        self.linear = nn.Linear(feature_dim, feature_dim)

    def forward(self, block, src_emb):
        if src_emb.is_cuda:
            return K.linear_relu_aggregate_nc("mean", src_emb, self.linear.weight, self.linear.bias, block)
        return _torch_reduce("mean", F.relu(self.linear(src_emb)), block)


class Network(nn.Module):

    def __init__(self, device, genotype, number_of_nodes, num_classes, num_rels, layers, zero_nodes, nodes, feature_dim,
                 init_fea_dim, num_base_r, criterion, args):
        super(Network, self).__init__()
        self._device = device
        self._layers = layers
        self._in_dim_n = number_of_nodes
        self._in_dim_e = num_rels
        self._feature_dim = feature_dim
        self._init_fea_dim = init_fea_dim
        self._num_base_r = num_base_r
        self._num_classes = num_classes
        self._criterion = criterion
        self._nb_zero_nodes = zero_nodes
        self._nb_first_nodes = nodes
        self._nb_last_nodes = nodes
        self._nb_zero_edges = self._nb_zero_nodes
        self._nb_first_edges = sum(self._nb_zero_nodes + i for i in range(self._nb_first_nodes))
        self._nb_middle_edges = self._nb_first_nodes
        self._nb_last_edges = sum(self._nb_first_nodes + i for i in range(self._nb_last_nodes))
        self.embedding_h = nn.Embedding(self._in_dim_n, self._init_fea_dim)
        self.embedding_e = nn.Embedding(self._num_base_r, self._init_fea_dim)
        self.rel_wt = self.get_param([self._in_dim_e, self._num_base_r])
        self.rel_num = torch.arange(self._num_base_r, device=self._device)
        self.embedding_h_init = nn.Linear(self._init_fea_dim, self._feature_dim, bias=False)
        self.embedding_e_init = nn.Linear(self._init_fea_dim, self._feature_dim, bias=False)
        self.cells = nn.ModuleList([Cell(args, genotype[i]) for i in range(self._layers)])
        self.classifier = MLPClassifier(self._feature_dim, self._num_classes)
        self.mean_aggre = mean_aggre(self._feature_dim)
        self.batchnorm_h = nn.BatchNorm1d(self._feature_dim)
        self.activate = nn.ReLU()
        _one(self)

    def _forward(self, trip_index, blocks):
        if len(blocks) != len(self.cells):
            raise ValueError(f"{len(self.cells)} cells need {len(self.cells)} blocks, got {len(blocks)}")
        # relation features once per relation type (reference: per edge), gathered by the blocks' edge types below
        rel_num = self.rel_num if self.rel_num.device == self.rel_wt.device else self.rel_num.to(self.rel_wt.device)
        rel_feat = self.embedding_e_init(torch.mm(self.rel_wt, self.embedding_e(rel_num)))
        for i, cell in enumerate(self.cells):
            block = blocks[i]
            if i == 0:
                src_b = torch.index_select(trip_index, dim=0, index=block.edata[EID])[:, 1]     # trip_index rows: (eid, src, dst)
                src_embed = self.embedding_h_init(self.embedding_h(src_b))
            else:
                src_embed = torch.index_select(node_embed, 0, block.edges()[0])     # block i's local sources = rows of block i - 1's output
            edges_embed = torch.index_select(rel_feat, 0, block.edata[ETYPE])
            node_embed = cell(block, src_embed, edges_embed)
        if _hip_ok(node_embed, self.batchnorm_h):
            return _bn_relu(node_embed, self.batchnorm_h, self._one)
        return self.activate(self.batchnorm_h(node_embed))

    def forward(self, trip_index, g):
        h = self._forward(trip_index, g)
        return self.classifier(h)

    def get_param(self, shape):
        param = nn.Parameter(torch.Tensor(*shape))
        nn.init.xavier_normal_(param, gain=nn.init.calculate_gain('relu'))
        return param

    def _loss(self, trip_index, g, labels, idx):
        logits = self.forward(trip_index, g)
        return self._criterion(logits, labels[idx])
