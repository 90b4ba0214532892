"""Drop-in search supernet for MR-GNAS node classification, MI355X-native.

Importable in place of the reference's ``models/model_search.py``: ``MLPClassifier``, ``mean_aggre`` and ``Network`` with the
reference's constructor signature, ``state_dict`` keys and architecture-parameter interface (``arch_parameters``, ``load_alpha``,
``show_weights``, ``normalize_weights``, ``show_genotype(s)``, ``_loss``).  The four alphas are plain tensors with ``requires_grad``
(``1e-3 * randn``), not Parameters: they are not in ``state_dict`` and ``Network.to()`` does not move them -- pass the device to the
constructor, as the reference's driver does.  ``Network.forward(trip_index, blocks)`` takes the blocks of
``sampler.full_neighbor_blocks`` and returns the logits of the last block's destination nodes.

As in ``model_nc.Network``: the relation features are formed once per relation type and gathered per edge (the reference forms them
per edge: same values within rounding), and between layers the reference's host-side relabel loop is replaced by the next block's
local source index (block i + 1's source nodes are block i's destination nodes in order).  The cells run on ``cell_nc``; the
embedding lookups, the basis product, the classifier and the loss stay on torch.

``new()`` raises: the reference's ``new()`` calls its own constructor with the wrong argument list and cannot run; only the
second-order architect step, which this package does not provide, would call it.
"""
import collections

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as K
from .cell_nc import Cell
from .graph import EID, ETYPE
from .model_nc import MLPClassifier, _bn_relu, _hip_ok, _one, mean_aggre      # noqa: F401  (the reference defines them here too)
from .operations_nc import FIRST_OPS, LAST_OPS, MIDDLE_OPS, PRE_OPS

# reference configs/genotypes.py:3 -- the definition of supernet.Genotype (equal repr, equal as tuples); not imported from there
# because supernet imports operations_lp, which installs the link-prediction task's lazy tensor indexing
Genotype = collections.namedtuple('Genotype', 'alpha_cell concat_node score_func')


def _best_edge(W, ops):
    """Among the rows of W (one per candidate input state), the row whose largest non-f_zero weight is largest and that weight's
    column; ties go to the lower index, as the reference's stable sort and strict comparison leave them."""
    zero = ops.index('f_zero')
    best_j = best_k = None
    for j, row in enumerate(W):
        k_row = None
        for k, v in enumerate(row):
            if k != zero and (k_row is None or v > row[k_row]):
                k_row = k
        if best_j is None or row[k_row] > W[best_j][best_k]:
            best_j, best_k = j, k_row
    return best_j, best_k


class Network(nn.Module):

    def __init__(self, device, number_of_nodes, num_classes, num_rels, layers, zero_nodes, nodes, feature_dim,
                 init_fea_dim, num_base_r,
                 dropout=0.0):
        super(Network, self).__init__()
        self._device = device
        self._layers = layers
        self._in_dim_n = number_of_nodes
        self._in_dim_e = num_rels
        self._feature_dim = feature_dim
        self._num_base_r = num_base_r
        self._init_fea_dim = init_fea_dim
        self._num_classes = num_classes
        self._criterion = nn.CrossEntropyLoss()
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
        self.cells = nn.ModuleList(
            [Cell(self._nb_zero_nodes, self._nb_first_nodes, self._nb_last_nodes, self._feature_dim)
             for i in range(self._layers)])
        self._initialize_alphas()
        self.classifier = MLPClassifier(self._feature_dim, self._num_classes)
        self.mean_aggre = mean_aggre(self._feature_dim)
        self.batchnorm_h = nn.BatchNorm1d(self._feature_dim)
        self.activate = nn.ReLU()
        self._dropout = dropout
        _one(self)

    def new(self):
        raise NotImplementedError("Network.new(): the reference's new() calls its own constructor with the wrong argument list and "
                                  "cannot run; it serves the second-order architect step only, which is not provided")

    def get_param(self, shape):
        param = nn.Parameter(torch.Tensor(*shape))
        nn.init.xavier_normal_(param, gain=nn.init.calculate_gain('relu'))
        return param

    def load_alpha(self, alphas):
        for x, y in zip(self.arch_parameters(), alphas):
            x.data.copy_(y.data)

    def arch_parameters(self):
        return self._arch_parameters

    def _initialize_alphas(self):
        def alpha(edges, ops):
            return (1e-3 * torch.randn(edges * self._layers, len(ops))).to(self._device).requires_grad_(True)

        self.alphas_zero_cell = alpha(self._nb_zero_edges, PRE_OPS)
        self.alphas_first_cell = alpha(self._nb_first_edges, FIRST_OPS)
        self.alphas_middle_cell = alpha(self._nb_middle_edges, MIDDLE_OPS)
        self.alphas_last_cell = alpha(self._nb_last_edges, LAST_OPS)
        self._arch_parameters = [self.alphas_zero_cell, self.alphas_first_cell, self.alphas_middle_cell, self.alphas_last_cell]

    def _forward(self, trip_index, block):
        if len(block) != len(self.cells):
            raise ValueError(f"{len(self.cells)} cells need {len(self.cells)} blocks, got {len(block)}")
        # relation features once per relation type (reference: per edge), gathered by the blocks' edge types below
        rel_num = self.rel_num if self.rel_num.device == self.rel_wt.device else self.rel_num.to(self.rel_wt.device)
        rel_feat = self.embedding_e_init(torch.mm(self.rel_wt, self.embedding_e(rel_num)))
        with K.deferred_counters():
            for i, cell in enumerate(self.cells):
                b = block[i]
                if i == 0:
                    src_b = torch.index_select(trip_index, dim=0, index=b.edata[EID])[:, 1]     # trip_index rows: (eid, src, dst)
                    src_embed = self.embedding_h_init(self.embedding_h(src_b))
                else:
                    src_embed = torch.index_select(node_embed, 0, b.edges()[0])     # block i's local sources = rows of block i - 1's output
                edges_embed = torch.index_select(rel_feat, 0, b.edata[ETYPE])
                W_zero, W_first, W_middle, W_last = self.show_weights(i)
                node_embed = cell(b, src_embed, edges_embed, W_zero, W_first, W_middle, W_last)
            if _hip_ok(node_embed, self.batchnorm_h):
                h = _bn_relu(node_embed, self.batchnorm_h, self._one)
            else:
                h = self.activate(self.batchnorm_h(node_embed))
        return F.dropout(h, self._dropout, training=self.training)

    def forward(self, trip_index, g):
        h = self._forward(trip_index, g)
        return self.classifier(h)

    def _loss(self, trip_index, g, labels, idx):
        logits = self.forward(trip_index, g)
        return self._criterion(logits, labels[idx])

    def normalize_weights(self, W_zero, W_first, W_middle, W_last):
        return F.softmax(W_zero, dim=1), F.softmax(W_first, dim=1), F.softmax(W_middle, dim=1), F.softmax(W_last, dim=1)

    def show_weights(self, nb_layer):
        def rows(a, per_layer):
            return a[nb_layer * per_layer: (nb_layer + 1) * per_layer]

        return self.normalize_weights(rows(self.alphas_zero_cell, self._nb_zero_edges), rows(self.alphas_first_cell, self._nb_first_edges),
                                      rows(self.alphas_middle_cell, self._nb_middle_edges), rows(self.alphas_last_cell, self._nb_last_edges))

    def show_genotype(self, nb_layer):
        """The discrete cell of layer nb_layer: per stage the strongest operator of every node (zero / middle stage: the argmax of
        the node's own MixedOp; first / last stage: the strongest non-f_zero operator over the node's candidate inputs).  Node
        numbering and tie-breaking are the reference's (models/model_search.py:208-289); the weights are read once."""
        nz, nf, nl = self._nb_zero_nodes, self._nb_first_nodes, self._nb_last_nodes
        with torch.no_grad():
            W_zero, W_first, W_middle, W_last = (w.detach().cpu() for w in self.show_weights(nb_layer))
        gene = []
        pre_nodes = list(range(nz))
        for n in range(nz):                                 # zero stage: a chain node n -> n + 1
            gene.append((PRE_OPS[int(torch.argmax(W_zero[n]))], n + 1, pre_nodes[n]))
            pre_nodes[n] = n + 1
        base = max(pre_nodes)
        W_first, W_last = W_first.tolist(), W_last.tolist()
        start = 0
        for n in range(1, nf + 1):                          # first stage: node base + n picks one of its n inputs
            j, k = _best_edge(W_first[start:start + n], FIRST_OPS)
            gene.append((FIRST_OPS[k], base + n, base + j))
            start += n
        concat_node = []
        middle_nodes = list(range(2, 2 + nf))
        for n in range(nf):                                 # middle stage: one aggregator per first-stage node
            new_node = max(middle_nodes) + 1
            gene.append((MIDDLE_OPS[int(torch.argmax(W_middle[n]))], new_node, middle_nodes[n]))
            concat_node.append(new_node)
            middle_nodes[n] = new_node
        top = max(middle_nodes)
        start = 0
        for n in range(nl):                                 # last stage: node top + 1 + n picks one of its nf + n inputs
            j, k = _best_edge(W_last[start:start + nf + n], LAST_OPS)
            pre = middle_nodes[j] if j < nf else j - nf + top + 1
            gene.append((LAST_OPS[k], top + 1 + n, pre))
            concat_node.append(top + 1 + n)
            start += nf + n
        return Genotype(alpha_cell=gene, concat_node=concat_node, score_func=None)

    def show_genotypes(self):
        return [self.show_genotype(i) for i in range(self._layers)]
