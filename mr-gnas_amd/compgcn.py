"""CompGCN layer and stack on the fused HIP kernel, and CompGCN with the ConvE scorer, importable in place of the
reference's ``models/compgcn.py`` (``CompGraphConv`` :12-113, ``CompGCN`` :116-185, ``CompGCN_ConvE`` :188-269).

Same constructors, same ``forward`` signatures and return values, same parameter names
(``W_O, W_I, W_S, W_R, loop_rel, bn``; ``basis, weights | rel_embds, n_embds, layers, dropouts``;
``compGCN_Model, bn0, bn1, bn2, hidden_drop, feature_drop, m_conv1, fc, bias``).

``CompGCN_ConvE`` runs the ConvE scorer on csrc/conve.hip (the interleaved image) for float32 HIP operands, with BN2 + ReLU on
the MixedOp epilogue kernels and the [B, N] product on the row GEMM; autocast, forward hooks on a scorer submodule, or a
BatchNorm without running statistics or with momentum=None run the reference's torch formulation instead.  Unlike the
reference, it raises a ValueError when ``k_w * k_h != layer_size[-1]`` (the reference's reshape then silently makes several
images per row and returns more score rows than queries).  It also follows the scorer protocol of operations_lp.py
(``embed``, ``query``, ``score_kind``, ``score_bias``, ``score_func`` = the model itself) and has ``loss_1n``: the training loss and, through
``evaluation.predict_1n`` / ``predict_topk``, the evaluation without a [B, N] tensor, the per-entity bias riding in the sweeps' epilogues.
``g`` is a ``RelGraph`` carrying ``edata['etype'|'norm'|'in_edges_mask'|'out_edges_mask']``.

What changes is the schedule: W_O and W_I are linear and applied before a *sum*, so they
commute with it.  The layer aggregates phi(h_src, r*norm) per (destination, direction) with ONE
fused gather->compose->segmented-sum launch (no [E, D] tensor exists), then applies
[W_O | W_I] to the [N, 2*Din] result on the MFMA pipe; the biases enter through the
per-node edge counts.  max|delta| against the reference's per-edge order is ~1e-6 (tested).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as K
from ._lib import MrgnasError
from .graph import cached_on


def _layer_plans(g, n_rel_rows):
    """Index structures of a graph for CompGraphConv, cached on the graph object for as long as the edge
    tensors they derive from (masks, norm, etype) are the same unmodified objects."""
    src, dst, _ = g.edges(form='all')
    deps = (src, dst, g.edata['in_edges_mask'], g.edata['out_edges_mask'], g.edata['norm'], g.edata['etype'])
    return cached_on(g, "_mrg_compgcn_plans", deps, n_rel_rows, lambda: _build_layer_plans(g, n_rel_rows))


def _build_layer_plans(g, n_rel_rows):
    src, dst, _ = g.edges(form='all')
    N, dev = g.number_of_nodes(), src.device
    in_m = g.edata['in_edges_mask'].bool()
    out_m = g.edata['out_edges_mask'].bool()
    keep = torch.nonzero(in_m | out_m).view(-1)                  # edges in neither mask contribute 0 (reference :80-82)
    direction = in_m[keep].long()                                # an edge in both masks is transformed by W_I (:82 overwrites :81)
    seg = dst[keep] * 2 + direction                              # segment = (destination, direction); 0 = out (W_O), 1 = in (W_I)
    norm = g.edata['norm'].reshape(-1).float()[keep]
    edges = K.ComposePlan(src[keep], g.edata['etype'].long()[keep], seg, norm, N, n_rel_rows, 2 * N)
    counts = torch.bincount(seg, minlength=2 * N).view(N, 2).float()
    ar = torch.arange(N, device=dev)
    loop = K.ComposePlan(ar, torch.full((N,), n_rel_rows - 1, dtype=torch.long, device=dev), ar, None, N, n_rel_rows, N)
    return {"n_rel_rows": n_rel_rows, "edges": edges, "counts": counts, "loop": loop}


class CompGraphConv(nn.Module):
    """One layer of CompGCN."""

    def __init__(self, in_dim, out_dim, comp_fn='sub', batchnorm=True, dropout=0.1):
        super().__init__()
        self.in_dim, self.out_dim, self.comp_fn, self.batchnorm = in_dim, out_dim, comp_fn, batchnorm
        self.actvation = torch.tanh
        self.dropout = nn.Dropout(dropout)
        if batchnorm:
            self.bn = nn.BatchNorm1d(out_dim)
        self.W_O = nn.Linear(in_dim, out_dim)
        self.W_I = nn.Linear(in_dim, out_dim)
        self.W_S = nn.Linear(in_dim, out_dim)
        self.W_R = nn.Linear(in_dim, out_dim)
        self.loop_rel = nn.Parameter(torch.empty(1, in_dim))
        self.register_buffer("_one", torch.ones(1), persistent=False)      # the one-branch epilogue's weight (not in state_dict)
        nn.init.xavier_normal_(self.loop_rel)

    def forward(self, g, n_in_feats, r_feats):
        if self.comp_fn not in ('sub', 'mul', 'ccorr'):
            raise Exception('Only supports sub, mul, and ccorr')
        r_plus = torch.cat((r_feats, self.loop_rel), 0)
        P = _layer_plans(g, r_plus.shape[0])
        N = g.number_of_nodes()
        # steps 1-3: sum over in-edges of phi(h_src, r*norm), per direction  -> [N, 2*Din]
        A = K.compose_aggregate(self.comp_fn, n_in_feats, r_plus, P["edges"]).view(N, 2 * self.in_dim)
        W_cat = torch.cat((self.W_O.weight, self.W_I.weight), dim=1)
        cnt = P["counts"]                                   # the biases enter through the per-node edge counts ([N, 2] x [2, D] as two broadcasts:
        comp_edge = K.linear(A, W_cat) + (cnt[:, :1] * self.W_O.bias + cnt[:, 1:] * self.W_I.bias)   # a K = 2 product costs a 66 us vendor GEMM)
        # step 4: self-loop composition with loop_rel
        comp_s = K.compose_aggregate(self.comp_fn, n_in_feats, r_plus, P["loop"])
        n_out = (K.linear(comp_s, self.W_S.weight, self.W_S.bias) + self.dropout(comp_edge)) * (1 / 3)
        r_out = K.linear(r_plus, self.W_R.weight, self.W_R.bias)
        if K.switches.COMPGCN_TAIL and self.batchnorm and self.actvation is torch.tanh and n_out.is_cuda and not (self.bn._forward_hooks or self.bn._forward_pre_hooks):
            # BatchNorm -> tanh on the MixedOp epilogue kernels with one branch of weight 1 and the tanh activation (statistics
            # pass + combine pass; backward one reduction + one apply pass) instead of torch's four BatchNorm kernels + tanh
            n_out = K.mixed_epilogue([n_out], [self.bn], self._one if self._one.device == n_out.device else self._one.to(n_out.device), act="tanh")
            return n_out, r_out[:-1]
        if self.batchnorm:
            n_out = self.bn(n_out)
        if self.actvation is not None:
            n_out = self.actvation(n_out)
        return n_out, r_out[:-1]


class CompGCN(nn.Module):
    def __init__(self, num_bases, num_rel, num_ent, in_dim=100, layer_size=[200], comp_fn='sub', batchnorm=True,
                 dropout=0.1, layer_dropout=[0.3]):
        super().__init__()
        self.num_bases, self.num_rel, self.num_ent = num_bases, num_rel, num_ent
        self.in_dim, self.layer_size, self.comp_fn = in_dim, layer_size, comp_fn
        self.batchnorm, self.dropout, self.layer_dropout = batchnorm, dropout, layer_dropout
        self.num_layer = len(layer_size)
        dims = [in_dim] + list(layer_size)
        self.layers = nn.ModuleList(CompGraphConv(dims[i], dims[i + 1], comp_fn=comp_fn, batchnorm=batchnorm, dropout=dropout)
                                    for i in range(self.num_layer))
        if num_bases > 0:
            self.basis = nn.Parameter(torch.empty(num_bases, in_dim))
            self.weights = nn.Parameter(torch.empty(num_rel, num_bases))
            nn.init.xavier_normal_(self.basis)
            nn.init.xavier_normal_(self.weights)
        else:
            self.rel_embds = nn.Parameter(torch.empty(num_rel, in_dim))
            nn.init.xavier_normal_(self.rel_embds)
        self.n_embds = nn.Parameter(torch.empty(num_ent, in_dim))
        nn.init.xavier_normal_(self.n_embds)
        self.dropouts = nn.ModuleList(nn.Dropout(layer_dropout[i]) for i in range(self.num_layer))

    def forward(self, graph):
        n_feats = self.n_embds
        r_feats = torch.mm(self.weights, self.basis) if self.num_bases > 0 else self.rel_embds
        for layer, drop in zip(self.layers, self.dropouts):
            n_feats, r_feats = layer(graph, n_feats, r_feats)
            n_feats = drop(n_feats)
        return n_feats, r_feats


class CompGCN_ConvE(nn.Module):
    """CompGCN with the ConvE score function (reference models/compgcn.py:188-269)."""

    def __init__(self, num_bases, num_rel, num_ent, in_dim, layer_size, comp_fn='sub', batchnorm=True, dropout=0.1,
                 layer_dropout=[0.3], num_filt=200, hid_drop=0.3, feat_drop=0.3, ker_sz=5, k_w=5, k_h=5):
        super().__init__()
        self.embed_dim = layer_size[-1]
        self.hid_drop, self.feat_drop, self.ker_sz, self.k_w, self.k_h, self.num_filt = hid_drop, feat_drop, ker_sz, k_w, k_h, num_filt
        self.compGCN_Model = CompGCN(num_bases, num_rel, num_ent, in_dim, layer_size, comp_fn, batchnorm, dropout, layer_dropout)
        self.bn0 = nn.BatchNorm2d(1)
        self.bn1 = nn.BatchNorm2d(self.num_filt)
        self.bn2 = nn.BatchNorm1d(self.embed_dim)
        self.hidden_drop = nn.Dropout(self.hid_drop)
        self.feature_drop = nn.Dropout(self.feat_drop)
        self.m_conv1 = nn.Conv2d(1, out_channels=self.num_filt, kernel_size=(self.ker_sz, self.ker_sz), stride=1, padding=0, bias=False)
        flat_sz_h = int(2 * self.k_w) - self.ker_sz + 1
        flat_sz_w = self.k_h - self.ker_sz + 1
        self.flat_sz = flat_sz_h * flat_sz_w * self.num_filt
        self.fc = nn.Linear(self.flat_sz, self.embed_dim)
        self.bias = nn.Parameter(torch.zeros(num_ent))
        self.register_buffer("_one", torch.ones(1), persistent=False)      # the one-branch epilogue's weight (not in state_dict)

    def concat(self, e1_embed, rel_embed):
        e1_embed = e1_embed.view(-1, 1, self.embed_dim)
        rel_embed = rel_embed.view(-1, 1, self.embed_dim)
        stack_inp = torch.cat([e1_embed, rel_embed], 1)
        return torch.transpose(stack_inp, 2, 1).reshape((-1, 1, 2 * self.k_w, self.k_h))

    # ---- the scorer protocol of the paths that keep no [B, N] tensor (operations_lp: query / score_kind / score_bias), with the model
    # as its own scorer, so that evaluation.predict_1n and evaluation.predict_topk take it unchanged.  No parameters, no buffers.
    score_kind = "dot"

    @property
    def score_func(self):
        return self

    @property
    def score_bias(self):
        return self.bias

    def _check_image(self):
        if self.k_w * self.k_h != self.embed_dim:
            raise ValueError(f"CompGCN_ConvE: k_w * k_h = {self.k_w} * {self.k_h} must equal the embedding width layer_size[-1] = "
                             f"{self.embed_dim} (one 2 k_w x k_h image per query)")

    def _hip_ok(self, tensors):
        mods = (self.bn0, self.m_conv1, self.bn1, self.feature_drop, self.fc, self.hidden_drop, self.bn2)
        return K.conve.hip_path_ok(mods, (self.bn0, self.bn1, self.bn2), tensors)

    def embed(self, graph):
        """(n_feats, r_feats): the CompGCN stack's entity and relation embeddings, the operands of ``query``."""
        return self.compGCN_Model(graph)

    def query(self, sub_emb, rel_emb):
        """The hidden vector after bn2 + ReLU [B, D], the row every entity is scored against (logit = query . entity + bias[entity]):
        forward without its last product, bias and sigmoid.  Like forward it draws the dropout masks and, in train mode, updates the
        BatchNorm statistics: one call per step.  HIP operands only (``_hip_ok``)."""
        self._check_image()
        if not self._hip_ok((sub_emb, rel_emb)):
            raise MrgnasError("CompGCN_ConvE.query runs the ConvE kernels: float32 HIP operands, no autocast, no forward hooks on the "
                              "scorer's submodules, BatchNorms that track running statistics (no CPU or torch fallback)")
        return K.conve_query(sub_emb, rel_emb, K.conve.INTERLEAVED, (2 * self.k_w, self.k_h), self.bn0, self.m_conv1, self.bn1,
                             self.feature_drop, self.fc, self.hidden_drop, self.bn2, self._one)

    def loss_1n(self, graph, sub, rel, label_index, label_smooth=0.0, col_chunk=None):
        """BCELoss(forward(graph, sub, rel), label_index.labels(sub, rel, label_smooth)) -- the reference's training loss -- as a float32
        scalar with no [B, N] tensor: one embed, one query, then the fused 1-N loss with the entity bias in its epilogue
        (functional.rows_bce_all(..., bias=self.bias)).  label_index: sampler.LabelIndex on the same device.  No host synchronisation;
        no CPU or torch fallback (MrgnasError)."""
        self._check_image()
        if not (self.bias.is_cuda and sub.is_cuda and rel.is_cuda):
            raise MrgnasError("CompGCN_ConvE.loss_1n runs on a HIP device (no CPU or torch fallback); got the model on "
                              f"{self.bias.device} and the batch on {sub.device}")
        n_feats, r_feats = self.embed(graph)
        sub_emb, rel_emb = n_feats[sub, :], r_feats[rel, :]
        if not self._hip_ok((n_feats, sub_emb, rel_emb)):
            raise MrgnasError("CompGCN_ConvE.loss_1n runs on a HIP device in float32 without autocast or forward hooks on the scorer's "
                              "submodules (no CPU or torch fallback); use forward and F.binary_cross_entropy otherwise")
        return K.rows_bce_all("dot", None, n_feats, self.query(sub_emb, rel_emb), label_index, sub, rel, label_smooth, col_chunk,
                              _what="CompGCN_ConvE.loss_1n", bias=self.bias)

    def forward(self, graph, sub, rel):
        self._check_image()
        n_feats, r_feats = self.embed(graph)
        sub_emb = n_feats[sub, :]
        rel_emb = r_feats[rel, :]
        if self._hip_ok((n_feats, sub_emb, rel_emb)):
            return K.linear(self.query(sub_emb, rel_emb), n_feats, self.bias, "sigmoid")        # the [B, N] product on the row GEMM
        x = self.bn0(self.concat(sub_emb, rel_emb))
        x = self.feature_drop(F.relu(self.bn1(self.m_conv1(x))))
        x = self.fc(x.view(-1, self.flat_sz))
        x = F.relu(self.bn2(self.hidden_drop(x)))
        x = torch.mm(x, n_feats.transpose(1, 0))
        x += self.bias.expand_as(x)
        return torch.sigmoid(x)
