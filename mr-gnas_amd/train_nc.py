"""Epoch drivers of the node-classification task: the bodies of the reference's ``train()`` / ``infer()`` (train/mr_nc_train.py:138-209,
search/mr_nc_search.py:152-224), the slice of DGL's ``NodeDataLoader`` they iterate over, its ``AverageMeter`` bookkeeping kept on
the device, and ``WeightedCE`` (utils/utils.py:162-179).

The networks are ``model_nc.Network`` / ``model_search_nc.Network`` (cells on HIP; classifier and loss on torch).  Nothing here
reads the device per step -- the reference synchronises two or three times per batch with ``.item()`` -- except the block builders'
own size reads: the loss, the accuracy count and the row count of every batch are added into ``Meters`` by in-place device
operations, and ``Meters.result()`` is the epoch's single host read.  CPU models run through the same calls."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import graph as G
from .architect_nc import search_step
from .sampler import NeighborSampler, full_neighbor_blocks


def balanced_weight(target, num_classes):
    """The reference's WeightedCE class weights (V - n_c) / V [n_c > 0] of one batch, without its nonzero / unique host reads."""
    V = target.size(0)
    n = torch.bincount(target, minlength=num_classes)
    return (V - n).float() / V * (n > 0).float()


class WeightedCE(nn.Module):
    """Drop-in for the reference's WeightedCE: cross-entropy under the class weights (V - n_c) / V [n_c > 0] of the batch's own
    label histogram, with ``bincount(minlength=C)`` in place of the reference's nonzero / unique host reads.  A batch of one class
    has no weight left: NaN, as the reference."""

    def __init__(self, num_classes, device):
        super(WeightedCE, self).__init__()
        self.n_classes = num_classes
        self.device = device

    def forward(self, pred, label):
        return F.cross_entropy(pred, label, weight=balanced_weight(label, self.n_classes))


class Meters:
    """The reference's AverageMeters of one epoch on the device: ``sums`` = float64 [3] (sum of loss_b * n_b, sum of correct, sum of
    n_b; n_b = the batch's row count) and ``arch``, a float64 scalar for the architect loss * n_b.  ``update`` is four in-place device
    operations and no host read; ``result()`` is the single host read: (accuracy, loss, architect loss) as the meters' ``avg``."""

    def __init__(self, device):
        self.sums = torch.zeros(3, dtype=torch.float64, device=device)
        self.arch = torch.zeros((), dtype=torch.float64, device=device)

    def update(self, loss, logits, target, arch_loss=None):
        n = logits.shape[0]
        with torch.no_grad():
            self.sums[0].add_(loss.detach().reshape(()), alpha=n)
            self.sums[1].add_((logits.argmax(dim=1) == target).sum())
            self.sums[2].add_(n)
            if arch_loss is not None:
                self.arch.add_(arch_loss.detach().reshape(()), alpha=n)

    def result(self):
        loss_n, correct, n, arch_n = torch.cat((self.sums, self.arch.reshape(1))).tolist()
        if n == 0:
            return 0.0, 0.0, 0.0                             # AverageMeter.avg before any update
        return correct / n, loss_n / n, arch_n / n


class NodeLoader:
    """The slice of DGL's ``NodeDataLoader(graph, nids, sampler, batch_size=, shuffle=, drop_last=)`` the reference uses: iterating
    yields ``(input_nodes, seeds, blocks)`` per batch of ``nids`` -- the blocks outermost first, the last block's destinations =
    ``seeds`` in order, ``input_nodes`` = the first block's source nodes.  sampler: an int (the number of layers: every in-edge,
    ``sampler.full_neighbor_blocks``) or a ``sampler.NeighborSampler``.  shuffle draws ``torch.randperm`` on the CPU from
    ``generator`` once per iteration, so a CPU run and a HIP run see the same batches."""

    def __init__(self, graph, nids, sampler, batch_size, shuffle=False, drop_last=False, generator=None):
        if isinstance(sampler, bool) or not isinstance(sampler, (int, NeighborSampler)):
            raise TypeError("NodeLoader: sampler is a number of layers or a sampler.NeighborSampler")
        if int(batch_size) < 1:
            raise ValueError("NodeLoader: batch_size must be positive")
        self.graph, self.sampler, self.batch_size = graph, sampler, int(batch_size)
        self.nids = torch.as_tensor(nids).long().reshape(-1).to(graph.device)
        self.shuffle, self.drop_last, self.generator = shuffle, drop_last, generator

    def __len__(self):
        n = int(self.nids.numel())
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        nids = self.nids
        if self.shuffle:
            nids = nids[torch.randperm(int(nids.numel()), generator=self.generator).to(nids.device)]
        for b in range(len(self)):
            seeds = nids[b * self.batch_size:(b + 1) * self.batch_size]
            if isinstance(self.sampler, NeighborSampler):
                blocks = self.sampler.sample(seeds)
            else:
                blocks = full_neighbor_blocks(self.graph, seeds, self.sampler)
            yield blocks[0].srcdata[G.NID], seeds, blocks


def _label_index(seeds, inv_target):
    return seeds if inv_target is None else inv_target[seeds]


def train_epoch(model, optimizer, triple_g, loader, labels, inv_target=None, criterion=None, scheduler=None):
    """One training epoch (reference train/mr_nc_train.py:138-178).  Returns (macro_acc, micro_acc, loss): the two accuracies are
    the same number there and here.  criterion: None = the model's own.  A batch of one seed raises in training mode, as the
    reference's BatchNorm does."""
    model.train()
    criterion = model._criterion if criterion is None else criterion
    meters = Meters(labels.device)
    for _, seeds, blocks in loader:
        target = labels[_label_index(seeds, inv_target)]
        optimizer.zero_grad()
        logits = model(triple_g, blocks)
        loss = criterion(logits, target)
        loss.backward()
        optimizer.step()
        meters.update(loss, logits, target)
    if scheduler is not None:
        scheduler.step()
    acc, loss, _ = meters.result()
    return acc, acc, loss


def infer_epoch(model, triple_g, loader, labels, inv_target=None, criterion=None):
    """One evaluation pass (reference train/mr_nc_train.py:181-209).  Returns (macro_acc, micro_acc, loss)."""
    model.eval()
    criterion = model._criterion if criterion is None else criterion
    meters = Meters(labels.device)
    with torch.no_grad():
        for _, seeds, blocks in loader:
            target = labels[_label_index(seeds, inv_target)]
            logits = model(triple_g, blocks)
            meters.update(criterion(logits, target), logits, target)
    acc, loss, _ = meters.result()
    return acc, acc, loss


def search_epoch(model, architect, optimizer, triple_g, loader, val_loader, labels, epoch, warm_epochs, inv_target=None, criterion=None,
                 scheduler=None, unrolled=False):
    """One epoch of the architecture search (reference search/mr_nc_search.py:152-199): per batch the first batch of `val_loader`
    (``next(iter(val_loader))``), ``architect_nc.search_step``, and the three meters.  Returns (acc, loss, arch_loss); arch_loss
    averages ``architect.loss * n``, the stale 1.0 of the warm-up epochs included.

    unrolled=True: the second-order architect step (`architect`: an ``architect_unrolled.SecondOrderArchitectNC``).  Its `eta` is the
    reference's (search/mr_nc_search.py:154): ``scheduler.get_last_lr()[-1]`` at the start of the epoch, or without a scheduler the
    optimiser's own learning rate."""
    model.train()
    criterion = model._criterion if criterion is None else criterion
    meters = Meters(labels.device)
    lr = None
    if unrolled:
        lr = scheduler.get_last_lr()[-1] if scheduler is not None else (optimizer.lr if hasattr(optimizer, "lr") else optimizer.param_groups[0]["lr"])
    for _, seeds, blocks in loader:
        _, val_seeds, val_blocks = next(iter(val_loader))
        idx = _label_index(seeds, inv_target)
        loss, arch_loss, logits = search_step(model, architect, optimizer, triple_g, (idx, blocks),
                                              (_label_index(val_seeds, inv_target), val_blocks), labels, epoch, warm_epochs, criterion,
                                              lr, bool(unrolled))
        meters.update(loss, logits, labels[idx], arch_loss)
    if scheduler is not None:
        scheduler.step()
    return meters.result()
