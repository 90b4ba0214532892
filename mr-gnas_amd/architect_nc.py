"""The DARTS architecture step of the reference's node-classification search loop (models/architect.py,
search/mr_nc_search.py:162-182).

``Architect`` is a drop-in for ``models/architect.Architect``: a supernet forward and backward on a validation block, then Adam on
the architecture parameters -- ``optim.FusedAdam`` (mrg_adam_step) when they live on a HIP device, ``torch.optim.Adam`` with the
same values otherwise.  ``search_step`` is the body of the reference's ``train()`` loop for one batch.

Where this loop differs from the link-prediction one (``architect.search_epoch``), as the reference's two drivers differ:

* the architect step runs when ``epoch > warm_epochs`` (strictly);
* ``optimizer.zero_grad()`` follows the architect step: the validation gradients it left in the weights are discarded, and the weight
  step is taken on the training sample's gradients alone;
* no gradient clipping.

``unrolled=True`` (the second-order step) raises: it calls ``model.new()``, which cannot run in the reference either.
``architect_unrolled.SecondOrderArchitectNC`` extends this class with that step, restated without ``new()``;
``search_step(..., lr=lr, unrolled=True)`` drives it.
"""
import torch


class Architect(object):

    def __init__(self, device, model, args):
        self.network_momentum = args.momentum
        self.network_weight_decay = args.weight_decay
        self.model = model
        alphas = list(self.model.arch_parameters())
        hyper = dict(lr=args.arch_learning_rate, betas=(0.5, 0.999), weight_decay=args.arch_weight_decay)
        if all(a.is_cuda for a in alphas):
            from .optim import FusedAdam
            self.optimizer = FusedAdam(alphas, **hyper)
        else:
            self.optimizer = torch.optim.Adam(alphas, **hyper)
        self.device = device
        self.loss = torch.ones(1, device=alphas[0].device)     # (the reference: on the CPU) where the alphas live, like every later loss

    def step(self, triple_g, block, labels, seeds, block_val_search, val_seeds_search, eta, optimizer, unrolled):
        """The reference's signature.  The training block and seeds, `eta` and `optimizer` serve the unrolled step only."""
        if unrolled:
            raise NotImplementedError("Architect.step(unrolled=True): the reference's second-order step cannot run (it calls model.new(), "
                                      "whose constructor call has the wrong argument list); only its first-order step is provided")
        self.optimizer.zero_grad()
        self._backward_step(triple_g, block_val_search, labels, val_seeds_search)
        self.optimizer.step()

    def _backward_step(self, triple_g, block, labels, seeds):
        self.loss = self.model._loss(triple_g, block, labels, seeds)
        self.loss.backward()


def search_step(model, architect, optimizer, triple_g, train, val, labels, epoch, warm_epochs, criterion, lr=None, unrolled=False):
    """One batch of the reference's search loop (search/mr_nc_search.py:162-182): the architect step on `val` when
    epoch > warm_epochs, ``optimizer.zero_grad()``, then forward, loss, backward and the weight step on `train`.
    train, val: (seeds, blocks) with the seeds already mapped to label indices; lr: the `eta` handed to the architect (unused by
    the first-order step).

    Returns (loss, architect.loss, logits) as detached tensors on their device: nothing here reads the device (the reference
    synchronises with ``.item()`` three times per batch).  Sampling, accuracy bookkeeping and the scheduler stay with the caller.

    unrolled=True: the second-order architect step (`architect`: an ``architect_unrolled.SecondOrderArchitectNC``); `lr` (a float or
    a one-element device tensor) is then required."""
    if unrolled and lr is None:
        raise ValueError("search_step(unrolled=True) needs lr, the weights' learning rate (the architect's eta)")
    seeds, blocks = train
    val_seeds, val_blocks = val
    if epoch > warm_epochs:
        architect.step(triple_g, blocks, labels, seeds, val_blocks, val_seeds, lr, optimizer, unrolled=bool(unrolled))
    optimizer.zero_grad()
    logits = model(triple_g, blocks)
    loss = criterion(logits, labels[seeds])
    loss.backward()
    optimizer.step()
    return loss.detach(), architect.loss.detach(), logits.detach()
