"""The DARTS architecture step of the reference's search loop (models/architect_lp.py, search/mr_lp_search.py:187-255).

``Architect`` is a drop-in for ``models/architect_lp.Architect``: a supernet forward and backward on a validation sample, then Adam on
the architecture parameters -- ``optim.FusedAdam`` (mrg_adam_step, two launches) when they live on a HIP device, ``torch.optim.Adam``
with the same values otherwise (the host logic then runs on the CPU, against the oracle).  ``search_epoch`` is the body of the
reference's ``train()`` from ``architect.step`` to ``optimizer.zero_grad()``.

Two things the reference does, which a restatement from the DARTS paper would miss:

* its first-order step is a plain ``loss.backward()``: the VALIDATION gradients stay in every weight's ``.grad``, the driver clears
  gradients only at the end of ``train()``, and so the weight step that follows is taken on the sum of the validation and the training
  gradients;
* the score-function alpha (the fifth architecture parameter) never receives a gradient: Adam skips it, its step count stays 0.
  That describes ``supernet.SearchNetwork``; ``supernet.ScoreSearchNetwork``, whose loss ends in the score-function cell, is the
  exception: there the fifth alpha is stepped like the other four.

``unrolled=True`` (the second-order step) cannot run in the reference -- it calls ``model.new()``, which models/model_search_lp.py has
commented out -- and raises here.  ``architect_unrolled.SecondOrderArchitect`` extends this class with that step, restated without
``new()``; ``search_epoch(..., unrolled=True, eta=lr)`` drives it.
"""
import torch


class Architect(object):

    def __init__(self, device, model, args, weight_grads=True):
        """weight_grads=True (the reference): step() runs ``loss.backward()``, which leaves the validation gradients in the weights'
        ``.grad`` for the weight step that follows.  weight_grads=False DEPARTS from the reference's weight step: step() takes
        ``torch.autograd.grad(loss, alphas, allow_unused=True)`` and writes only the alphas' ``.grad``; the weights' ``.grad`` are not
        touched (the weight step then sees training gradients alone) and the weight-gradient products are skipped wherever a Function
        consults ``needs_input_grad``."""
        self.network_momentum = args.momentum
        self.network_weight_decay = args.weight_decay
        self.model = model
        self.weight_grads = bool(weight_grads)
        alphas = list(self.model.arch_parameters())
        hyper = dict(lr=args.arch_learning_rate, betas=(0.5, 0.999), weight_decay=args.arch_weight_decay)
        if all(a.is_cuda for a in alphas):
            from .optim import FusedAdam
            self.optimizer = FusedAdam(alphas, **hyper)
        else:
            self.optimizer = torch.optim.Adam(alphas, **hyper)
        self.device = device
        self.loss = torch.ones(1)

    def step(self, g_train, node_id, src_in, edge_type, data, labels, g_val, node_id_val, src_in_val, edge_type_val, data_val, labels_val,
             eta, optimizer, unrolled):
        """The reference's signature.  `eta` and `optimizer` serve the unrolled step only and are ignored (the reference's own call
        site passes them swapped, search/mr_lp_search.py:231-233); so are the training sample's six arguments."""
        if unrolled:
            raise NotImplementedError("Architect.step(unrolled=True): the reference's second-order step cannot run (it calls model.new(), "
                                      "which models/model_search_lp.py has commented out); only its first-order step is provided")
        self.optimizer.zero_grad()
        self._backward_step(g_val, node_id_val, src_in_val, edge_type_val, data_val, labels_val)
        self.optimizer.step()

    def _backward_step(self, g_train, node_id, src_in, edge_type, data, labels):
        self.loss = self.model._loss(g_train, node_id, src_in, edge_type, data, labels)
        if self.weight_grads:
            self.loss.backward()
            return
        alphas = self.model.arch_parameters()
        for a, g in zip(alphas, torch.autograd.grad(self.loss, alphas, allow_unused=True)):
            a.grad = g


def search_epoch(model, architect, optimizer, train, val, epoch, warm_epochs, grad_norm=None, unrolled=False, eta=None):
    """One epoch of the reference's search loop between sampling and the scheduler (search/mr_lp_search.py:230-253): the architect
    step on `val` when epoch >= warm_epochs, then forward, loss and backward on `train`, gradient clipping, the weight step and
    ``optimizer.zero_grad()``.  train, val: tuples (g, node_id, src_in, edge_type, data, labels).

    An ``optim.ClippedSGD`` clips by its own ``max_norm``; with any other optimiser
    ``clip_grad_norm_(model.parameters(), grad_norm)`` runs before ``optimizer.step()`` (grad_norm=None: no clipping).

    Returns (loss, architect.loss) as tensors on their device: nothing here reads the device (the reference synchronises twice per
    epoch with ``.item()``).  Sampling and the learning-rate scheduler stay with the caller.

    unrolled=True: the second-order architect step (`architect`: an ``architect_unrolled.SecondOrderArchitect``) with `eta`, the
    weights' learning rate (a float or a one-element device tensor; required), and `optimizer` for its momentum buffers."""
    from .optim import ClippedSGD
    if unrolled and eta is None:
        raise ValueError("search_epoch(unrolled=True) needs eta, the weights' learning rate")
    g, node_id, src_in, edge_type, data, labels = train
    if epoch >= warm_epochs:
        architect.step(g, node_id, src_in, edge_type, data, labels, *val, eta if unrolled else None, optimizer, unrolled=bool(unrolled))
    ent, rel = model(g, node_id, src_in, edge_type)
    loss = model.get_loss(g, ent, rel, data, labels)
    loss.backward()
    if not isinstance(optimizer, ClippedSGD) and grad_norm is not None:
        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_norm)
    optimizer.step()
    optimizer.zero_grad()
    return loss.detach(), architect.loss.detach()
