"""The second-order (unrolled) DARTS architecture step -- ``--unrolled`` of the reference's two search drivers (models/architect_lp.py:26-103,
models/architect.py:23-99) -- which the reference itself cannot run: its ``_construct_model_from_theta`` calls ``model.new()``.  That is a
fault of its plumbing; the arithmetic is sound and is restated here WITHOUT a second model: the weights are moved in place and put back.

``SecondOrderArchitect`` (link prediction) and ``SecondOrderArchitectNC`` (node classification) extend ``architect.Architect`` and
``architect_nc.Architect`` -- which go on raising for ``unrolled=True`` -- and keep the reference's constructor and ``step`` signatures.
With ``unrolled=False`` they are their parents.  With ``unrolled=True``, for weights theta, alphas a, the training sample's loss L_t and
the validation sample's L_v:

1. g = dL_t(theta, a)/dtheta                                     (``autograd.grad``, allow_unused=False as in the reference; the
                                                                  node-classification class differs, see its docstring)
2. theta' = theta - eta * (momentum * buf + (g + wd * theta))     in place, theta kept in ``backup``; the model's buffers are snapshotted
3. loss = L_v(theta', a);  dalpha = dloss/da,  v = dloss/dtheta'  (one ``autograd.grad``); the buffers are put back
4. R = 0.01 / |v|;  theta = backup + R v;  gp = dL_t/da           (alpha-only backward: the weight-gradient products are skipped)
5. theta = backup - R v;  gn = dL_t/da
6. theta = backup                                                 (a copy: bit for bit)
7. a.grad = dalpha - eta * (gp - gn) / (2 R);  Adam on the alphas

On a HIP device passes 2, 4, 5, 6 and 7 and the norm are mrg_unrolled_* launches over every parameter tensor at once (csrc/optim.hip;
``eta``, |v|, R and 1 / (2 R) live in device memory), anywhere else the same expressions on torch ops: that is how the CPU tests drive the
engine against the oracle.  Nothing in the step reads the device.

What the step leaves behind, as the reference's copy formulation does: the weights' ``.grad`` are not touched (the validation gradients
stay in the reference's copy, so the weight step that follows sees training gradients alone); the model's buffers have seen three
training-mode passes on the training sample and none on the validation sample; the passes run in the reference's order, so random
draws are consumed in its order.  If anything raises after pass 2, parameters and buffers are put back.

Two intended differences from the reference's arithmetic:
* |v| == 0: the reference divides by zero.  Here R = 0 and 1 / (2 R) is stored as 0: the implicit term comes out as zero.
* the reference's ``add_(R, v); sub_(2 R, v); add_(R, v)`` does not give the weights back in float32; here every shifted point is formed
  from ``backup`` and the last pass is a copy.

``dalpha``, ``implicit_grads`` (lists, None for an alpha the loss does not reach) and ``scal`` = [|v|, R, 1 / (2 R)] of the last step stay
on the instance as device tensors.
"""
import torch

from . import _lib, architect, architect_nc
from ._lib import call, ptr, stream_of

R_SMALL = 1e-2          # the reference's r (models/architect_lp.py:88)


class UnrolledEngine:
    """The parameter passes and the order of the second-order step, shared by the two architects."""

    def __init__(self, model, momentum, weight_decay, allow_unused=False):
        """allow_unused: whether a weight the training loss does not reach counts as having a zero gradient in pass 1 (False: the
        reference's ``allow_unused=False``, autograd raises)."""
        self.model = model
        self.momentum, self.weight_decay, self.allow_unused = float(momentum), float(weight_decay), bool(allow_unused)
        self.params = list(model.parameters())
        self.alphas = list(model.arch_parameters())
        buffers = getattr(model, "buffers", None)
        self.buffers = list(buffers()) if callable(buffers) else []
        self._saved = [torch.empty_like(b) for b in self.buffers]      # the snapshot of pass 2: written there, before it is read
        self.hip = all(p.is_cuda for p in self.params) and all(a.is_cuda for a in self.alphas)
        self.dalpha = self.implicit_grads = self.scal = None
        if not self.hip:
            self.backup = None
            return
        from .optim import _ParamTables
        tab = self._tab = _ParamTables("SecondOrderArchitect", self.params, 0, width=2)       # [g | momentum buffers], then [v]
        self._a_tab = _ParamTables("SecondOrderArchitect", self.alphas, 0, width=5)           # [out | ig | dalpha | gp | gn]
        # every slot 256-byte aligned; none of the three is initialised: each is written before it is read
        self._backup_flat, self.backup, self._backup_ptrs = tab.flat_state(64, zero=False)
        self._partial = torch.empty(max(tab.n_chunks, 1), dtype=torch.float64, device=tab.dev)
        self.scal = torch.empty(3, dtype=torch.float32, device=tab.dev)
        self._eta_host = 0.0
        self._eta_dev = torch.zeros(1, dtype=torch.float32, device=tab.dev)

    # ---- the pieces: HIP launches, or the same expressions on torch ops ---------------------------------------------------------
    def _moments(self, optimizer):
        """The momentum buffers of the weights' optimiser, one per parameter, or None for a zero moment (the reference's ``except:``
        branch: any parameter without a buffer).  Returns (tensors or None, device pointer table or None)."""
        if optimizer is None or self.momentum == 0.0:
            return None, None
        from .optim import ClippedSGD
        if isinstance(optimizer, ClippedSGD):
            if len(optimizer.params) == len(self.params) and all(a is b for a, b in zip(optimizer.params, self.params)):
                return optimizer.bufs, (optimizer._b_ptrs if self.hip else None)
            by_param = {id(p): b for p, b in zip(optimizer.params, optimizer.bufs)}
            bufs = [by_param.get(id(p)) for p in self.params]
        else:
            state = getattr(optimizer, "state", None)
            if state is None:
                raise TypeError("the unrolled step takes an optim.ClippedSGD, a torch.optim.SGD or None as `optimizer` (in the "
                                f"declared order: eta, optimizer), not {type(optimizer).__name__}")
            bufs = [state[p].get("momentum_buffer") if p in state else None for p in self.params]
        return (None if any(b is None for b in bufs) else bufs), None

    def _eta(self, eta):
        if eta is None:
            raise ValueError("the unrolled step needs `eta`, the weights' learning rate (a float or a one-element tensor)")
        if not self.hip:
            return eta.detach().reshape(()) if torch.is_tensor(eta) else float(eta)
        if torch.is_tensor(eta):
            if eta.numel() != 1:
                raise ValueError("eta: a float or a ONE-element tensor")
            eta = eta.detach().reshape(1)
            if eta.dtype != torch.float32 or eta.device != self._tab.dev or not eta.is_contiguous():
                eta = eta.to(device=self._tab.dev, dtype=torch.float32).contiguous()
            return eta
        if float(eta) != self._eta_host:
            self._eta_host = float(eta)
            self._eta_dev.fill_(self._eta_host)
        return self._eta_dev

    def _virtual(self, g, optimizer, eta):
        """theta -> theta' in place; theta kept in backup."""
        bufs, b_ptrs = self._moments(optimizer)
        if not self.hip:
            with torch.no_grad():
                self.backup = [p.detach().clone() for p in self.params]
                for i, p in enumerate(self.params):
                    d = 0.0 if g[i] is None else g[i]
                    if self.weight_decay != 0.0:
                        d = d + self.weight_decay * p
                    p.sub_(eta * (self.momentum * bufs[i] + d if bufs is not None else d))
            return
        tab = self._tab
        for i, p in enumerate(self.params):
            if p.data_ptr() != tab._p_ptr_host[i]:
                raise _lib.MrgnasError("SecondOrderArchitect: a parameter's storage moved since construction (build the architect after .to(device))")
        if bufs is None or b_ptrs is not None:               # no moment, or the optimiser's own table of buffer pointers
            held, b_ptrs = tab.stage(g), ptr(b_ptrs)
        else:
            held, b_ptrs = tab.stage(g, bufs), tab.table(1)
        call("mrg_unrolled_virtual_step", (ptr(tab.p_ptrs), tab.table(0), b_ptrs, ptr(self._backup_ptrs), ptr(tab.chunk_tensor),
                                           ptr(tab.chunk_off), ptr(tab.chunk_len), tab.n_chunks, ptr(eta), self.momentum, self.weight_decay,
                                           stream_of(self._backup_flat)))
        del held                                              # (held until here: the launch that reads them is enqueued)
        torch.autograd.graph.increment_version(self.params)   # the kernel wrote the parameters behind autograd's back: say so

    def _radius(self, v):
        """scal = [|v|, R, 1 / (2 R)], and v staged for the shifts.  Returns what must stay alive until the last shift is enqueued."""
        if not self.hip:
            sq = sum((x.detach().double() ** 2).sum() for x in v if x is not None)
            norm = torch.as_tensor(sq, dtype=torch.float64).sqrt()
            zero = torch.zeros_like(norm)
            R = torch.where(norm > 0, R_SMALL / norm, zero)
            self.scal = torch.stack([norm, R, torch.where(R > 0, 1.0 / (2.0 * R), zero)]).to(self.params[0].dtype)
            return v
        tab = self._tab
        held = tab.stage(v)
        call("mrg_unrolled_radius", (tab.table(0), ptr(tab.chunk_tensor), ptr(tab.chunk_off), ptr(tab.chunk_len), tab.n_chunks,
                                     ptr(self._partial), R_SMALL, ptr(self.scal), stream_of(self._backup_flat)))
        return held[0]

    def _snapshot_buffers(self):
        if self.buffers:                                      # (a few hundred BatchNorm statistics and counters: one multi-tensor copy)
            with torch.no_grad():
                torch._foreach_copy_(self._saved, self.buffers)

    def _restore_buffers(self):
        if self.buffers:
            with torch.no_grad():
                torch._foreach_copy_(self.buffers, self._saved)

    def _shift(self, v, sign):
        """theta = backup + sign * R * v, always from backup; sign 0: theta = backup, bit for bit."""
        if not self.hip:
            with torch.no_grad():
                for p, k, x in zip(self.params, self.backup, v if sign else [None] * len(self.params)):
                    p.copy_(k if x is None else k + (sign * self.scal[1]) * x)
            return
        tab = self._tab
        call("mrg_unrolled_shift", (ptr(tab.p_ptrs), ptr(self._backup_ptrs), tab.table(0) if sign else None, ptr(tab.chunk_tensor),
                                    ptr(tab.chunk_off), ptr(tab.chunk_len), tab.n_chunks, ptr(self.scal), int(sign),
                                    stream_of(self._backup_flat)))
        torch.autograd.graph.increment_version(self.params)

    def _combine(self, dalpha, gp, gn, eta):
        """implicit_grads = (gp - gn) / (2 R); returns dalpha - eta * implicit_grads per alpha (None where gp / gn is None)."""
        live = [a is not None and b is not None for a, b in zip(gp, gn)]
        if not self.hip:
            ig = [(a - b) * self.scal[2] if ok else None for a, b, ok in zip(gp, gn, live)]
            self.implicit_grads = ig
            return [((d if d is not None else 0.0) - eta * i) if ok else d for d, i, ok in zip(dalpha, ig, live)]
        tab = self._a_tab
        out = [torch.empty_like(a) if ok else None for a, ok in zip(self.alphas, live)]
        ig = [torch.empty_like(a) if ok else None for a, ok in zip(self.alphas, live)]
        held = tab.stage(out, ig, dalpha, gp, gn)
        call("mrg_unrolled_alpha_grad", (tab.table(0), tab.table(1), tab.table(2), tab.table(3), tab.table(4), ptr(tab.chunk_tensor),
                                         ptr(tab.chunk_off), ptr(tab.chunk_len), tab.n_chunks, ptr(eta), ptr(self.scal),
                                         stream_of(self._backup_flat)))
        del held
        self.implicit_grads = ig
        return [o if ok else d for o, d, ok in zip(out, dalpha, live)]

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    def step(self, train_loss, val_loss, eta, optimizer):
        """train_loss(), val_loss(): the model's loss on the training / validation sample at its CURRENT weights.  Writes the alphas'
        ``.grad`` and returns the validation loss at theta'."""
        params, alphas = self.params, self.alphas
        eta = self._eta(eta)
        g = torch.autograd.grad(train_loss(), params, allow_unused=self.allow_unused)
        self._snapshot_buffers()
        self._virtual(g, optimizer, eta)
        del g
        done = False
        try:
            loss = val_loss()
            grads = torch.autograd.grad(loss, alphas + params, allow_unused=True)
            dalpha, v = list(grads[:len(alphas)]), list(grads[len(alphas):])
            del grads
            self._restore_buffers()                     # the validation pass ran on the reference's COPY: its statistics are dropped
            v = self._radius(v)                              # (as staged: alive until the last shift is enqueued)
            self._shift(v, +1)
            gp = torch.autograd.grad(train_loss(), alphas, allow_unused=True)
            self._shift(v, -1)
            gn = torch.autograd.grad(train_loss(), alphas, allow_unused=True)
            done = True
        finally:
            self._shift(None, 0)
            if not done:
                self._restore_buffers()
        del v
        self.dalpha = dalpha
        for a, grad in zip(alphas, self._combine(dalpha, gp, gn, eta)):
            if grad is not None:
                a.grad = grad
        return loss


class SecondOrderArchitect(architect.Architect):
    """``architect.Architect`` with the second-order step.  ``step(..., eta, optimizer, unrolled)``: the reference's signature; `eta`
    (a float or a one-element device tensor: the weights' learning rate) and `optimizer` (the weights' ``optim.ClippedSGD`` or
    ``torch.optim.SGD``, whose momentum buffers the virtual step reads, or None for a zero moment) are taken in the DECLARED order only
    -- the reference's link-prediction call site passes them swapped (search/mr_lp_search.py:231-233).  The virtual step is not
    clipped, as the reference's is not."""

    def __init__(self, device, model, args, weight_grads=True):
        super().__init__(device, model, args, weight_grads)
        self.engine = UnrolledEngine(model, self.network_momentum, self.network_weight_decay)

    dalpha = property(lambda self: self.engine.dalpha)
    implicit_grads = property(lambda self: self.engine.implicit_grads)
    scal = property(lambda self: self.engine.scal)

    def step(self, g_train, node_id, src_in, edge_type, data, labels, g_val, node_id_val, src_in_val, edge_type_val, data_val, labels_val,
             eta, optimizer, unrolled):
        if not unrolled:
            return super().step(g_train, node_id, src_in, edge_type, data, labels, g_val, node_id_val, src_in_val, edge_type_val, data_val,
                                labels_val, eta, optimizer, unrolled)
        self.optimizer.zero_grad()
        self.loss = self.engine.step(lambda: self.model._loss(g_train, node_id, src_in, edge_type, data, labels),
                                     lambda: self.model._loss(g_val, node_id_val, src_in_val, edge_type_val, data_val, labels_val),
                                     eta, optimizer)
        self.optimizer.step()


class SecondOrderArchitectNC(architect_nc.Architect):
    """``architect_nc.Architect`` with the second-order step; `eta` and `optimizer` as for ``SecondOrderArchitect``.

    One more difference from the reference, without which the step could not run on this supernet: the node-classification Network
    owns weights its loss never reaches (``mean_aggre.linear``, as in the reference's models/model_search.py), and the reference's
    ``autograd.grad(loss, parameters, allow_unused=False)`` raises for them.  Here such a weight has a zero gradient in pass 1 -- its
    virtual step is momentum and weight decay alone -- and, being unreached by the validation loss too, no part in v."""

    def __init__(self, device, model, args):
        super().__init__(device, model, args)
        self.engine = UnrolledEngine(model, self.network_momentum, self.network_weight_decay, allow_unused=True)

    dalpha = property(lambda self: self.engine.dalpha)
    implicit_grads = property(lambda self: self.engine.implicit_grads)
    scal = property(lambda self: self.engine.scal)

    def step(self, triple_g, block, labels, seeds, block_val_search, val_seeds_search, eta, optimizer, unrolled):
        if not unrolled:
            return super().step(triple_g, block, labels, seeds, block_val_search, val_seeds_search, eta, optimizer, unrolled)
        self.optimizer.zero_grad()
        self.loss = self.engine.step(lambda: self.model._loss(triple_g, block, labels, seeds),
                                     lambda: self.model._loss(triple_g, block_val_search, labels, val_seeds_search), eta, optimizer)
        self.optimizer.step()
