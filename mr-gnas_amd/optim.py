"""The optimisers of the reference's drivers, each as ONE call over every parameter tensor.

``ClippedSGD``: the reference's search step ends with ``torch.nn.utils.clip_grad_norm_(model.parameters(), grad_norm)`` and
``optimizer.step()`` of ``torch.optim.SGD(lr, momentum, weight_decay)`` (search/mr_lp_search.py:118-119,243-245).  On ~300
parameter tensors torch issues ~30 ``multi_tensor_apply`` launches for the pair; ``ClippedSGD.step()`` is the same arithmetic
(same clip coefficient, same momentum recurrence, buffers starting at zero = torch's ``buf = grad`` first step) through a device
table of pointers (mrg_clip_sgd_step: three launches).

``FusedAdam``: ``torch.optim.Adam`` (the architect's optimiser, models/architect_lp.py:20-22, and the training driver's,
train/mr_lp_train.py:140) through the same tables (mrg_adam_step: two launches), with the step counts and the learning rate in
device memory, so that a step captured into a HIP graph advances its bias correction and follows a schedule on replay.

The product path has no CPU form: CPU parameters raise.
"""
import torch

from . import _lib
from ._lib import call, ptr, stream_of


class _ParamTables:
    """What the optimisers share: the parameter list cut into fixed chunks (device tables, built once: the shapes never change), the
    device table of parameter pointers, and the per-step table of gradient pointers -- staged through pinned memory, with pinned
    tables of their own for steps captured into HIP graphs."""

    def __init__(self, who, params, capture_tables, width=1):
        """width: how many tensor lists one stage() call may place side by side in g_ptrs (stage_grads() uses the first)."""
        self.who = who
        self.width = int(width)
        self.params = [p for p in params]
        if not self.params:
            raise ValueError(f"{who}: no parameters")
        dev = self.dev = self.params[0].device
        for p in self.params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise _lib.MrgnasError(f"{who}: parameters must be contiguous float32 tensors on one HIP device")
        chunk = int(_lib.load().mrg_optim_chunk())
        self.sizes = [p.numel() for p in self.params]
        t_idx, c_off, c_len = [], [], []
        for t, n in enumerate(self.sizes):
            for a in range(0, n, chunk):
                t_idx.append(t)
                c_off.append(a)
                c_len.append(min(chunk, n - a))
        self.n_chunks = len(t_idx)
        self.chunk_tensor = torch.tensor(t_idx, dtype=torch.int32, device=dev)
        self.chunk_off = torch.tensor(c_off, dtype=torch.int64, device=dev)
        self.chunk_len = torch.tensor(c_len, dtype=torch.int32, device=dev)
        self._p_ptr_host = [p.data_ptr() for p in self.params]
        self.p_ptrs = torch.tensor(self._p_ptr_host, dtype=torch.int64, device=dev)
        # pinned staging for the gradient pointers: two buffers used in turn, each guarded by the event of the copy that last read it
        # (the host may run a whole step ahead of the device)
        self._g_host = [torch.zeros(self.width * len(self.params), dtype=torch.int64).pin_memory() for _ in range(2)]
        self._g_np = [h.numpy() for h in self._g_host]      # the same pinned memory: one vectorised write per step
        self._g_event = [None, None]
        self._turn = 0
        self._captured = []
        self._spare = [torch.zeros(len(self.params), dtype=torch.int64).pin_memory() for _ in range(capture_tables)]
        self.g_ptrs = torch.zeros(self.width * len(self.params), dtype=torch.int64, device=dev)

    def table(self, j):
        """Device address of the j-th pointer table inside g_ptrs (what stage() filled with its j-th list)."""
        import ctypes
        return ctypes.c_void_p(self.g_ptrs.data_ptr() + 8 * j * len(self.params))

    def flat_state(self, pad=1, zero=True):
        """One zeroed float32 allocation with a slot per parameter (each padded to a multiple of `pad` elements): the allocation, the
        per-parameter views, and the device table of their pointers.  zero=False: left as allocated, for a slot that is always
        written before it is read."""
        offs, o = [], 0
        for n in self.sizes:
            offs.append(o)
            o += -(-n // pad) * pad
        flat = torch.zeros(o, dtype=torch.float32, device=self.dev) if zero else torch.empty(o, dtype=torch.float32, device=self.dev)
        views = [flat[a:a + n].view_as(p) for a, n, p in zip(offs, self.sizes, self.params)]
        return flat, views, torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device=self.dev)

    def stage_grads(self):
        """Fill g_ptrs (in stream order) with where autograd left the gradients: 0 for a parameter without one; a gradient that is not
        a contiguous float32 tensor is made one, as torch does.  Returns the gradients: the caller holds them until its launches
        are enqueued (the caching allocator hands their memory out again in stream order)."""
        grads = []
        for i, p in enumerate(self.params):
            if p.data_ptr() != self._p_ptr_host[i]:
                raise _lib.MrgnasError(f"{self.who}: a parameter's storage moved since construction (build the optimiser after .to(device))")
            g = p.grad
            if g is not None and (g.dtype != torch.float32 or not g.is_contiguous()):
                g = g.float().contiguous()
            grads.append(g)
        self._copy_in([0 if g is None else g.data_ptr() for g in grads])
        return grads

    def stage(self, *lists):
        """stage_grads() for GIVEN tensors (what ``torch.autograd.grad`` returned, an optimiser's momentum buffers): up to `width`
        lists of one entry per parameter (a tensor or None; a whole list may be None), placed side by side in g_ptrs -- list j at
        table(j) -- by ONE copy through the same pinned double buffer.  A tensor that is not contiguous float32 is made so.  Returns
        the tensors as staged, list by list: the caller holds them until its launches are enqueued."""
        n = len(self.params)
        if not 1 <= len(lists) <= self.width:
            raise ValueError(f"{self.who}: stage() takes 1..{self.width} tensor lists")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MrgnasError(f"{self.who}: stage() inside a graph capture is not supported")
        held, ptrs = [], []
        for ts in lists:
            ts = [None] * n if ts is None else list(ts)
            if len(ts) != n:
                raise ValueError(f"{self.who}: stage(): a list of {len(ts)} tensors for {n} parameters")
            for i, t in enumerate(ts):
                if t is None:
                    continue
                if t.dtype != torch.float32 or not t.is_contiguous():
                    t = ts[i] = t.float().contiguous()
                if t.numel() != self.sizes[i] or t.device != self.dev:
                    raise _lib.MrgnasError(f"{self.who}: stage(): tensor {i} does not match its parameter")
            held.append(ts)
            ptrs.extend(0 if t is None else t.data_ptr() for t in ts)
        self._copy_in(ptrs)
        return held

    def _copy_in(self, ptrs):
        """The first len(ptrs) entries of g_ptrs, in stream order."""
        full = len(ptrs) == self.g_ptrs.numel()
        if torch.cuda.is_current_stream_capturing():
            # the captured copy node reads its host buffer again on every replay: a buffer of its own, never rewritten (the gradients
            # of a captured step live at fixed addresses of the graph's memory pool)
            if not self._spare:                              # (pinning allocates: not allowed while a capture is open)
                raise _lib.MrgnasError(f"{self.who}: more captures than spare pinned pointer tables ({self.who}.CAPTURE_TABLES)")
            host = self._spare.pop()
            host.numpy()[:] = ptrs                           # (stage_grads() of a width-1 table: the only captured form)
            self._captured.append(host)
            self.g_ptrs.copy_(host, non_blocking=True)
        else:
            k = self._turn
            self._turn ^= 1
            if self._g_event[k] is not None:
                self._g_event[k].synchronize()              # normally long complete
            else:
                self._g_event[k] = torch.cuda.Event()
            if full:
                self._g_np[k][:] = ptrs
                self.g_ptrs.copy_(self._g_host[k], non_blocking=True)
            else:
                self._g_np[k][:len(ptrs)] = ptrs
                self.g_ptrs[:len(ptrs)].copy_(self._g_host[k][:len(ptrs)], non_blocking=True)
            self._g_event[k].record()


class ClippedSGD:
    CAPTURE_TABLES = 4          # step() calls that may be captured into HIP graphs over the optimiser's life (one pinned table each)

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, max_norm=0.0):
        self._tab = _ParamTables("ClippedSGD", params, self.CAPTURE_TABLES)
        self.params = self._tab.params
        self.lr, self.momentum, self.weight_decay, self.max_norm = float(lr), float(momentum), float(weight_decay), float(max_norm)
        self._flat, self.bufs, self._b_ptrs = self._tab.flat_state()                     # the momentum buffers, one allocation
        self.n_chunks = self._tab.n_chunks
        self._partial = torch.empty(max(self.n_chunks, 1), dtype=torch.float64, device=self._tab.dev)
        self.norm_coef = torch.zeros(2, dtype=torch.float32, device=self._tab.dev)      # [total gradient norm, clip coefficient] of the last step

    def step(self):
        """Clip (when max_norm > 0) and update.  Gradients are read where autograd left them; a parameter without a gradient, or
        whose gradient is not a contiguous float32 tensor, is handled as torch does (skipped / made contiguous)."""
        tab = self._tab
        grads = tab.stage_grads()
        call("mrg_clip_sgd_step", (ptr(tab.p_ptrs), ptr(tab.g_ptrs), ptr(self._b_ptrs), ptr(tab.chunk_tensor), ptr(tab.chunk_off),
                                   ptr(tab.chunk_len), self.n_chunks, ptr(self._partial), ptr(self.norm_coef), self.max_norm, self.lr,
                                   self.momentum, self.weight_decay, stream_of(self._flat)))
        del grads                                             # (held until here: the launches that read them are enqueued)
        torch.autograd.graph.increment_version(self.params)   # the kernels wrote the parameters behind autograd's back: say so
        return self.norm_coef

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def state_dict(self):
        return {"momentum_buffers": [b.clone() for b in self.bufs], "lr": self.lr, "momentum": self.momentum,
                "weight_decay": self.weight_decay, "max_norm": self.max_norm}

    def load_state_dict(self, state):
        for b, s in zip(self.bufs, state["momentum_buffers"]):
            b.copy_(s)
        self.lr, self.momentum = float(state["lr"]), float(state["momentum"])
        self.weight_decay, self.max_norm = float(state["weight_decay"]), float(state["max_norm"])


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) -- amsgrad and maximize off -- as one mrg_adam_step call.  A
    torch.optim.Optimizer, so torch.optim.lr_scheduler.* drives it (step() reads param_groups[0]['lr']); one parameter group.

    state[p] = {'step', 'exp_avg', 'exp_avg_sq'}: VIEWS of flat device buffers the kernels address through pointer tables built at
    construction -- they exist from the start (all zero) and are never replaced; load_state_dict copies into them.  'step' is per
    parameter, as torch's: a parameter without a gradient in some step is skipped and lags behind.

    Captured into a HIP graph, a step advances its own bias correction on every replay; set_lr(x) changes the learning rate between
    replays (the kernels read it from device memory)."""

    CAPTURE_TABLES = 4          # step() calls that may be captured into HIP graphs over the optimiser's life (one pinned table each)
    PAD = 64                    # elements a parameter's slot in the moment buffers is padded to: every slot starts 256-byte aligned

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        self._tab = None
        super().__init__(params, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay)))
        tab = self._tab = _ParamTables("FusedAdam", self.param_groups[0]["params"], self.CAPTURE_TABLES)
        self._m_flat, self._m, self._m_ptrs = tab.flat_state(self.PAD)
        self._v_flat, self._v, self._v_ptrs = tab.flat_state(self.PAD)
        n = len(tab.params)
        self._steps = torch.zeros(n, dtype=torch.float32, device=tab.dev)               # torch's state['step'], one per parameter
        self._scal = torch.zeros(n, 2, dtype=torch.float32, device=tab.dev)             # the tick kernel's [step size, 1 / sqrt(bias correction 2)]
        self._lr_host = self.param_groups[0]["lr"]
        self._lr_dev = torch.full((1,), self._lr_host, dtype=torch.float32, device=tab.dev)
        for i, p in enumerate(tab.params):
            self.state[p] = {"step": self._steps[i], "exp_avg": self._m[i], "exp_avg_sq": self._v[i]}

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("FusedAdam: one parameter group only")
        super().add_param_group(param_group)

    def set_lr(self, lr):
        """New learning rate, in stream order: for use between replays of a captured step (and anywhere else)."""
        self.param_groups[0]["lr"] = self._lr_host = float(lr)
        self._lr_dev.fill_(self._lr_host)

    @torch.no_grad()
    def step(self, closure=None):
        """Update every parameter that has a gradient.  Gradients are read where autograd left them; a parameter without a gradient,
        or whose gradient is not a contiguous float32 tensor, is handled as torch does (skipped / made contiguous)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group, tab = self.param_groups[0], self._tab
        if group["lr"] != self._lr_host:                      # a scheduler (or the caller) changed it
            if torch.cuda.is_current_stream_capturing():      # (a captured fill would reset the rate on every replay)
                raise _lib.MrgnasError("FusedAdam: the learning rate changed inside a graph capture: call set_lr() before capturing")
            self.set_lr(group["lr"])
        grads = tab.stage_grads()
        b1, b2 = group["betas"]
        call("mrg_adam_step", (ptr(tab.p_ptrs), ptr(tab.g_ptrs), ptr(self._m_ptrs), ptr(self._v_ptrs), len(tab.params), ptr(tab.chunk_tensor),
                               ptr(tab.chunk_off), ptr(tab.chunk_len), tab.n_chunks, ptr(self._steps), ptr(self._scal), ptr(self._lr_dev),
                               float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), stream_of(self._m_flat)))
        del grads                                             # (held until here: the launches that read them are enqueued)
        torch.autograd.graph.increment_version(tab.params)    # the kernels wrote the parameters behind autograd's back: say so
        return loss

    def state_dict(self):
        """torch.optim.Optimizer's layout (what torch.optim.Adam over the same parameters writes), the state tensors copied."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.clone() if torch.is_tensor(t) else t) for n, t in st.items()} for k, st in sd["state"].items()}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Copies INTO the flat buffers (the pointer tables stay valid).  Accepts its own state_dict() and that of a torch.optim.Adam
        over the same parameter list: a parameter torch has not stepped yet has no entry there and starts from zero."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._tab.params):
            raise ValueError("FusedAdam.load_state_dict: one parameter group over the same parameter list expected")
        g = groups[0]
        if g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("FusedAdam.load_state_dict: amsgrad / maximize states are not supported")
        entries = []
        for i, key in enumerate(g["params"]):
            st = state_dict["state"].get(key)
            if st is not None and tuple(st["exp_avg"].shape) != tuple(self._m[i].shape):
                raise ValueError(f"FusedAdam.load_state_dict: parameter {i}: state of shape {tuple(st['exp_avg'].shape)}")
            entries.append(st)
        for i, st in enumerate(entries):
            if st is None:
                self._steps[i].zero_()
                self._m[i].zero_()
                self._v[i].zero_()
            else:
                self._steps[i].copy_(torch.as_tensor(st["step"], dtype=torch.float32))
                self._m[i].copy_(st["exp_avg"])
                self._v[i].copy_(st["exp_avg_sq"])
        mine = self.param_groups[0]
        lr = g["lr"]
        mine["betas"], mine["eps"] = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        mine["weight_decay"] = float(g["weight_decay"])
        if "initial_lr" in g:                                  # what a scheduler left in the group travels with it
            mine["initial_lr"] = g["initial_lr"]
        self.set_lr(float(lr))
