"""Gradient fan-in of a tensor with several readers: K-way sums, the Fan alias bookkeeping and the running sum that readers add
to in their own stores (csrc/accum.hip; the *_acc2 / _acc / _chain entry points of linear.hip, gate.hip, segreduce.hip).

Part of ``mr_gnas_amd.functional`` (autograd Functions over the C ABI, include/mrgnas.h): every Function enqueues HIP kernels of
libmrgnas_hip.so on torch's current stream through ctypes; every call site states the algorithmic bytes / flops of the launch."""
import weakref

import torch

from .._lib import ptr_array, call, f32c, ptr, require_hip, stream_of
from . import switches as SW
from .reducers import _seg_bwd


def sum_buffers(xs):
    """Sum of equally-shaped HIP tensors in K-way passes (mrg_sum_buffers), k = 0..K-1 order."""
    xs = [f32c(x) for x in xs]
    require_hip(*xs)
    out = torch.empty_like(xs[0])
    n = out.numel()
    for i in range(0, len(xs), 8):
        part = xs[i:i + 8]
        call("mrg_sum_buffers", (ptr_array(part), len(part), ptr(out), n, int(i > 0), stream_of(out)),
             nbytes=4 * n * (len(part) + 1 + int(i > 0)))
    return out


class _Fanout(torch.autograd.Function):
    """k aliases of one tensor whose gradients are summed in one K-way pass instead of k - 1
    pairwise adds.  Aliases nobody reads cost nothing (their gradient stays None).  Readers that take part in the gradient fan-in
    chain (_FanBox.total) have added theirs on the way: the pass covers only what arrived through autograd, and is no launch at all
    when nothing did."""

    @staticmethod
    def forward(ctx, x, k, box):
        ctx.set_materialize_grads(False)
        ctx.box = box                                       # mailbox of this batch of aliases (Fan.take / the readers' backward)
        return tuple(x.view_as(x) for _ in range(k))

    @staticmethod
    def backward(ctx, *grads):
        box = ctx.box
        gs = [g for g in grads if g is not None]
        tot = box.take_total(None)                          # what the chained readers left (None: nobody chained in this backward)
        box.spent = True
        # (a further batch of aliases hangs off the last alias of the previous one: its sum goes there through autograd, as the LAST
        #  term of that batch's sum -- joining that batch's chain instead would add it first and change the sum's association)
        return _Fanout._sum(box, gs, tot), None, None

    @staticmethod
    def _sum(box, gs, tot):
        """The sum of the running sum tot (first), the gradients gs that arrived through autograd (in alias order) and the gathered
        term: tot itself when there is nothing else.  (The chained readers are the ones that ran first, which took their aliases
        last: where they are all of the lowest alias numbers this is the association of the unchained sum.)"""
        if tot is not None:
            gs = [tot] + gs
        gathered = box.gathered
        if gathered is not None:                            # a reader (a_sum) left its gradient as a gather of an [N, D] tensor
            gh, gself, graph, ev = gathered
            box.gathered = None
            cur = torch.cuda.current_stream(gh.device)
            cur.wait_event(ev)                                # the producer's stream may not be this one
            for t in (gh, gself):
                if t is not None:
                    t.record_stream(cur)                      # ... and its allocator must not recycle the blocks under this launch
            E, N, D = graph.num_edges(), graph.number_of_nodes(), gh.shape[1]
            if len(gs) <= 8 and all(g.is_cuda and g.shape == (E + N, D) for g in gs):
                gs = [f32c(g) for g in gs]
                out = torch.empty(E + N, D, dtype=torch.float32, device=gh.device)
                call("mrg_sum_rows_gather", (ptr_array(gs), len(gs), ptr(f32c(gh)), ptr(f32c(gself)), ptr(graph.i32("dst")), E, E + N, D, ptr(out),
                                             stream_of(out)), nbytes=4 * D * (E + N) * (len(gs) + 1))
                return out
            gx = torch.empty(E + N, D, dtype=torch.float32, device=gh.device)      # shapes the kernel does not take: materialise
            if gself is not None:
                gx[E:] = gself
            else:
                gx[E:].zero_()
            _seg_bwd(0, gh, graph, None, gx, None)
            gs.append(gx)
        if not gs:
            return None
        if len(gs) == 1:
            return gs[0]
        if not gs[0].is_cuda or any(g.shape != gs[0].shape for g in gs):
            out = gs[0]
            for g in gs[1:]:
                out = out + g
            return out
        return sum_buffers(gs)


_RAW_STREAM = torch._C._cuda_getCurrentRawStream           # the current stream's handle as an int: no Stream object per deposit / take


def _graph_task():
    """The id of the backward pass that is running (-1: none)."""
    return torch._C._current_graph_task_id()


class _FanBox:
    """Mailbox of one batch of Fan aliases, read by the batch's fan-in sum (_Fanout.backward).

    gathered: a reader whose gradient w.r.t. the alias is a gather of a small tensor (a_sum) leaves the small tensor here instead of
    materialising [rows, D].

    total: the RUNNING SUM of a gradient fan-in chain (switches.FANIN_CHAIN).  A reader that takes part (join below) does not return
    its [rows, D] gradient to autograd: the first one deposits the buffer it wrote, every later one takes the deposit, adds it in the
    store of its own last kernel (in place where it can: the chain allocated the buffer and autograd has not seen it) and deposits the
    result.  When every gradient came this way the fan-in sum returns the deposit without a launch.  A deposit carries the handle of the stream it
    was written on (a taker on another stream orders itself behind that stream's work) and the id of its backward pass (a deposit
    that a backward left behind without reaching the fan-in sum is dropped by the next one).

    spent: the fan-in sum has run; a later backward over the retained graph takes the unchained path."""
    __slots__ = ("gathered", "total", "spent")

    def __init__(self):
        self.gathered = None
        self.total = None
        self.spent = False

    def take_total(self, like):
        """The running sum of this backward pass, handed over to the caller (None: there is none).  like: a tensor the caller will
        add it to -- a deposit of another shape, type or device stays where it is and None is returned with ``self.total`` still
        set (the caller then takes the unchained path); None: any."""
        if self.total is None:
            return None
        buf, stream, task = self.total
        if task != _graph_task():
            self.total = None
            return None
        if like is not None and (buf.shape != like.shape or buf.device != like.device or buf.dtype != like.dtype):
            return None
        self.total = None
        if stream is not None and _RAW_STREAM(buf.get_device()) != stream:
            cur = torch.cuda.current_stream(buf.device)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.ExternalStream(stream, device=buf.device))    # behind everything the depositor's stream holds now, its store included
            cur.wait_event(ev)
            buf.record_stream(cur)
        return buf

    def deposit(self, buf):
        """buf becomes the running sum: a buffer the caller allocated (or took from here) and does not return to autograd."""
        self.total = (buf, _RAW_STREAM(buf.get_device()) if buf.is_cuda else None, _graph_task())


class _Join:
    """A reader's seat in the chain of one backward pass: ``total`` (the running sum to add; None for the first reader) and
    ``deposit(buf)`` for the result.  Between join() and deposit() the mailbox is empty."""
    __slots__ = ("box", "total")

    def __init__(self, box, total):
        self.box, self.total = box, total

    def deposit(self, buf):
        self.box.deposit(buf)


def join(box, like, absorbs_gather=False):
    """Called by a reader's backward for the alias whose mailbox is `box` (Fan.node_of at forward time) before it stores its gradient,
    a HIP tensor shaped like `like`.  Returns a _Join, or None when the gradient has to go back through autograd as it always did: no
    mailbox (the operand was no Fan alias), the switch is off, not a HIP tensor, double backward (create_graph: the gradient must
    stay on the tape), a second backward over a retained graph, a deposit the reader cannot add to (another shape) -- or a gathered
    term waiting in the mailbox that the reader will not add itself (absorbs_gather False): the fan-in sum then needs its pass for
    the gather anyway, adds the gather FIRST as it always did, and a gradient joined now would only change the order of that sum."""
    if box is None or not SW.FANIN_CHAIN or box.spent or not like.is_cuda or torch.is_grad_enabled() or _graph_task() < 0:
        return None
    if box.gathered is not None and not absorbs_gather:
        return None
    tot = box.take_total(like)
    if tot is None and box.total is not None:
        return None
    return _Join(box, tot)


class Fan:
    """Hands out aliases of `x` to its readers: ``fan.take()`` per reader, at most `cap` of them.
    Aliases are created a dozen at a time (a further batch hangs off the last alias of the previous one, so
    its gradients arrive as one pre-summed tensor).  Without autograd (or for tensors that need no
    gradient) the tensor itself is returned."""

    BATCH = 12

    def __init__(self, x, cap):
        self.x = x
        self.left = cap
        self._live = torch.is_grad_enabled() and x.requires_grad and cap > 1
        self._views = []
        self._root = x

    def take(self):
        if not self._live:
            return self.x
        if self.left <= 0:
            raise RuntimeError("Fan: more readers than announced")
        self.left -= 1
        if not self._views:
            self._box = _FanBox()
            views = list(_Fanout.apply(self._root, self.BATCH, self._box))
            self._root = views.pop()                    # source of the next batch, if one is ever needed
            self._views = views
        v = self._views.pop()
        Fan._remember(v, self._box)                     # lets a reader leave its gradient with the fan-in sum (the readers' backward)
        return v

    # alias tensor -> the mailbox of the fan-out batch it came from.  A side table keyed by the alias OBJECT's id (tensors compare
    # elementwise, so they cannot key a dict themselves) holding a weak reference that removes the entry when the alias dies: a reader
    # handed anything else -- a copy, a cast that allocates -- simply is not found and materialises its gradient as usual.
    _NODE = {}

    @staticmethod
    def _remember(v, box):
        key = id(v)
        Fan._NODE[key] = (weakref.ref(v, lambda _r, key=key: Fan._NODE.pop(key, None)), box)

    @staticmethod
    def node_of(x):
        hit = Fan._NODE.get(id(x))
        return hit[1] if hit is not None and hit[0]() is x else None
