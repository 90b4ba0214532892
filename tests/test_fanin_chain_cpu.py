"""The bookkeeping of the gradient fan-in chain (functional/fanin.py: _FanBox.total, join) on CPU tensors with stub readers: deposit,
take, the in-place hand-over of the running sum, what the fan-in sum does with it, and the reset after a backward.  (The HIP readers
and kernels: tests/test_fanin_chain_gpu.py.)"""
import torch

import mr_gnas_amd  # noqa: F401
from mr_gnas_amd import functional as K
from mr_gnas_amd.functional import fanin


class _Scale(torch.autograd.Function):
    """y = c * x for an alias x of a Fan; the backward is a chain member written out by hand (join() itself admits HIP tensors only):
    the first reader deposits the buffer it wrote, a later one adds onto the deposit in place."""

    @staticmethod
    def forward(ctx, x, c, log):
        ctx.box, ctx.c, ctx.log = K.Fan.node_of(x), c, log
        return x * c

    @staticmethod
    def backward(ctx, g):
        mine = g * ctx.c                                   # a buffer of this node's own
        tot = ctx.box.take_total(mine)
        ctx.log.append(("first", id(mine)) if tot is None else ("add", id(tot)))
        if tot is None:
            assert ctx.box.total is None                   # between take and deposit the mailbox is empty
            ctx.box.deposit(mine)
        else:
            tot += mine                                    # the chain owns the buffer: in place
            ctx.box.deposit(tot)
        return None, None, None


def _fan(n, cap=None):
    x = torch.arange(6.0).reshape(2, 3).requires_grad_(True)
    return x, K.Fan(x, cap or n)


def test_deposit_take_and_in_place_hand_over():
    x, fan = _fan(3)
    log = []
    y = _Scale.apply(fan.take(), 2.0, log) + _Scale.apply(fan.take(), 3.0, log) + _Scale.apply(fan.take(), 5.0, log)
    box = fan._box
    g = torch.ones(2, 3)
    y.backward(g)
    assert torch.equal(x.grad, g * 10.0)
    # one buffer travelled: the first reader's, which the two others added onto
    assert [k for k, _ in log] == ["first", "add", "add"] and log[1][1] == log[0][1] == log[2][1]
    # after the backward: nothing left behind, and the batch is marked as summed
    assert box.total is None and box.gathered is None and box.spent


def test_chained_and_plain_readers_are_summed_together():
    x, fan = _fan(4)
    log = []
    y = _Scale.apply(fan.take(), 2.0, log) + fan.take() * 7.0 + _Scale.apply(fan.take(), 3.0, log)
    unread = fan.take()
    y.backward(torch.ones(2, 3))
    del unread
    assert torch.equal(x.grad, torch.full((2, 3), 12.0))


def test_further_batches_of_aliases():
    """More readers than one batch of aliases: each batch has a running sum of its own, and a later batch's sum reaches the batch
    it hangs off through autograd (as the last term of that batch's sum: the association of the unchained path)."""
    n = 2 * K.Fan.BATCH + 3
    x, fan = _fan(n)
    log = []
    y = sum(_Scale.apply(fan.take(), float(i + 1), log) for i in range(n))
    y.backward(torch.ones(2, 3))
    assert torch.equal(x.grad, torch.full((2, 3), n * (n + 1) / 2.0))
    assert sum(k == "first" for k, _ in log) == 3          # one running sum per batch


def test_a_deposit_of_another_backward_pass_or_shape_is_not_taken():
    x, fan = _fan(2)
    a = fan.take()
    box = K.Fan.node_of(a)
    assert box is fan._box
    stale = torch.full((2, 3), 100.0)
    box.deposit(stale)                                     # outside any backward pass
    log = []
    y = _Scale.apply(a, 2.0, log) + _Scale.apply(fan.take(), 3.0, log)
    y.backward(torch.ones(2, 3))
    assert torch.equal(x.grad, torch.full((2, 3), 5.0))    # dropped, not added
    assert log[0][0] == "first"
    # another shape: left where it is, the asker gets nothing
    box2 = fanin._FanBox()
    box2.deposit(torch.zeros(4, 3))
    assert box2.take_total(torch.zeros(2, 3)) is None and box2.total is not None
    assert box2.take_total(None) is not None and box2.total is None


def test_join_declines_what_it_cannot_chain(monkeypatch):
    box = fanin._FanBox()
    t = torch.zeros(2, 3)
    assert fanin.join(None, t) is None                     # the operand was no Fan alias
    assert fanin.join(box, t) is None                      # not a HIP tensor
    monkeypatch.setattr(K.switches, "FANIN_CHAIN", False)
    assert fanin.join(box, t) is None


def test_second_backward_over_a_retained_graph():
    """The stub keeps chaining in the second pass (join() would decline: _FanBox.spent); the deposits of the two passes stay apart."""
    x, fan = _fan(2)
    log = []
    y = _Scale.apply(fan.take(), 2.0, log) + _Scale.apply(fan.take(), 3.0, log)
    g = torch.ones(2, 3)
    y.backward(g, retain_graph=True)
    assert fan._box.spent
    y.backward(g)
    assert torch.equal(x.grad, torch.full((2, 3), 10.0))
    assert [k for k, _ in log] == ["first", "add", "first", "add"]
