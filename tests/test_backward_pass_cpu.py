"""Host state that lives for one backward pass (ops._first_in_pass, dp.FlatModel.begin_backward, ops.deferring) on the CPU:
passes are told apart by the autograd engine's graph-task id, so a backward that raises - the engine then runs none of its
end-of-backward callbacks - must leave nothing behind that changes the next one.  No HIP library is needed: the tape nodes
here are toy Functions whose backward goes through ops._bw like every real one, over an nn.Linear whose own gradients
autograd accumulates into the flat buffer through `.grad`."""
import types

import pytest
import torch

from sbl_for_multilingual_lip_reading_amd import dp, ops


class _Twice(torch.autograd.Function):
    """y = 2 x; the backward raises while `_Twice.fail` is set."""
    fail = False

    @staticmethod
    def forward(ctx, x):
        return x * 2

    @staticmethod
    @ops._bw
    def backward(ctx, dy):
        if _Twice.fail:
            raise RuntimeError("told to fail")
        return dy * 2


class _TwiceNested(torch.autograd.Function):
    """y = 2 x as well, but the factor of the backward comes out of a second backward pass, run inside this node over a
    small graph of its own that holds an ops._bw node too (what torch.utils.checkpoint does)."""

    @staticmethod
    def forward(ctx, x):
        return x * 2

    @staticmethod
    @ops._bw
    def backward(ctx, dy):
        outer = torch._C._current_graph_task_id()
        with torch.enable_grad():
            z = torch.ones(1, requires_grad=True)
            (two,) = torch.autograd.grad(_Twice.apply(z).sum(), z)
        assert torch._C._current_graph_task_id() == outer
        return dy * two


class _Probe(torch.autograd.Function):
    """Identity whose backward asks twice whether `key` is new in the running pass, logs both answers and the pass id."""

    @staticmethod
    def forward(ctx, x, key, log, fail):
        ctx.key, ctx.log, ctx.fail = key, log, fail
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        ctx.log.append((ops._first_in_pass(ctx.key), ops._first_in_pass(ctx.key), torch._C._current_graph_task_id()))
        if ctx.fail:
            raise RuntimeError("told to fail")
        return dy, None, None, None


def test_first_in_pass_is_true_once_per_pass_and_after_a_failed_pass():
    key, log = types.SimpleNamespace(), []
    x = torch.ones(2, requires_grad=True)

    def run(fail=False):
        del log[:]
        _Probe.apply(_Probe.apply(x, key, log, fail), key, log, False).sum().backward()

    run()
    assert [e[:2] for e in log] == [(True, False), (False, False)] and log[0][2] == log[1][2] != -1
    first = log[0][2]
    run()                                         # the next pass
    assert [e[:2] for e in log] == [(True, False), (False, False)] and log[0][2] > first
    with pytest.raises(RuntimeError, match="told to fail"):
        run(fail=True)                            # the node nearer the input raises: the pass never ends
    assert [e[:2] for e in log] == [(True, False), (False, False)]
    run()                                         # ...and the pass after it starts afresh
    assert [e[:2] for e in log] == [(True, False), (False, False)]
    # outside a backward there is no pass to remember
    assert torch._C._current_graph_task_id() == -1
    assert ops._first_in_pass(key) and ops._first_in_pass(key)


def _flat_linear():
    torch.manual_seed(0)
    lin = torch.nn.Linear(4, 4)
    return lin, dp.FlatModel(lin)


def _loss(lin, x, fn=_Twice):
    return (fn.apply(lin(x)) ** 2).sum()


X_BAD, X_GOOD = torch.arange(8.0).view(2, 4) / 8 - 0.3, torch.arange(12.0).view(3, 4) / 5 - 1.0


@pytest.fixture(scope="module")
def good_grad():
    """flat_grad of a fresh model after ONE backward of the X_GOOD loss (kept unchanged by the tests that compare with it)."""
    lin, fm = _flat_linear()
    _loss(lin, X_GOOD).backward()
    assert float(fm.flat_grad.abs().max()) > 0
    return fm.flat_grad.clone()


def _attached(lin):
    return all(p.grad is p._sbl_grad for p in lin.parameters())


def test_flat_model_recovers_after_a_backward_that_raised(good_grad):
    lin, fm = _flat_linear()
    _Twice.fail = True
    try:
        with pytest.raises(RuntimeError, match="told to fail"):
            _loss(lin, X_BAD).backward()
    finally:
        _Twice.fail = False
    for p in lin.parameters():
        p.grad = None                             # torch.optim's zero_grad()
    _loss(lin, X_GOOD).backward()
    assert _attached(lin)
    assert torch.equal(fm.flat_grad, good_grad)
    _loss(lin, X_GOOD).backward()                 # nothing dropped this time: accumulates
    assert _attached(lin) and torch.equal(fm.flat_grad, 2 * good_grad)


def test_flat_model_accumulates_over_backwards_without_zeroing(good_grad):
    lin, fm = _flat_linear()
    _loss(lin, X_GOOD).backward()
    _loss(lin, X_GOOD).backward()
    assert _attached(lin) and torch.equal(fm.flat_grad, 2 * good_grad)


def test_flat_model_reference_loop_order_on_cpu(good_grad):
    """Forward, THEN every `.grad` dropped, then backward: one zeroed and re-attached gradient per step, not two steps' sum."""
    lin, fm = _flat_linear()
    for _ in range(2):
        loss = _loss(lin, X_GOOD)
        for p in lin.parameters():
            p.grad = None
        loss.backward()
        assert _attached(lin) and torch.equal(fm.flat_grad, good_grad)


def test_flat_model_nested_backward_pass(good_grad):
    """A pass nested in a node re-enters begin_backward (another graph-task id, then the outer one again); that must neither
    zero nor double anything: same flat gradient as the twin without nesting."""
    lin, fm = _flat_linear()
    loss = _loss(lin, X_GOOD, _TwiceNested)
    for p in lin.parameters():
        p.grad = None
    loss.backward()
    assert _attached(lin) and torch.equal(fm.flat_grad, good_grad)
    _loss(lin, X_GOOD, _TwiceNested).backward()
    assert torch.equal(fm.flat_grad, 2 * good_grad)


def test_deferring_scope_ends_when_the_forward_raises():
    with pytest.raises(ZeroDivisionError):
        with ops.deferring():
            assert isinstance(ops._tls.collector, ops.WgradCollector)
            1 / 0
    assert ops._tls.collector is None
