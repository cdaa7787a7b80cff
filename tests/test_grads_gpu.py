"""dfu_hip.grads on the GPU: which stream a parameter's gradient is noted to come from, when that
note turns MIXED and who clears it, and which optimizers the global step pre-hook joins for.
Every case is one hnn.Linear(8, 4) at batch 2 (LinearFn's exact-fp32 small path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _linear(seed):
    from dfu_hip import nn as hnn
    from dfu_hip import streams
    streams.join_grad_streams()  # whatever an earlier test left noted
    torch.manual_seed(seed)
    return hnn.Linear(8, 4).to(DEV), torch.randn(2, 8, device=DEV)


def _backward(lin, x, stream=None):
    """One forward and backward of lin on `stream` (autograd runs a node's backward on its
    forward's stream), ordered after and before the current stream's work."""
    from dfu_hip import streams
    if stream is None:
        lin(x).sum().backward()
        return
    cur = streams.current_stream()
    streams.stream_wait(stream, cur)
    with streams.on_stream(stream):
        lin(x).sum().backward()
    streams.stream_wait(cur, stream)


def test_producer_is_the_stream_that_ran_the_backward():
    from dfu_hip import grads, streams
    lin, x = _linear(0)
    assert grads.producer(lin.weight) is None and grads.producer(lin.bias) is None
    assert not streams.grad_streams
    _backward(lin, x)
    cur = streams.current_stream()
    assert grads.producer(lin.weight) is cur
    assert grads.producer(lin.bias) is cur
    assert list(streams.grad_streams.values()) == [cur]
    streams.join_grad_streams()
    assert not streams.grad_streams
    assert grads.producer(lin.weight) is cur  # a join clears the stream set, not the producers
    torch.cuda.synchronize()
    assert torch.equal(lin.weight.grad, x.sum(0).expand(4, 8))


def test_producer_on_a_side_stream_then_mixed_then_cleared():
    from dfu_hip import grads, streams
    lin, x = _linear(1)
    side = streams.side_stream(DEV)
    assert side != streams.current_stream()
    _backward(lin, x, side)
    # (equal, not identical: the producer is the cached current-stream object of that handle)
    assert grads.producer(lin.weight) == side
    assert grads.producer(lin.bias) == side
    assert list(streams.grad_streams.values()) == [side]
    _backward(lin, x)  # a second producer stream, no clear in between
    assert grads.producer(lin.weight) is grads.MIXED
    assert grads.producer(lin.bias) is grads.MIXED
    assert set(streams.grad_streams.values()) == {side, streams.current_stream()}
    grads.clear_producers([lin.weight, lin.bias])
    assert grads.producer(lin.weight) is None and grads.producer(lin.bias) is None
    streams.join_grad_streams()
    torch.cuda.synchronize()
    assert torch.equal(lin.weight.grad, 2 * x.sum(0).expand(4, 8))  # both passes accumulated


def _counting_join(monkeypatch):
    from dfu_hip import streams
    real, calls = streams.join_grad_streams, []

    def join(*a, **k):
        calls.append((a, k))
        return real(*a, **k)
    monkeypatch.setattr(streams, "join_grad_streams", join)
    return calls


def test_fused_adamw_clears_the_producers_and_joins_by_itself(monkeypatch):
    from dfu_hip import grads, streams
    from dfu_hip.optim import FusedAdamW
    lin, x = _linear(2)
    opt = FusedAdamW(lin.parameters(), lr=1e-2)
    before = lin.weight.detach().clone()
    _backward(lin, x, streams.side_stream(DEV))
    assert grads.producer(lin.weight) == streams.side_stream(DEV)
    assert streams.grad_streams
    calls = _counting_join(monkeypatch)
    opt.step()
    assert len(calls) == 1, "FusedAdamW.step joins once itself; the global pre-hook must not"
    assert not streams.grad_streams
    assert all(grads.producer(p) is None for p in lin.parameters())
    assert not grads.join_armed()
    torch.cuda.synchronize()
    assert not torch.equal(lin.weight.detach(), before)


def test_the_step_pre_hook_joins_for_any_other_optimizer(monkeypatch):
    from dfu_hip import grads, streams
    lin, x = _linear(3)
    side = streams.side_stream(DEV)
    opt = torch.optim.SGD(lin.parameters(), lr=1e-2)
    before = lin.weight.detach().clone()
    _backward(lin, x, side)
    assert list(streams.grad_streams.values()) == [side]
    calls = _counting_join(monkeypatch)
    opt.step()
    assert len(calls) == 1 and calls[0] == ((), {})  # the pre-hook's clearing join
    assert not streams.grad_streams
    assert grads.producer(lin.weight) == side  # only the parameters' own optimizer clears it
    torch.cuda.synchronize()
    # p - lr g with g = the column sums of x: two roundings of values below 1 (ulp 6e-8 each)
    want = before - 1e-2 * x.sum(0).expand(4, 8)
    assert (lin.weight.detach() - want).abs().max().item() <= 2.5e-7
