"""How a parameter's gradient is produced, announced, joined and consumed.

  * Who writes: a Function's backward takes ``grad_buffer(p)`` (``grad_or_none(p)`` where p may
    not want one) and its kernels ACCUMULATE into that persistent ``p.grad`` on the stream that is
    current then; backward returns None for p, so .grad addresses stay stable for graph replay,
    the fused optimizer and bucketed all-reduce.  It calls ``grads_done(p, ...)`` once p's
    gradient is complete, which runs the grad-ready hooks (data-parallel bucketing).
  * Producer: the one stream that wrote p's gradient since the last reset -- ``producer(p)``
    gives that stream, None (nothing written yet) or MIXED (several streams, or an unknown one).
    The streams themselves are collected in ``streams.grad_streams``.
  * Who clears: the consumer that has used every gradient of the step, i.e. the optimizer that
    owns the parameters (FusedAdamW.step -> ``clear_producers``).  Nothing else resets it.
  * Who joins: ``streams.join_grad_streams`` makes a stream wait for every producer stream.
    FusedAdamW.step and GradAllReducer call it themselves (``mark_self_joining``); for any other
    reader of p.grad the first encoder-boundary backward arms an end-of-backward join
    (``arm_backward_join``), and every other torch.optim optimizer joins in a step pre-hook.

Imports torch, ops and streams only: optim, parallel, graphs, nn and functional import this.
"""
import torch

from . import ops
from . import streams
from .streams import current_stream
from .streams import grad_streams as _grad_streams  # grad_buffer stores into it directly

# producer(p) when more than one stream, or an unknown one, wrote p's gradient
MIXED = False

_grad_ready_hooks = []


def register_grad_ready_hook(fn):
    """fn(param) is called after a Function has finished writing param.grad (DP bucketing)."""
    _grad_ready_hooks.append(fn)
    return fn


def remove_grad_ready_hook(fn):
    if fn in _grad_ready_hooks:
        _grad_ready_hooks.remove(fn)


def grad_buffer(p):
    """Persistent fp32 gradient buffer of parameter p (zeroed on first use); notes the current
    stream as a gradient producer."""
    g = p.grad
    if g is None:
        g = torch.empty_like(p, memory_format=torch.contiguous_format)
        ops.zero_(g)
        p.grad = g
    if g.is_cuda:
        st = _current_stream_obj(g)
        _grad_streams[id(st)] = st
        note_producer(p, st)
    return g


def _current_stream_obj(t):
    """The current stream of t's device as one cached torch Stream object
    (streams.current_stream; called for every parameter gradient of the step)."""
    return current_stream(t.get_device())


def note_producer(p, stream):
    """`stream` wrote p's gradient: this step's producer stream of p (MIXED: more than one), for
    FusedAdamW's early update of parameters whose gradients are final on a side stream."""
    prev = getattr(p, "_dfu_grad_stream", None)
    p._dfu_grad_stream = stream if prev is None or prev is stream else MIXED


def producer(p):
    """The stream that wrote p's gradient since the last clear_producers, None (nothing written)
    or MIXED."""
    return getattr(p, "_dfu_grad_stream", None)


def clear_producers(params):
    for p in params:
        p._dfu_grad_stream = None


def wants(p):
    return p is not None and p.requires_grad


def grad_or_none(p):
    return grad_buffer(p) if wants(p) else None


def grads_done(*params):
    if not _grad_ready_hooks:
        return
    hooks = tuple(_grad_ready_hooks)  # (a hook may be removed meanwhile: GC)
    for p in params:
        if p is not None:
            for h in hooks:
                h(p)


# Parameter gradients are written in place, possibly on a branch's side stream or the ViT
# weight-gradient stream, which autograd does not synchronise (it only orders the gradients it
# returns).  So that user code after loss.backward() -- torch.optim optimizers, clip_grad_norm_,
# manual reductions -- may read every p.grad on the stream that called backward, the first
# encoder-boundary backward of a graph task (arm_backward_join: the head side of TokenNormFn /
# AvgPoolFn / ConcatFn, which run on the forward's stream) queues an engine final callback that
# makes that stream wait for every gradient-producing stream once all backward nodes are
# enqueued.  Optimizers joined through join_grad_streams anyway (FusedAdamW, GradAllReducer)
# see no extra wait; any other torch.optim optimizer also joins in a step pre-hook.
_join_armed = [False]
_backward_end_hooks = []


def register_backward_end_hook(fn):
    """fn() is called when a backward pass through the HIP encoders has ended (the engine's
    final callback, after every node ran)."""
    _backward_end_hooks.append(fn)
    return fn


def remove_backward_end_hook(fn):
    if fn in _backward_end_hooks:
        _backward_end_hooks.remove(fn)


def arm_backward_join():
    if _join_armed[0] or not torch.cuda.is_available():
        return
    target = current_stream()
    _join_armed[0] = True

    def _join():
        _join_armed[0] = False
        streams.join_grad_streams(target, clear=False)
        for fn in list(_backward_end_hooks):
            fn()
    try:
        torch.autograd.Variable._execution_engine.queue_callback(_join)
    except RuntimeError:  # not inside a backward pass (a direct .backward() call of a Function)
        _join_armed[0] = False


def disarm_backward_join():
    """Forget an armed join whose backward pass a failed graph capture cut short."""
    _join_armed[0] = False


def join_armed():
    """Whether an end-of-backward join is queued and has not run yet."""
    return _join_armed[0]


def mark_self_joining(optimizer):
    """`optimizer`.step() joins the gradient streams itself: the global pre-hook leaves it be."""
    optimizer._dfu_joins_itself = True


def _optimizer_pre_hook(optimizer, args, kwargs):
    if _grad_streams and not getattr(optimizer, "_dfu_joins_itself", False):
        streams.join_grad_streams()


try:
    from torch.optim.optimizer import register_optimizer_step_pre_hook
    register_optimizer_step_pre_hook(_optimizer_pre_hook)
except ImportError:  # torch without global optimizer hooks
    pass
