"""The host-side stream and capture state of the library, and the one function that resets it.

Everything keyed by a HIP stream lives here: the raw-stream queries of the hot path, the record
of the streams a capture in progress launched on, the library-owned streams (one per role and
device), the per-stream caches (Stream objects, split-K tile counters) and the set of streams
that wrote parameter gradients.  dfu_hip.graphs recovers from a failed capture through `forget`
alone, so a cache added here is reset with the others.  Imports only torch and the loader:
ops, grads, functional, graphs, optim, parallel and models.fusion import from this module.
"""
import contextlib
import ctypes

import torch

from . import _lib as L
from ._lib import check

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


# ------------------------------------------------------------------------ capture recorder
# (device, raw stream) of every launch while dfu_hip.graphs.try_capture records a graph (None
# otherwise): the capture joins each of these streams that is still capturing into its origin
# before hipStreamEndCapture, so library work a step left on a stream it forked -- a plain torch
# stream included -- becomes part of the graph instead of failing the capture as unjoined.
_seen = None


@contextlib.contextmanager
def recording():
    """Record the stream of every library launch in the body (try_capture's capture and its
    recovery); "not recording" again afterwards, also when the body raises."""
    global _seen
    _seen = set()
    try:
        yield
    finally:
        _seen = None


def seen_streams():
    """The streams library launches went to during the capture being recorded (stream_ptr),
    as torch streams -- user streams the step forked onto included."""
    if not _seen:
        return []
    return [torch.cuda.ExternalStream(raw, device=torch.device("cuda", dev))
            for dev, raw in sorted(_seen)]


# ---------------------------------------------------------------------- raw-stream helpers
def stream_ptr():
    """The current HIP stream of the current device (the raw-pointer query: torch.cuda.
    current_stream() builds a Stream object per call, ~8 us of host time x ~260 calls a step).
    Pointers go to the C ABI as plain ints (ctypes converts them for c_void_p parameters:
    0.4 us per argument less than a c_void_p object, ~2000 arguments a step)."""
    if _raw_stream is not None and _cur_device is not None:
        dev = _cur_device()
        s = _raw_stream(dev)
    else:
        st = torch.cuda.current_stream()
        dev, s = st.device_index, st.cuda_stream
    if _seen is not None:
        _seen.add((dev, s))
    return s


_get_cur_stream = getattr(torch._C, "_cuda_getCurrentStream", None)
_set_cur_stream = getattr(torch._C, "_cuda_setStream", None)
_stream_objs = {}


def current_stream(idx=None):
    """torch.cuda.current_stream(idx) as one cached Stream object per (device, raw HIP stream):
    torch builds a new object per call (2.7 us of host time against 0.2 us,
    tools/host_breakdown.py).  An entry lives until `forget` evicts its handle."""
    if _raw_stream is None or _cur_device is None:
        return torch.cuda.current_stream(idx)
    if idx is None:
        idx = _cur_device()
    raw = _raw_stream(idx)
    st = _stream_objs.get((idx, raw))
    if st is None:
        st = _stream_objs[(idx, raw)] = torch.cuda.current_stream(idx)
    return st


class on_stream:
    """``with torch.cuda.stream(s):`` for a stream of the current device without the Stream
    object torch's context builds on entry (5.9 us of host time per entry against ~1 us,
    tools/host_breakdown.py); any other case goes through torch's own context."""

    __slots__ = ("s", "prev")

    def __init__(self, s):
        self.s = s
        self.prev = None

    def __enter__(self):
        s = self.s
        if s is None:
            return None
        if _get_cur_stream is None or _set_cur_stream is None or _cur_device is None or \
                s.device_index != _cur_device():
            self.prev = torch.cuda.stream(s)
            self.prev.__enter__()
            return s
        dev = s.device_index
        self.prev = _get_cur_stream(dev)
        _set_cur_stream(s.stream_id, dev, s.device_type)
        return s

    def __exit__(self, *exc):
        p, self.prev = self.prev, None
        if isinstance(p, tuple):
            _set_cur_stream(p[0], p[1], p[2])
        elif p is not None:
            p.__exit__(*exc)
        return False


def stream_wait(waiter, producer):
    """waiter.wait_stream(producer) for torch streams of the current device by one C call
    (dfu_stream_wait: a pooled event instead of a torch Event object per call, 6.5 us of host
    time against ~2 us); any other case goes through torch."""
    dev = waiter.device_index
    if producer.device_index != dev or _cur_device is None or dev != _cur_device():
        waiter.wait_stream(producer)
        return
    w = waiter.cuda_stream
    if _seen is not None:  # a fork into a capture: try_capture joins it at the end
        _seen.add((dev, w))
    check(L.load().dfu_stream_wait(w, producer.cuda_stream), "dfu_stream_wait")


def refuse_in_capture(what):
    """Raise DfuError while a graph is being recorded -- try_capture's recorder is active, or
    the current stream is capturing: `what` would either invalidate the capture (a stream
    creation is not a capturable call, from any stream, under the global capture mode) or leave
    state that only a replay initialises (a zero-fill recorded into the graph)."""
    if _seen is None:
        # (a process that has not initialised the GPU has no capture, and the query needs one)
        if not torch.cuda.is_initialized() or not torch.cuda.is_current_stream_capturing():
            return
    elif torch.cuda.is_initialized():
        stream_ptr()  # a fork with no library launch yet: join_forked must still see it
    raise L.DfuError(f"{what} requested inside a HIP-graph capture: run the step once "
                     f"eagerly on the same streams before capturing it")


# ------------------------------------------------------------------- library-owned streams
# (role, device index) -> stream.
# Every library stream runs at the default HIP priority: a high-priority ViT side stream gained
# 0.3% in the eager fusion step, but a C5 Grad-CAM step whose warm-up ran with it replayed from
# a HIP graph at 49.6-54.4 ms against 22.9 ms (round 3).
_library_streams = {}


def new_stream(idx, priority=0):
    """A library-owned non-blocking HIP stream (dfu_stream_create) as a torch ExternalStream.
    Never returned to torch's stream pool: a stream a failed graph capture left capturing is
    retired (`forget`) and this makes a fresh one."""
    # hipStreamCreate is not a capturable call: under a global-mode capture it invalidates the
    # capture of every stream forked into it, so every such request is refused
    refuse_in_capture("a new library stream")
    h = ctypes.c_void_p(0)
    with torch.cuda.device(idx):
        check(L.load().dfu_stream_create(int(priority), ctypes.byref(h)), "dfu_stream_create")
    return torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))


def _library_stream(role, device):
    idx = device if isinstance(device, int) else torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    st = _library_streams.get((role, idx))
    if st is None:
        st = _library_streams[(role, idx)] = new_stream(idx)
    return st


def side_stream(device):
    """One persistent side stream per device for the concurrent encoder branch."""
    return _library_stream("side", device)


def wgrad_stream(device):
    """One persistent stream per device for the ViT blocks' weight-gradient GEMMs: they depend
    only on tensors already produced and feed only the optimizer, so they run beside the input-
    gradient chain, whose N = 768 GEMMs fill 150 of the 256 CUs (12608 / 256 x 768 / 256 tiles)
    and whose LayerNorm / attention kernels leave the MFMAs idle."""
    return _library_stream("wgrad", device)


def capture_stream(idx):
    """One capture stream per device, reused by every capture (a graph does not need its
    origin stream after the capture ends); retired, never reused, if a failure leaves it
    capturing."""
    return _library_stream("capture", idx)


# --------------------------------------------------------------------- split-K tile counters
_COUNTERS = {}
_COUNTER_POOLS = {}  # device index -> [zeroed pool, next free slot]
TILE_COUNTERS = 1 << 16
COUNTER_SLOTS = 64  # streams per pool (64 x 256 KiB)


def tile_counters(device):
    """Per-stream zeroed int32 tile counters for the in-kernel split-K reduction (every launch
    returns them zeroed; launches on one stream never overlap).  A stream's counters are a slot
    of a per-device pool zeroed when the pool is made, so a stream first seen inside a graph
    capture takes a slot by host bookkeeping alone (a zero-fill made inside the capture would be
    recorded into the graph and run only at its replays: eager launches on that stream before
    the first replay would read uninitialised counters)."""
    idx = device.index if isinstance(device, torch.device) and device.index is not None else None
    if _raw_stream is not None and idx is not None:
        key = (idx, _raw_stream(idx))  # the raw query: ~0.3 us against ~5 us for a Stream object
        t = _COUNTERS.get(key)
        if t is not None:
            return t
    st = torch.cuda.current_stream(device)
    key = (st.device_index, st.cuda_stream)
    t = _COUNTERS.get(key)
    if t is None:
        pool = _COUNTER_POOLS.get(st.device_index)
        if pool is None or pool[1] == COUNTER_SLOTS:
            refuse_in_capture(f"a fresh pool of split-K tile counters (stream "
                              f"{st.cuda_stream:#x})")
            pool = _COUNTER_POOLS[st.device_index] = [
                torch.zeros(COUNTER_SLOTS * TILE_COUNTERS, dtype=torch.int32, device=device), 0]
        i = pool[1]
        pool[1] += 1
        t = _COUNTERS[key] = pool[0][i * TILE_COUNTERS:(i + 1) * TILE_COUNTERS]
    return t


# ------------------------------------------------------------------------ gradient producers
# Streams that wrote persistent parameter gradients since the last join.  Autograd synchronises
# only the gradients it returns; these buffers are written in place (possibly on a branch's side
# stream, see models.fusion), so consumers (FusedAdamW.step, GradAllReducer.finish) join first.
# grads.grad_buffer stores into this dict directly (one dict store per gradient).
grad_streams = {}


def join_grad_streams(stream=None, clear=True):
    """Make `stream` (default: the current stream) wait for every stream that wrote parameter
    gradients since the last clearing join."""
    if not grad_streams:
        return
    cur = stream if stream is not None else current_stream()
    for st in grad_streams.values():
        if st != cur:
            stream_wait(cur, st)
    if clear:
        grad_streams.clear()


# ----------------------------------------------------------------------- the state as a whole
def known_streams(device=None, extra=()):
    """Every stream a DFU step may enqueue on, once each: the current one, the library-owned
    streams, `extra`, and the streams library launches went to during the capture in
    progress."""
    out = [torch.cuda.current_stream(device)]
    out += list(_library_streams.values()) + list(extra) + seen_streams()
    seen, uniq = set(), []
    for s in out:
        if s.cuda_stream not in seen:
            seen.add(s.cuda_stream)
            uniq.append(s)
    return uniq


def cached_handles():
    """The raw handles the per-stream caches hold: (Stream objects, tile counters)."""
    return {raw for _, raw in _stream_objs}, {raw for _, raw in _COUNTERS}


def forget(raw_handles):
    """The host-state reset after a failed capture: drop everything that refers to the streams
    `raw_handles` (those HIP left capturing for good) and the gradient-producer set."""
    for k in [k for k, s in _library_streams.items() if s.cuda_stream in raw_handles]:
        del _library_streams[k]  # leaked on purpose: it cannot be destroyed or reused
    # a retired stream's counter slot stays taken (256 KiB of its pool): only the entry goes, so
    # a later stream at the same address takes a slot no kernel of the old one can still touch
    for cache in (_stream_objs, _COUNTERS):
        for k in [k for k in cache if k[1] in raw_handles]:
            del cache[k]
    grad_streams.clear()
