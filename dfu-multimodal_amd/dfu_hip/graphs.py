"""HIP-graph capture of a step with a clean fallback to eager execution.

A captured step replays every kernel launch of the step from one graph launch (the host-side
enqueue cost of the ~700 launches disappears).  Capture can fail -- work forked onto a side
stream and not joined back, a host synchronisation inside the step -- and a failed capture can
leave the streams it forked into still in capture mode, so that the next eager launch or event
on them fails as well (bench.py round 2: "event last recorded in a capturing stream": the
timing event went to torch.cuda.graph's capture stream, which its __exit__ leaves current when
capture_end raises).
try_capture ends such leftover captures (dfu_streams_abort_capture over every stream the step
can touch), drops the host state that refers to them (streams.forget), and reports the failure,
so the caller runs eager.  The stream state itself -- which streams exist, which a capture has
seen, what is cached per stream -- belongs to dfu_hip.streams; this module is capture logic only.
"""
import ctypes
import sys

import torch

from . import _lib as L
from . import grads
from . import streams


def capture_status(stream):
    """0 none, 1 active, 2 invalidated (dfu_stream_capture_status)."""
    st = ctypes.c_int32(0)
    L.check(L.load().dfu_stream_capture_status(ctypes.c_void_p(stream.cuda_stream),
                                               ctypes.byref(st)), "dfu_stream_capture_status")
    return st.value


def join_forked(origin, extra=()):
    """Inside a capture on `origin`: make it wait for every step stream that is capturing (a
    fork of this capture), so work left on a side stream joins the graph instead of failing
    the capture as unjoined -- which HIP cannot undo: the origin's hipStreamEndCapture then
    returns hipErrorStreamCaptureUnjoined and leaves the origin and its forks capturing for
    good (a second end returns hipErrorStreamCaptureWrongThread).  The step streams
    include every stream a library launch went to during this capture, so a fork onto a plain
    torch stream that the step did not join back (the C5 split-graph
    attempt's crash at hipStreamEndCapture) is joined here too; only non-library work on a
    stream the library never saw can still leave a fork unjoined."""
    for s in streams.known_streams(extra=extra):
        if s.cuda_stream != origin.cuda_stream and capture_status(s) == 1:
            origin.wait_stream(s)


def abort_captures(known):
    """End any capture left active on the streams `known` (dfu_streams_abort_capture); returns
    (streams that were capturing, streams still capturing afterwards)."""
    lib = L.load()
    handles = [s.cuda_stream for s in known]
    before = 0
    for s in known:
        with torch.cuda.stream(s):
            before += int(torch.cuda.is_current_stream_capturing())
    arr = (ctypes.c_void_p * len(handles))(*handles)
    left = ctypes.c_int32(0)
    L.check(lib.dfu_streams_abort_capture(arr, len(handles), ctypes.byref(left)),
            "dfu_streams_abort_capture")
    return before, left.value


def reset_after_failed_capture(extra=()):
    """Recover after a failed capture: end what HIP lets us end, retire the library-owned
    streams still capturing (HIP cannot end a capture whose origin's end already failed: the
    origin and its forks keep reporting an active capture, see join_forked) -- the next
    side_stream / wgrad_stream / capture_stream call makes fresh ones -- and reset the host-side stream state (streams.forget).  Returns (streams
    that were capturing, streams retired)."""
    known = streams.known_streams(extra=extra)
    n, _ = abort_captures(known)
    stuck = {s.cuda_stream for s in known if capture_status(s) != 0}
    streams.forget(stuck)
    cur = torch.cuda.current_stream()
    if cur.cuda_stream in stuck:
        raise RuntimeError("dfu: the caller's stream is still capturing after a failed capture")
    grads.disarm_backward_join()
    try:  # can the process run eager work again?  (an allocation + a kernel + a host sync)
        torch.empty(1024, device=cur.device).fill_(0.0)
        torch.cuda.synchronize()
    except RuntimeError as e:
        # HIP leaves an INVALIDATED capture that had forked streams active for good (e.g. a host
        # synchronisation inside the step): every later legacy-stream or allocation call fails
        # with hipErrorStreamCaptureImplicit.  Nothing in-process can end it.
        raise RuntimeError("dfu: a failed HIP-graph capture left this process unable to run "
                           "eager work (HIP cannot end an invalidated capture with forked "
                           "streams); rerun without graph capture") from e
    return n, len(stuck)


def try_capture(step, log=None, pool=None):
    """Capture `step()` into a torch.cuda.CUDAGraph on a fresh capture stream; returns the graph,
    or None after a failed capture (streams recovered, the failure reported through `log`,
    default stderr).  Work the step left on a forked stream is joined into the capture
    (join_forked).  The caller warms `step` up eagerly first, as graph capture requires."""
    prev = torch.cuda.current_stream()
    cap = streams.capture_stream(prev.device_index)
    cap.wait_stream(prev)
    # the capture stream's split-K tile counters exist before the capture: created inside it,
    # their zero-fill would be recorded into this graph and run only at its replays (and once
    # the recorder is on, creating a stream or a counter pool is refused)
    with torch.cuda.stream(cap):
        streams.tile_counters(cap.device)
    g = torch.cuda.CUDAGraph()
    with streams.recording():  # through the recovery too, which aborts what the capture saw
        try:
            with torch.cuda.graph(g, pool=pool, stream=cap):
                try:
                    step()
                finally:
                    # also when step() raised (a DfuError refusing a non-capturable call):
                    # joined forks let torch.cuda.graph's hipStreamEndCapture succeed, so the
                    # failure is a Python exception and the streams are clean for the eager
                    # fallback
                    join_forked(cap)
            return g
        except Exception as e:  # noqa: BLE001 -- any capture failure falls back to eager
            # torch.cuda.graph.__exit__ leaves its capture stream current when capture_end raises
            torch.cuda.set_stream(prev)
            n, stuck = reset_after_failed_capture(extra=(cap,))
            msg = (f"[dfu] graph capture failed ({type(e).__name__}: {str(e).splitlines()[0]}); "
                   f"{n} stream(s) were left capturing, {stuck} retired; running eager")
            if log is None:
                print(msg, file=sys.stderr)
            elif log:
                log(msg)
            del g
            return None
