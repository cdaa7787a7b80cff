"""The host-side stream helpers of the hot path (dfu_hip.streams, also known by ops.<name>):
dfu_stream_wait (a pooled event per join instead of a torch Event object), the cached
current-stream objects and the stream context without a Stream object per entry -- each against
torch's own behaviour -- and the stream state that module owns: the library's streams by role,
the per-stream caches and their reset (streams.forget)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_stream_wait_orders_a_consumer_after_a_producer():
    from dfu_hip import ops
    dev = torch.device("cuda", 0)
    prod, cons = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    n = 1 << 24
    x = torch.zeros(n, device=dev)
    out = []
    torch.cuda.synchronize()
    for it in range(300):  # more joins than the event ring holds (256): re-recorded events
        # both directions: the producer's next fill must also wait for the consumer's read
        ops.stream_wait(prod, cons)
        with torch.cuda.stream(prod):
            x.fill_(float(it))
            for _ in range(3):  # keep the producer busy so an unordered read would see old data
                x.mul_(1.0)
        ops.stream_wait(cons, prod)
        with ops.on_stream(cons):
            out.append(x[-1:].clone())
    ops.stream_wait(torch.cuda.current_stream(dev), cons)
    torch.cuda.synchronize()
    got = torch.cat(out).cpu()
    assert torch.equal(got, torch.arange(300, dtype=torch.float32))


def test_stream_wait_on_itself_is_a_no_op():
    from dfu_hip import ops
    s = torch.cuda.Stream()
    ops.stream_wait(s, s)
    torch.cuda.synchronize()


def test_on_stream_sets_and_restores_like_torch():
    from dfu_hip import ops
    dev = torch.device("cuda", 0)
    before = torch.cuda.current_stream(dev)
    s = torch.cuda.Stream(dev)
    with ops.on_stream(s) as got:
        assert got is s
        assert torch.cuda.current_stream(dev) == s
        assert ops.stream_ptr() == s.cuda_stream
        inner = torch.cuda.Stream(dev)
        with ops.on_stream(inner):
            assert torch.cuda.current_stream(dev) == inner
        assert torch.cuda.current_stream(dev) == s
    assert torch.cuda.current_stream(dev) == before
    with ops.on_stream(None):
        assert torch.cuda.current_stream(dev) == before
    # an exception inside restores the caller's stream too
    with pytest.raises(RuntimeError):
        with ops.on_stream(s):
            raise RuntimeError("x")
    assert torch.cuda.current_stream(dev) == before


def test_current_stream_is_cached_and_follows_the_context():
    from dfu_hip import ops
    dev = torch.device("cuda", 0)
    a = ops.current_stream()
    assert a is ops.current_stream(0)
    assert a == torch.cuda.current_stream(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        b = ops.current_stream()
        assert b == s and b.cuda_stream == s.cuda_stream
    assert ops.current_stream() is a


def test_library_streams_are_one_per_role():
    from dfu_hip import streams
    dev = torch.device("cuda", 0)
    side, wgrad = streams.side_stream(dev), streams.wgrad_stream(dev)
    cap = streams.capture_stream(0)
    assert streams.side_stream(dev) is side
    assert streams.wgrad_stream(dev) is wgrad
    assert streams.capture_stream(0) is cap
    assert len({side.cuda_stream, wgrad.cuda_stream, cap.cuda_stream}) == 3


def test_forget_evicts_a_retired_stream_from_every_cache():
    from dfu_hip import streams
    dev = torch.device("cuda", 0)
    side = streams.side_stream(dev)
    old = side.cuda_stream
    with streams.on_stream(side):
        streams.tile_counters(dev)
        assert streams.current_stream().cuda_stream == old
    objs, counters = streams.cached_handles()
    assert old in objs and old in counters
    assert old in [s.cuda_stream for s in streams.known_streams()]
    streams.forget({old})
    objs, counters = streams.cached_handles()
    assert old not in objs and old not in counters
    assert old not in [s.cuda_stream for s in streams.known_streams()]
    fresh = streams.side_stream(dev)
    assert fresh.cuda_stream != old  # the retired stream is leaked, so its address is not reused
    with streams.on_stream(fresh):
        cnt = streams.tile_counters(dev)
    torch.cuda.synchronize()
    assert cnt.numel() == streams.TILE_COUNTERS and int(cnt.abs().sum().item()) == 0


def test_known_streams_lists_a_stream_once():
    from dfu_hip import streams
    s = torch.cuda.Stream()
    handles = [k.cuda_stream for k in streams.known_streams(extra=[s, s])]
    assert handles.count(s.cuda_stream) == 1
    assert len(handles) == len(set(handles))
    assert handles[0] == torch.cuda.current_stream().cuda_stream
