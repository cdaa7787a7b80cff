"""Host side of train-mode dropout: the per-instance key (dfu_hip.nn.dropout_seed, hnn.Dropout's
seed and rng_offset) against the numpy restatement in dropout_ref.py, and a statistical
self-check of that restatement, which pins the oracle before test_dropout_gpu.py compares the
kernels with it.  No GPU.

Bounds: the keep count of n independent draws is binomial, so the keep fraction is bounded at 5
standard deviations, 5 sqrt(p (1 - p) / n) (2.6 were measured); two independent streams at
p = 0.7 agree where both keep or both drop, 0.3^2 + 0.7^2 = 0.58, with a standard deviation of
sqrt(0.58 * 0.42 / 65536) = 0.0019: 0.58 +- 0.01 is 5 of those."""
import itertools

import numpy as np
import pytest
import torch

import dropout_ref as R

N = 65536
BASES = (0, 1234, 2**63 + 12345, -7)


def test_seed_matches_restatement():
    from dfu_hip import nn as hnn
    for base in BASES + (2**64 - 1, 2**64 + 5, -2**63):
        for inst, rank in itertools.product((0, 1, 2, 3, 97, 2**31 + 1), (0, 1, 3, 7, 255)):
            got = hnn.dropout_seed(inst, rank=rank, base=base)
            assert 0 <= got < 2**64
            assert got == R.seed_of(inst, rank, base), (inst, rank, base)


def test_keys_pairwise_distinct():
    from dfu_hip import nn as hnn
    keys = [hnn.dropout_seed(i, rank=r, base=b)
            for i in range(4) for r in range(4) for b in BASES]
    assert len(keys) == 64 and len(set(keys)) == 64
    # instance and rank are not interchangeable: (1, 0) and (0, 1) are different streams
    assert hnn.dropout_seed(1, rank=0, base=1234) != hnn.dropout_seed(0, rank=1, base=1234)


def test_rank_follows_environment(monkeypatch):
    from dfu_hip import nn as hnn
    # no process group here (one left open by another test would outrank the variable)
    monkeypatch.setattr(hnn.dist, "is_initialized", lambda: False)
    monkeypatch.delenv("RANK", raising=False)
    assert hnn.dropout_seed(2, base=99) == R.seed_of(2, 0, 99)
    monkeypatch.setenv("RANK", "5")
    assert hnn.dropout_seed(2, base=99) == R.seed_of(2, 5, 99)
    assert hnn.dropout_seed(2, base=99) != R.seed_of(2, 0, 99)


def test_base_follows_manual_seed():
    from dfu_hip import nn as hnn
    old = torch.initial_seed()
    try:
        for s in (0, 777, 2**63 + 1):
            torch.manual_seed(s)
            assert hnn.dropout_seed(3, rank=1) == R.seed_of(3, 1, s)
    finally:
        torch.manual_seed(old)


def test_modules_get_their_own_stream(monkeypatch):
    """Two Dropouts built one after the other: consecutive instance indices under the current
    torch seed and rank, different keys, and an rng_offset buffer each, starting at 0."""
    from dfu_hip import nn as hnn
    monkeypatch.setattr(hnn.dist, "is_initialized", lambda: False)
    monkeypatch.delenv("RANK", raising=False)
    old = torch.initial_seed()
    try:
        torch.manual_seed(4321)
        i0 = next(hnn._dropout_instances)  # the creation counter: the next two follow it
        a, b = hnn.Dropout(0.7), hnn.Dropout(0.7)
    finally:
        torch.manual_seed(old)
    assert a.seed != b.seed
    assert a.seed == R.seed_of(i0 + 1, 0, 4321) and b.seed == R.seed_of(i0 + 2, 0, 4321)
    for m in (a, b):
        assert m.rng_offset.dtype == torch.int64 and m.rng_offset.shape == ()
        assert int(m.rng_offset) == 0
        assert "rng_offset" in dict(m.named_buffers()) and "rng_offset" not in m.state_dict()
    assert a.rng_offset.data_ptr() != b.rng_offset.data_ptr()
    a.rng_offset += 5
    assert int(b.rng_offset) == 0


def test_threshold_and_scale():
    assert R.threshold(0.0) == 0
    assert R.threshold(0.5) == 2**31
    assert R.threshold(np.float32(0.7)) == int(np.floor(float(np.float32(0.7)) * 2.0**32))
    assert R.threshold(np.nextafter(np.float32(1), np.float32(0))) == 2**32 - 256
    assert R.scale(0.0) == np.float32(1) and R.scale(0.5) == np.float32(2)
    assert R.scale(0.7).dtype == np.float32
    assert R.scale(np.nextafter(np.float32(1), np.float32(0))) == np.float32(2.0**24)


def test_restatement_against_python_integers():
    """The numpy uint64 arithmetic (wrapping adds and multiplies) against the same contract in
    Python's unbounded integers, at counters around the 32- and 64-bit boundaries."""
    def h(seed, ctr):
        z = (seed + 0x9E3779B97F4A7C15 * (ctr + 1)) & R.M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.M64
        return (z ^ (z >> 31)) >> 32
    for seed in (0, 1234, 2**63 + 12345, 2**64 - 1):
        for off in (0, 2**32 - 5, 2**40 + 3, 2**64 - 3):
            got = R.hash_u32(seed, off, 8)
            assert got.dtype == np.uint32
            assert [int(v) for v in got] == [h(seed, (off + i) & R.M64) for i in range(8)]


KEYS = (1234, R.seed_of(0, 0, 1234), R.seed_of(1, 0, 1234), R.seed_of(0, 1, 1234))


@pytest.mark.parametrize("p", [0.3, 0.5, 0.7])
def test_keep_fraction(p):
    bound = 5.0 * np.sqrt(p * (1.0 - p) / N)
    for key in KEYS:
        for off in (0, N, 2**40 + 3):
            k = R.keep(key, off, N, p)
            assert k.dtype == np.bool_ and k.shape == (N,)
            frac = k.mean()
            print(f"p={p} key={key:#x} off={off}: keep {frac:.5f}, "
                  f"{abs(frac - (1 - p)) / (bound / 5):.2f} sd")
            assert abs(frac - (1.0 - p)) <= bound, (p, key, off, frac)


def test_p_edges():
    assert R.keep(1234, 0, N, 0.0).all()
    top = np.nextafter(np.float32(1), np.float32(0))
    k = R.keep(1234, 0, 1 << 22, top)
    # keep probability 256 / 2^32 per element: ~0.25 expected in 2^22, never more than a few
    assert k.sum() <= 8


def test_streams_are_independent():
    p = 0.7
    base = R.keep(R.seed_of(0, 0, 1234), 0, N, p)
    others = {
        "instance 0 vs 1": R.keep(R.seed_of(1, 0, 1234), 0, N, p),
        "rank 0 vs 1": R.keep(R.seed_of(0, 1, 1234), 0, N, p),
        "offset 0 vs n": R.keep(R.seed_of(0, 0, 1234), N, N, p),
    }
    for what, k in others.items():
        agree = (base == k).mean()
        print(f"{what}: agreement {agree:.4f}")
        assert abs(agree - 0.58) <= 0.01, (what, agree)
    # continuity: the second half of one long call is the call that starts at offset n
    both = R.keep(R.seed_of(0, 0, 1234), 0, 2 * N, p)
    assert np.array_equal(both[:N], base) and np.array_equal(both[N:], others["offset 0 vs n"])
