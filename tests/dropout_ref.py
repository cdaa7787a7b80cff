"""Host restatement of the train-mode dropout mask stream (csrc/elem.hip: hash_u32,
k_dropout_fwd) and of the per-instance key (dfu_hip.nn.dropout_seed), in numpy uint64 arithmetic
written from the documented contract, not from the library's own Python:

    z    = seed + 0x9E3779B97F4A7C15 * (offset + i + 1)          (mod 2^64)
    z    = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB
    keep = (z ^ z >> 31) >> 32  >=  floor(float32(p) * 2^32)
    y    = keep ? x * (float32(1) / (float32(1) - float32(p))) : +0

The mask is a pure function of (seed, offset + i, p), so this is an exact oracle: the tests
compare masks bit for bit (tests/test_dropout_cpu.py pins the restatement's own statistics)."""
import numpy as np

M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_MUL1 = 0xBF58476D1CE4E5B9
_MUL2 = 0x94D049BB133111EB


def _u64(v):
    """Python int (any sign or size) -> 1-element uint64 array of its low 64 bits."""
    return np.array([int(v) & M64], dtype=np.uint64)


def _finalise(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_MUL2)
    return z ^ (z >> np.uint64(31))


def _splitmix64(z):
    """One splitmix64 step of a uint64 array: add the golden increment, then finalise."""
    with np.errstate(over="ignore"):
        return _finalise(z + np.uint64(_GOLDEN))


def hash_u32(seed, offset, n):
    """uint32 array: the kernel's hash of counters offset .. offset + n - 1 under `seed`."""
    with np.errstate(over="ignore"):
        ctr = np.arange(n, dtype=np.uint64) + _u64(offset)
        z = _u64(seed) + np.uint64(_GOLDEN) * (ctr + np.uint64(1))
    return (_finalise(z) >> np.uint64(32)).astype(np.uint32)


def threshold(p):
    """floor(float32(p) * 2^32): a power-of-two scaling, exact in float32."""
    return int(np.float32(p) * np.float32(4294967296.0))


def keep(seed, offset, n, p):
    """bool array of length n: element i of a call that starts at counter `offset` is kept."""
    return hash_u32(seed, offset, n).astype(np.uint64) >= np.uint64(threshold(p))


def scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def seed_of(instance, rank, base):
    """splitmix64(splitmix64(splitmix64(base) ^ instance) ^ rank), as dropout_seed documents."""
    z = _splitmix64(_u64(base))
    z = _splitmix64(z ^ _u64(instance))
    z = _splitmix64(z ^ _u64(rank))
    return int(z[0])


def apply_f32(x, k, p):
    """numpy float32 reference of y = where(keep, x * scale, +0)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(k, x.astype(np.float32) * scale(p), np.float32(0)).astype(np.float32)


def apply_torch(x, k, p):
    """torch CPU reference for fp32 or bf16 x: (x.float() * scale) rounded to x.dtype (round to
    nearest even), dropped positions +0."""
    import torch
    y = (x.float() * float(scale(p))).to(x.dtype)
    return torch.where(torch.from_numpy(np.ascontiguousarray(k)).view(x.shape), y,
                       torch.zeros((), dtype=x.dtype))
