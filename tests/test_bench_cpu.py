"""bench.py --gpus N without a launcher: it either starts N ranks
(torch.distributed.run, one child process) or fails -- it never times one process and reports
n_gpus = N."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env):
    env = dict(os.environ, DFU_DIST_BACKEND="gloo", **extra_env)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps",
                        "1", "--warmup", "0", "--no-cpu-baseline", "--no-parity"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, [json.loads(ln) for ln in lines]


def test_dump_outputs_is_bounded_typed_and_repeatable(tmp_path):
    """--dump-outputs: float32 files (float64 for 64-bit tensors), at most 64 MB in all, a long
    array cut to the same seeded sample of its elements on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    big = torch.arange(5_000_000, dtype=torch.float32)
    arrays = {"logits": torch.randn(64, 2).bfloat16(), "loss": torch.tensor(0.5),
              "pred": torch.arange(5), "params": big, "grads": -big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = 0
    for name, t in arrays.items():
        a, b = (np.load(tmp_path / d / f"{name}.npy") for d in ("a", "b"))
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.int64 else np.float32)
        assert np.array_equal(a, b)
        if t.numel() < 1_000_000:
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.float().numpy())
    assert total <= bench.DUMP_BYTES
    # the bound holds with every array long and 8 bytes an element, .npy headers included
    wide = {"a": torch.arange(5_000_000), "b": torch.arange(5_000_000).double()}
    bench.dump_outputs(str(tmp_path / "w"), wide)
    sizes = [os.path.getsize(tmp_path / "w" / f"{n}.npy") for n in wide]
    assert 60 << 20 < sum(sizes) <= bench.DUMP_BYTES
    assert all(np.load(tmp_path / "w" / f"{n}.npy").dtype == np.float64 for n in wide)
    p, g = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "a" / "grads.npy")
    assert 0 < p.size < big.numel() and np.array_equal(p, -g)  # the same elements of both
    assert np.all(np.diff(p) >= 0) and p.max() > big.numel() // 2  # drawn from the whole array


def test_gpus2_without_enough_devices_fails():
    import torch
    if torch.cuda.device_count() >= 2:
        return  # a real 2-GPU node: the launch path runs instead (driver's SCALE runs)
    p, lines = _run({})
    assert p.returncode == 2, p.stderr[-2000:]
    assert "needs 2 GPUs" in p.stderr
    assert not lines  # no line at all, least of all an n_gpus 2 one


def test_gpus2_rehearsal_launches_two_ranks():
    """DFU_SHARE_DEVICE=1 (the one-GPU gloo rehearsal): the parent launches 2 ranks; without a
    GPU they fail, and the failure is the exit status -- never a one-process line."""
    p, lines = _run({"DFU_SHARE_DEVICE": "1"})
    assert "[bench] launching 2 ranks" in p.stderr
    for ln in lines:  # (on a GPU box the ranks run: every line reports the 2 ranks it ran)
        assert ln["n_gpus"] == 2 and ln["config"]["dist"]["ranks"] == 2
    if not lines:
        assert p.returncode != 0
