"""tools/kernel_time.py on the GPU: every case runs against today's dfu_hip.ops signatures."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what starts each case's result lines (the former per-kernel scripts' wording)
RESULT = {"adamw": "adamw_flat n=", "attn": "attention fwd ", "bn_apply": "bn_apply M=",
          "bn_apply_x3": "M=", "bn_bwd": "bn_bwd M=", "colsum": "colsum rows=",
          "ln_fwd": "ln_fwd rows=", "ln_bwd": "ln_bwd rows=", "pool": "maxpool bwd ",
          "stem": "fused stem kernel", "t1x1": "6272x64x", "dgrad_strided": "dgrad s2 ",
          "epi": "product BF16 "}


@pytest.mark.gpu
def test_kernel_time_runs_every_case_at_batch_2():
    """B = 2 keeps the geometries the kernels require (the stem's 2 x 112 x 112 rows are a
    multiple of 128) and finishes in seconds after torch's import."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_time.py"), "--all",
                        "--batch", "2", "--iters", "2"], capture_output=True, text=True,
                       timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    case, lines = None, {}
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            case = line[3:]
        elif case:
            lines.setdefault(case, []).append(line)
    assert list(lines) == list(RESULT)
    for case, start in RESULT.items():
        hits = [ln for ln in lines[case] if ln.startswith(start)]
        assert hits, (case, lines[case])
        for ln in hits:
            # "<time> us", or dgrad_strided's "t<tile> <time>" columns
            times = [float(a or b) for a, b in re.findall(r"(\d+\.\d+) ?us|t\d+ +(\d+\.\d+)", ln)]
            assert times and all(t > 0 for t in times), ln
