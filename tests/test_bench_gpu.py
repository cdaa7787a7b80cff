"""bench.py end to end on the GPU: what a plain line and a --full line hold, and that
--dump-outputs writes the arrays of the step that was timed (small runs of the real command)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *argv],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_fusion_line_and_dump(tmp_path):
    """A plain run: the headline fields, nothing that takes a run of its own, and a dump whose
    loss is the weighted cross-entropy of its own logits on the run's seeded labels (class
    weights 2, 2: the plain mean), i.e. both come from the same step of the timed path."""
    import bench
    B = 8
    line = _bench("--steps", "2", "--warmup", "1", "--batch", str(B), "--dump-outputs",
                  str(tmp_path))
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "images/sec" and line["dtype"] and line["metric"]
    assert abs(line["value"] - B / (line["ms_per_step"] / 1e3)) <= 1e-3 * line["value"]
    for k in ("parity", "roofline", "cpu_baseline", "value_meets_parity_bar"):
        assert line[k] is None, k
    assert list(line["precision_modes"]) == [line["precision"]]
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["grads", "logits", "loss", "params"]
    for k, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
    assert got["logits"].shape == (B, 2) and got["loss"].shape == ()
    assert got["params"].shape == got["grads"].shape and got["params"].ndim == 1
    assert np.abs(got["grads"]).max() > 0 and np.abs(got["params"]).max() > 0
    _, _, y = bench.synthetic(B, DEV, seed=42)
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(got["logits"]).double(), y.cpu())
    # fp32 log-softmax and mean of 8 terms: a few ulp of the loss
    assert abs(ce.item() - float(got["loss"])) <= 1e-5 * max(1.0, abs(ce.item()))


def test_full_gradcam_line_and_dump(tmp_path):
    """--full fills the roofline (the CPU baseline switched off stays null), and the Grad-CAM dump
    -- written from the graph's buffers when the replay is the timed path -- is what a direct
    eager run of the same seeded model and batch computes.  The maps are min-max normalised to
    [0, 1]; replay and eager run the same kernels, and 1e-2 is the bar bench.py itself holds a
    replay to before timing it."""
    import bench
    from models.fusion import MultimodalFusionModel
    from models.gradcam import GradCAM
    B = 32
    line = _bench("--config", "gradcam", "--steps", "2", "--warmup", "1", "--full",
                  "--no-cpu-baseline", "--dump-outputs", str(tmp_path))
    print("hip_graph", line["config"]["hip_graph"], line["config"]["graph_vs_eager_ms"])
    assert line["full"] is True and line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None
    assert line["roofline"]["achieved"] > 0 and line["roofline"]["launches_per_step"] > 0
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["cam", "pred", "sal"]

    torch.manual_seed(42)  # as bench.main: rank 0
    model = MultimodalFusionModel(num_classes=2, dropout=0.7).to(DEV).eval()
    rgb, th, _ = bench.synthetic(B, DEV, seed=42)
    with torch.no_grad():
        pred = torch.softmax(model(rgb, th), dim=1).argmax(1)
    cam = GradCAM(model.resnet, ["layer4"]).generate_cams(rgb)
    sal = GradCAM(model.vit, ["blocks"]).generate_cams(th)
    torch.cuda.synchronize()
    assert got["pred"].dtype == np.float64 and got["pred"].shape == (B,)
    assert np.array_equal(got["pred"], pred.cpu().numpy().astype(np.float64))
    for name, want in (("cam", cam), ("sal", sal)):
        a, w = got[name], want.detach().float().cpu().numpy()
        assert a.dtype == np.float32 and a.shape == w.shape
        d = np.abs(a - w).max()
        print(name, "max |dump - direct|", d)
        assert d <= 1e-2, name
