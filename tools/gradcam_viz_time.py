"""Time the Grad-CAM visualisation pass for ten fusion samples (training.gradcam_viz.
visualize_batch: one forward, one generate_cams per encoder, the picture kernels, one host read)
against the reference script's shape, a per-sample loop of the same library calls at batch 1.
Both end in their host read, so a host clock around them includes the device work.  The two are
timed alternately; the pictures of both are compared first.  Prints one JSON line."""
import argparse
import json
import statistics
import time

import _harness  # noqa: F401
import numpy as np
import torch

from models.fusion import MultimodalFusionModel
from training import gradcam_viz as V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--iters", type=int, default=15)
    a = ap.parse_args()

    torch.manual_seed(0)
    model = MultimodalFusionModel().cuda()
    g = torch.Generator().manual_seed(1)
    rgb = torch.randn(a.samples, 3, 224, 224, generator=g).cuda()
    thermal = (torch.rand(a.samples, 3, 224, 224, generator=g) * 2 - 1).cuda()

    def one_pass():
        return V.visualize_batch(model, "multimodal", rgb=rgb, thermal=thermal)

    def per_sample():
        return [V.visualize_batch(model, "multimodal", rgb=rgb[i:i + 1], thermal=thermal[i:i + 1])
                for i in range(a.samples)]

    for _ in range(3):  # every shape of the timed window
        batch, singles = one_pass(), per_sample()
    # the model's own arithmetic depends on the batch size in the last bits (other GEMM tiles), so
    # the maps of the two are compared by their largest difference and the pictures by bytes
    same = {}
    for k in batch:
        stacked = np.stack([s[k][0] for s in singles])
        if k.startswith("cam"):
            same["max_abs_diff_" + k] = float(np.abs(batch[k] - stacked).max())
        elif k.startswith(("image", "heatmap", "overlay")):
            same["equal_bytes_" + k] = round(float((batch[k] == stacked).mean()), 5)
    times = {"one_pass": [], "per_sample": []}
    for _ in range(a.iters):
        for name, fn in (("one_pass", one_pass), ("per_sample", per_sample)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"samples": a.samples, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "batch_vs_per_sample": same}
    for name, t in times.items():
        out[name + "_ms"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2),
                             "max": round(max(t), 2)}
    out["ratio"] = round(out["per_sample_ms"]["median"] / out["one_pass_ms"]["median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
