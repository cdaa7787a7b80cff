"""Time the GPU input pipeline on a batch of decoded images: the whole GpuPreprocessor call (host
staging + one H2D copy + the two HIP kernels) on a host clock, and the reference's per-sample
PIL/torch transform on one host core for comparison.  --spec picks the train transform: rgb (the
default), thermal, thermal_only (the thermal one plus the GaussianBlur of
train_thermal_only.py; the host reference has no blur, so its figure is of the other ops), or
standardized (the rgb one after standardize_images.py's letterbox: dfu_letterbox_batch in place
of dfu_resize_batch; the host reference letterboxes with PIL first)."""
import argparse
import os
import sys
import time

import _harness
import numpy as np
import torch

from data import gpu_transforms as GT

SPECS = {"rgb": GT.rgb_train_transform, "thermal": GT.thermal_train_transform,
         "thermal_only": GT.thermal_only_train_transform,
         "standardized": GT.standardized(GT.rgb_train_transform)}


def _letterbox(im, target):
    """standardize_images.py's resize + paste on the host."""
    from PIL import Image
    ow, oh, px, py = GT.letterbox_dims(im.shape[1], im.shape[0], target)
    canvas = Image.new("RGB", (target, target), color=0)
    canvas.paste(Image.fromarray(im).resize((ow, oh), Image.BILINEAR), (px, py))
    return np.asarray(canvas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--spec", choices=sorted(SPECS), default="rgb")
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (a.h, a.w, 3), dtype=np.uint8) for _ in range(a.batch)]
    spec = SPECS[a.spec]
    g = torch.Generator().manual_seed(0)
    params = [GT.sample_params(spec, g) for _ in imgs]
    pre = GT.GpuPreprocessor(spec)
    for _ in range(3):
        pre(imgs, params)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        pre(imgs, params)
    torch.cuda.synchronize()
    full = (time.perf_counter() - t0) / a.iters
    what = "" if a.spec == "rgb" else f" [{a.spec}]"
    print(f"GpuPreprocessor{what} batch {a.batch} of {a.h}x{a.w}: {full * 1e3:.2f} ms/batch "
          f"({a.batch / full:.0f} img/s incl. host staging + H2D)")
    sys.path.insert(0, os.path.join(_harness.ROOT, "oracle"))
    import transforms_ref as TR
    t0 = time.perf_counter()
    n = min(8, a.batch)
    for im, p in zip(imgs[:n], params[:n]):
        if spec.standardize is not None:
            im = _letterbox(im, spec.standardize)
        TR.reference_transform(im, spec.size, spec.mean, spec.std, p.hflip, p.vflip, p.angle,
                               p.ops, p.affine)
    cpu = (time.perf_counter() - t0) / n
    print(f"PIL/torch reference transform: {cpu * 1e3:.2f} ms/img ({1 / cpu:.0f} img/s, 1 core)")


if __name__ == "__main__":
    main()
