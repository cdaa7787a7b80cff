"""Shared by test_gradcam_viz_cpu.py and test_gradcam_viz_gpu.py: a numpy restatement of the pixel
arithmetic that include/dfu_hip.h defines for dfu_image_minmax / dfu_cam_overlay and of the two
host tables (dfu_hip.ops.linear_taps, jet_lut).  Everything is fp32 with one rounding per
operation, in the kernel's operation order; the tables are written here a second time, element by
element, so that the library's vectorised forms are checked against something else."""
import math

import numpy as np

F32 = np.float32


def taps_ref(n_in, n_out):
    """OpenCV's INTER_LINEAR source coordinates, one output coordinate at a time (fp64)."""
    i0, i1, w = [], [], []
    for d in range(n_out):
        f = (d + 0.5) * (n_in / n_out) - 0.5
        lo = math.floor(f)
        wt = F32(f - lo)
        if wt == 1:  # f a rounding error below an integer: the next sample, weight 0
            lo, wt = lo + 1, F32(0)
        if lo < 0:
            lo, wt = 0, F32(0)
        if lo >= n_in - 1:
            lo, wt = n_in - 1, F32(0)
        i0.append(lo)
        i1.append(min(lo + 1, n_in - 1))
        w.append(wt)
    return np.array(i0, np.int32), np.array(i1, np.int32), np.array(w, F32)


def jet_ref():
    """255 * (1.5 - |4 i / 255 - c|) for c = 3, 2, 1, clamped, rounded half to even: in exact
    rationals (the value is (765 - 2 |4 i - 255 c|) / 2, always a half-integer)."""
    lut = np.zeros((256, 3), np.uint8)
    for i in range(256):
        for k, c in enumerate((3, 2, 1)):
            n = 765 - 2 * abs(4 * i - 255 * c)
            below = (n - 1) // 2  # n is odd: the value lies midway between below and below + 1
            lut[i, k] = min(max(below if below % 2 == 0 else below + 1, 0), 255)
    return lut


def minmax_ref(x):
    flat = np.asarray(x, F32).reshape(x.shape[0], -1)
    return np.stack([flat.min(1), flat.max(1)], 1)


def image_ref(x, minmax=None):
    """uint8 [B, H, W, 3] = trunc(((x - min) / (max - min)) * 255), zeros when max == min."""
    x = np.asarray(x, F32)
    mm = minmax_ref(x) if minmax is None else np.asarray(minmax, F32)
    out = np.zeros(x.shape, np.uint8)
    for b in range(x.shape[0]):
        mn, mx = mm[b]
        if mx != mn:
            v = (x[b] - mn) / F32(mx - mn)
            assert v.dtype == F32
            out[b] = (v * F32(255)).astype(np.uint8)
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1))


def resize_ref(cam, H, W):
    """fp32 [B, H, W]: the bilinear resample, horizontal pass first, every product and sum
    rounded to fp32."""
    cam = np.asarray(cam, F32)
    xi0, xi1, xw = taps_ref(cam.shape[2], W)
    yi0, yi1, yw = taps_ref(cam.shape[1], H)
    ux, uy = F32(1) - xw, F32(1) - yw
    t = cam[:, :, xi0] * ux + cam[:, :, xi1] * xw          # [B, h, W]
    v = t[:, yi0, :] * uy[None, :, None] + t[:, yi1, :] * yw[None, :, None]
    assert t.dtype == F32 and v.dtype == F32
    return v


def heatmap_ref(cam, H, W, lut=None):
    lut = jet_ref() if lut is None else np.asarray(lut, np.uint8)
    idx = (resize_ref(cam, H, W) * F32(255)).astype(np.uint8)
    return lut[idx]


def blend_ref(image, heatmap, alpha):
    """clamp(rint(image * (1 - alpha) + heatmap * alpha), 0, 255), rint to nearest even."""
    a = F32(alpha)
    b = F32(1) - a
    s = image.astype(F32) * b + heatmap.astype(F32) * a
    assert s.dtype == F32
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def overlay_ref(x, cam, alpha=0.5, lut=None, minmax=None):
    """(image, heatmap, overlay) as ops.cam_overlay returns them."""
    image = image_ref(x, minmax)
    heatmap = heatmap_ref(cam, x.shape[2], x.shape[3], lut)
    return image, heatmap, blend_ref(image, heatmap, alpha)


def overlay_on_image_ref(image_np, cam, alpha=0.5):
    """training.gradcam_viz.overlay_gradcam_on_image: the script's uint8 coercion (:445-449),
    then the heat map and the blend of the image as given."""
    if image_np.dtype != np.uint8:
        if image_np.max() <= 1.0:
            image_np = (image_np * 255).astype(np.uint8)
        else:
            image_np = image_np.astype(np.uint8)
    heatmap = heatmap_ref(np.asarray(cam, F32)[None], image_np.shape[0], image_np.shape[1])[0]
    return blend_ref(image_np, heatmap, alpha), heatmap
