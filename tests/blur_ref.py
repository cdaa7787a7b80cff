"""Reference for the GaussianBlur of the thermal-only train transform (dfu_augment_blur): the
pre-blur image from the PIL-backed oracle (oracle/transforms_ref.py), the blur in fp64 with the
kernel's own fp32 weights, and a comparison that accepts either neighbouring integer only where
the fp64 value lies within 2^-11 of a rounding tie.

The margin is derived, not measured: an fp32 evaluation of the nine products and eight adds
errs by at most (9 + 8) * 2^-24 * 255 ~ 2.6e-4 < 2^-11 whatever its summation order, so outside
the zone every correct fp32 evaluation rounds to round_half_even(v), and inside it torchvision's
own conv2d and a sequential sum may legitimately differ.  Helper module, no test."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import transforms_ref as TR  # noqa: E402

from data import gpu_transforms as GT  # noqa: E402

TIE_MARGIN = 2.0 ** -11
ZONE_CAP = 0.01  # at most 1 % of a case's values may lie in the tie zone


def img(h, w, seed):
    """tests/test_augment_gpu.py's _img."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(x / (5 + 3 * c) + c) * np.cos(y / (11 + c))
                  for c in range(3)], -1)
    return np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)


def _u8(t):
    """The uint8 image behind an un-normalised ToTensor output, exactly."""
    return torch.round(t * 255).to(torch.uint8)


def pre_blur(image, spec, p):
    """uint8 [3, H, W]: the image entering the blur, from the PIL oracle.  "rotate_flip" (the
    TTA Compose's order) is two oracle calls: resize + rotation, then flips + affine."""
    zero, one = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    rot = p.angle if spec.rotation else None
    if spec.order == "flip_rotate":
        return _u8(TR.reference_transform(image, spec.size, zero, one, p.hflip, p.vflip, rot,
                                          p.ops, p.affine))
    assert not p.ops
    first = _u8(TR.reference_transform(image, spec.size, zero, one, rotation=rot))
    return _u8(TR.reference_transform(first.permute(1, 2, 0).numpy(), spec.size, zero, one,
                                      p.hflip, p.vflip, None, (), p.affine))


def blur_f64(u8, sigma):
    """fp64 [3, H, W]: reflect pad by 1 and the 3 x 3 sum with the fp32 weights fp32(k[j] * k[i])
    converted to fp64."""
    k = torch.from_numpy(GT.blur_weights(sigma))
    assert k.dtype == torch.float32
    w2 = (k[:, None] * k[None, :]).double()
    x = torch.nn.functional.pad(u8.double()[None], (1, 1, 1, 1), mode="reflect")[0]
    H, W = u8.shape[1:]
    v = torch.zeros(u8.shape, dtype=torch.float64)
    for j in range(3):
        for i in range(3):
            v += w2[j, i] * x[:, j:j + H, i:i + W]
    return v


def normalise(u8, spec):
    """ToTensor + Normalize as the oracle does them, in fp32."""
    t = u8.float().div(255)
    return t.sub_(torch.as_tensor(spec.mean, dtype=torch.float32).view(-1, 1, 1)).div_(
        torch.as_tensor(spec.std, dtype=torch.float32).view(-1, 1, 1))


class Expected:
    """What a transform's output must be: `out` fp32 [3, H, W] must equal `lo` or `hi`, which
    differ only inside the tie zone."""

    def __init__(self, image, spec, p):
        self.pre = pre_blur(image, spec, p)
        if p.blur is None:
            lo = hi = self.pre
            self.zone = 0.0
        else:
            v = blur_f64(self.pre, p.blur)
            tie = ((v - torch.floor(v)) - 0.5).abs() <= TIE_MARGIN
            r = torch.round(v)  # half to even
            lo = torch.where(tie, torch.floor(v), r).to(torch.uint8)
            hi = torch.where(tie, torch.ceil(v), r).to(torch.uint8)
            self.zone = tie.double().mean().item()
        self.lo, self.hi = normalise(lo, spec), normalise(hi, spec)
        self.plain = normalise(self.pre, spec)  # the unblurred output

    def mismatches(self, out):
        return int(((out != self.lo) & (out != self.hi)).sum())


def check(out, image, spec, p, what=""):
    """Assert one output row against the reference; returns the Expected for further checks."""
    e = Expected(image, spec, p)
    assert e.zone <= ZONE_CAP, f"{what}: tie zone {e.zone:.4f} of the values (change the seed)"
    out = out.cpu()
    assert out.shape == e.lo.shape and out.dtype == torch.float32
    bad = e.mismatches(out)
    assert bad == 0, f"{what} {p}: {bad} values differ outside the tie zone " \
                     f"(zone {e.zone:.4f}, max {(out - e.lo).abs().max().item()})"
    return e
