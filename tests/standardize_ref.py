"""Reference for the aspect-preserving standardisation (dfu_letterbox_batch;
TransformSpec.standardize) by PIL itself, written from the behaviour of the reference's
scripts/standardize_images.py: resize so that the longest edge is T (bilinear, the sizes by the
script's float expressions), a new black T x T canvas, paste at the centred offset; then the
PIL-backed oracle (oracle/transforms_ref.reference_transform) on the canvas, which skips its
resize at equal size.  Helper module, no test."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import transforms_ref as TR  # noqa: E402

# (h, w) of the GPU tests: square, both orientations, the 223 quirk (55, and 55 x 40), the
# smallest image, a short side that is no integer, a long thin one, large sources, sources at
# the target size one way, an exact half
SIZES = [(224, 224), (480, 640), (640, 480), (55, 55), (55, 40), (1, 1), (200, 300), (389, 97),
         (2000, 3000), (224, 100), (100, 224), (71, 142)]


def img(h, w, seed):
    """tests/test_augment_gpu.py's _img."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(x / (5 + 3 * c) + c) * np.cos(y / (11 + c))
                  for c in range(3)], -1)
    return np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)


def dims(w, h, target):
    """(out_w, out_h, pad_x, pad_y) as the script computes them."""
    scale = target / max(w, h)
    new_w, new_h = int(w * scale), int(h * scale)
    return new_w, new_h, (target - new_w) // 2, (target - new_h) // 2


def canvas_image(image, target=224):
    """The script's standardised PIL image of an H x W x 3 uint8 array."""
    im = Image.fromarray(np.ascontiguousarray(image, np.uint8))
    assert im.mode == "RGB"
    new_w, new_h, pad_x, pad_y = dims(im.size[0], im.size[1], target)
    out = Image.new("RGB", (target, target), color=0)
    out.paste(im.resize((new_w, new_h), Image.BILINEAR), (pad_x, pad_y))
    return out


def canvas(image, target=224):
    """uint8 [T, T, 3]."""
    return np.array(canvas_image(image, target), np.uint8, copy=True)


def transform(image, spec, p):
    """fp32 [3, T, T]: the oracle on the standardised image, for one sample's parameters."""
    T = spec.standardize
    assert tuple(spec.size) == (T, T)
    return TR.reference_transform(canvas(image, T), spec.size, spec.mean, spec.std, p.hflip,
                                  p.vflip, p.angle if spec.rotation else None, p.ops, p.affine)
