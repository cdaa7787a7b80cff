"""Aspect-preserving standardisation on the GPU (dfu_letterbox_batch: k_letterbox_h, k_letterbox_v
in csrc/augment.hip, through GT.GpuPreprocessor with TransformSpec.standardize and through
data.standardize) against PIL itself (tests/standardize_ref.py: resize, black canvas, paste, then
the PIL-backed oracle): 0 differing values.  Source sizes cover both orientations, the 223 quirk,
a 1 x 1 source, sources at the target size one way, up- and downscales and a large photograph."""
import numpy as np
import pytest
import torch
from PIL import Image

import blur_ref as BR
import standardize_ref as SR
from data import gpu_transforms as GT
from data import standardize as SZ

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 224


def _imgs(seed):
    return [SR.img(h, w, seed + i) for i, (h, w) in enumerate(SR.SIZES)]


def _run(spec, imgs, params=None, views=None):
    out = GT.GpuPreprocessor(spec)(imgs, params, views)
    assert out.is_cuda and out.dtype == torch.float32
    assert out.shape == (len(imgs) * (views or 1), 3, T, T)
    return out.cpu()


def _check(out, imgs, spec, params):
    for i, (im, p) in enumerate(zip(imgs, params)):
        ref = SR.transform(im, spec, p)
        bad = (out[i] != ref).sum().item()
        assert bad == 0, f"image {i} {im.shape} {p}: {bad} values differ, " \
                         f"max {(out[i] - ref).abs().max().item()}"


def _normalised(u8_hwc, spec):
    t = torch.from_numpy(np.array(u8_hwc, np.uint8, copy=True))
    return BR.normalise(t.permute(2, 0, 1), spec)


@pytest.mark.parametrize("name", ["rgb", "thermal"])
def test_eval_transform_bitwise(name):
    spec = GT.standardized(GT.rgb_val_test_transform if name == "rgb"
                           else GT.thermal_val_test_transform)
    imgs = _imgs(0)
    out = _run(spec, imgs)
    _check(out, imgs, spec, [GT.AugParams() for _ in imgs])
    black = _normalised(np.zeros((1, 1, 3), np.uint8), spec)  # the normalised value of 0
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        ow, oh, px, py = SR.dims(w, h, T)
        border = torch.ones(T, T, dtype=torch.bool)
        border[py:py + oh, px:px + ow] = False
        assert border.sum().item() == T * T - ow * oh
        assert (out[i][:, border] == black[:, 0, 0, None]).all(), f"image {i}: border"
        # the box by PIL's resize alone (no canvas, no paste), found at (pad_y, pad_x)
        box = _normalised(np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR)), spec)
        assert torch.equal(out[i][:, py:py + oh, px:px + ow], box), f"image {i}: box"
        assert not (box[:, 0, 0] == black[:, 0, 0]).all(), "the corner pixel should not be black"


def test_train_transform_sampled_params_bitwise():
    """The augment stage reads the canvas: rotation and affine move the black border."""
    spec = GT.standardized(GT.rgb_train_transform)
    g = torch.Generator().manual_seed(11)
    imgs = _imgs(50)
    params = [GT.sample_params(spec, g) for _ in imgs]
    assert any(p.affine for p in params) and any(p.ops for p in params)
    _check(_run(spec, imgs, params), imgs, spec, params)


def test_views_on_the_canvas():
    """views = 3 in the TTA Compose's order: one letterbox per image, three gathers from it."""
    K = 3
    spec = GT.standardized(GT.thermal_tta_transform)
    g = torch.Generator().manual_seed(5)
    imgs = _imgs(100)
    params = [GT.sample_params(spec, g) for _ in range(len(imgs) * K)]
    out = _run(spec, imgs, params, views=K)
    for v, p in enumerate(params):
        e = BR.check(out[v], SR.canvas(imgs[v // K]), spec, p, f"view {v}")
        assert e.zone == 0.0  # no blur: lo == hi, exact


def test_blur_on_the_canvas():
    """The thermal-only train transform: the blur reference on the standardised image, with the
    tie allowance of tests/blur_ref.py (test_blur_gpu.py's) and no other."""
    spec = GT.standardized(GT.thermal_only_train_transform)
    g = torch.Generator().manual_seed(7)
    imgs = _imgs(150)
    params = [GT.sample_params(spec, g) for _ in imgs]
    assert 0 < sum(p.blur is not None for p in params) < len(params)
    out = _run(spec, imgs, params)
    for i, p in enumerate(params):
        BR.check(out[i], SR.canvas(imgs[i]), spec, p, f"image {i}")


def test_isolation_and_every_byte_written():
    """dfu_letterbox_batch into a canvas buffer pre-filled with 0xAA.  The sources hold no value
    above 160 and the taps are non-negative, so no correct output byte is 0xAA (170): one left
    in the buffer was not written.  Each image's canvas equals its canvas when run alone."""
    sizes = [(96, 64), (60, 90), (55, 55)]  # portrait, landscape, the 223 case
    imgs = [np.minimum(SR.img(h, w, 200 + i), 160) for i, (h, w) in enumerate(sizes)]
    pre = GT.GpuPreprocessor(GT.standardized(GT.rgb_val_test_transform))
    buf = torch.full((len(imgs) + 2, T, T, 3), 0xAA, dtype=torch.uint8, device=DEV)
    out = pre.resize(pre.stage(imgs), out=buf[1:-1])
    assert out.data_ptr() == buf[1].data_ptr()
    torch.cuda.synchronize()
    assert (buf[0] == 0xAA).all() and (buf[-1] == 0xAA).all()  # nothing outside the output
    assert not (out == 0xAA).any()
    out = out.cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(out[i], SR.canvas(im)), i
        alone = torch.full((1, T, T, 3), 0x55, dtype=torch.uint8, device=DEV)
        pre.resize(pre.stage([im]), out=alone)
        assert np.array_equal(alone[0].cpu().numpy(), out[i]), i
    assert (out[2][:, 223] == 0).all() and (out[2][223] == 0).all()  # the one-pixel strips
    assert (out[2][:223, :223].reshape(-1, 3).max(1) > 0).all()


def test_refused_image_raises_before_the_device_is_used():
    spec = GT.standardized(GT.rgb_val_test_transform)
    pre = GT.GpuPreprocessor(spec)
    imgs = [SR.img(48, 64, 300), SR.img(1000, 5, 301), SR.img(64, 48, 302)]
    with pytest.raises(NotImplementedError, match="image 1 of the batch"):
        pre.stage(imgs)  # the host half: no copy, no launch
    good = [imgs[0], imgs[2]]
    _check(pre(good).cpu(), good, spec, [GT.AugParams()] * 2)


def test_offline_tool_writes_the_scripts_files(tmp_path):
    """standardize_tree's files against the helper's canvas saved the same way, byte for byte."""
    src, dst, ref = tmp_path / "raw", tmp_path / "std", tmp_path / "ref"
    files = [("a.png", (48, 64), "RGB"), ("healthy/b.jpg", (64, 48), "RGB"),
             ("healthy/deep/c.JPEG", (55, 55), "RGB"), ("ulcer/d.png", (40, 70), "L"),
             ("ulcer/e.Png", (224, 224), "RGB"), ("ulcer/f.jpg", (100, 30), "RGB")]
    for k, (name, (h, w), mode) in enumerate(files):
        (src / name).parent.mkdir(parents=True, exist_ok=True)
        im = Image.fromarray(SR.img(h, w, 400 + k))
        (im.convert("L") if mode == "L" else im).save(src / name, quality=90)
    (src / "ulcer" / "broken.png").write_bytes(b"\x89PNG no image")
    assert SZ.standardize_tree(src, dst, batch_size=4) == (len(files), 1)
    assert sorted(p.relative_to(dst).as_posix() for p in dst.rglob("*") if p.is_file()) == \
        sorted(name for name, _, _ in files)
    for name, _, mode in files:
        with Image.open(src / name) as im:
            assert im.mode == mode
            decoded = np.asarray(im.convert("RGB"))
        (ref / name).parent.mkdir(parents=True, exist_ok=True)
        SR.canvas_image(decoded).save(ref / name, quality=95)
        assert (dst / name).read_bytes() == (ref / name).read_bytes(), name
    assert SZ.verify_standardization(dst) == (True, {(T, T): len(files)})
