"""The Grad-CAM visualisation pass on the GPU (notebooks/grad_cam_visualization.py:432-859):
  * dfu_image_minmax (ops.image_minmax) against numpy;
  * dfu_cam_overlay (ops.cam_overlay) bit for bit against the numpy restatement of its definition
    (gradcam_viz_ref.py), into poisoned buffers with guards, and its argument checks;
  * training.gradcam_viz: overlay_gradcam_on_image, visualize_batch with a model of each kind,
    run_gradcam_visualization on a synthetic tree.
Agreement with cv2 itself is not tested (OpenCV is not available to this project)."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import data_inputs as DI  # noqa: E402

import gradcam_viz_ref as VR  # noqa: E402
from dfu_hip import ops  # noqa: E402
from training import gradcam_viz as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
POISON = 0xA5
PICTURES = ("image", "heatmap", "overlay")
KINDS = V.KINDS


# ------------------------------------------------------------------------------ image_minmax
def _minmax(x):
    got = ops.image_minmax(torch.from_numpy(x).to(DEV))
    assert got.shape == (x.shape[0], 2) and got.dtype == torch.float32 and got.is_cuda
    return got.cpu().numpy()


@pytest.mark.parametrize("B,n", [(1, 1), (3, 255), (2, 3 * 37 * 29), (10, 3 * 224 * 224)])
def test_image_minmax_against_numpy(B, n):
    rng = np.random.default_rng(B * 1000 + n)
    x = (rng.normal(size=(B, n)) * rng.uniform(0.5, 3, (B, 1)) +
         rng.uniform(-2, 2, (B, 1))).astype(np.float32)
    assert np.array_equal(_minmax(x), VR.minmax_ref(x))
    # the extremes at the first and the last element, and on either side of every boundary
    # between two blocks' parts of an image (4096 elements each)
    spots = sorted({0, n - 1} | {p for k in range(4096, n, 4096) for p in (k - 1, k)})
    for lo, hi in zip(spots, spots[::-1]):
        if lo == hi:
            continue
        y = x.copy()
        y[:, lo], y[:, hi] = -50.0, 60.0
        want = VR.minmax_ref(y)
        assert np.array_equal(_minmax(y), want)
        assert (want[:, 0] == -50.0).all() and (want[:, 1] == 60.0).all()
    # all-negative and all-positive images (either branch of the integer min / max), and one
    # constant image among others
    for y in (-np.abs(x) - 1, np.abs(x) + 1):
        y[B // 2] = y[B // 2, 0]
        got = _minmax(y)
        assert np.array_equal(got, VR.minmax_ref(y)) and got[B // 2, 0] == got[B // 2, 1]


def test_image_minmax_takes_the_image_batch_shape():
    x = torch.randn(3, 3, 5, 7, device=DEV)
    x[1] = 0.0
    got = ops.image_minmax(x).cpu().numpy()
    assert np.array_equal(got, VR.minmax_ref(x.cpu().numpy())) and not got[1].any()
    assert ops.image_minmax(torch.empty(0, 3, 4, 4, device=DEV)).shape == (0, 2)
    with pytest.raises(ValueError):
        ops.image_minmax(torch.zeros(2, 3))  # a host tensor
    with pytest.raises(TypeError):
        ops.image_minmax(torch.zeros(2, 3, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------- cam_overlay
SHAPES = [(1, 7, 7, 224, 224),       # the ResNet map
          (3, 224, 224, 224, 224),   # the ViT saliency: identity taps
          (2, 5, 3, 37, 29),         # ragged: H * W * 3 is no multiple of 16, odd strides
          (1, 1, 1, 8, 8),
          (10, 7, 7, 224, 224)]      # the pass's ten samples


@functools.lru_cache(maxsize=None)
def _case(shape, custom_lut):
    """Inputs of one shape and the restatement's image and heat map for them (computed once,
    shared by every alpha, never modified)."""
    B, h, w, H, W = shape
    rng = np.random.default_rng(B * 1000003 + h * 10007 + H * 101 + W)
    x = (rng.normal(size=(B, 3, H, W)) * rng.uniform(0.3, 4, (B, 1, 1, 1)) +
         rng.uniform(-3, 3, (B, 1, 1, 1))).astype(np.float32)
    cam = rng.random((B, h, w), dtype=np.float32)
    cam[:, -1, -1] = 1.0
    if h * w > 1:
        cam[:, 0, 0] = 0.0
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8) if custom_lut else None
    image = VR.image_ref(x)
    heat = VR.heatmap_ref(cam, H, W, lut)
    for a in (x, cam, image, heat) + ((lut,) if custom_lut else ()):
        a.setflags(write=False)
    return x, cam, lut, image, heat


def _poisoned(nbytes):
    return tuple(torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
                 for _ in range(3))


def _run_overlay(x, cam, alpha, lut=None, minmax=None):
    """ops.cam_overlay into poisoned buffers with a GUARD-byte tail each; returns the three host
    pictures after checking the tails untouched."""
    B, _, H, W = x.shape
    nbytes = B * H * W * 3
    out = _poisoned(nbytes)
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    got = ops.cam_overlay(dev(x), dev(cam), alpha=alpha, lut=dev(lut), minmax=dev(minmax),
                          out=out)
    assert len(got) == 3
    host = []
    for g, o, name in zip(got, out, PICTURES):
        assert g.data_ptr() == o.data_ptr() and g.shape == (B, H, W, 3), name
        assert g.dtype == torch.uint8 and g.is_cuda
        assert (o[nbytes:] == POISON).all().item(), f"{name}: bytes past the picture written"
        host.append(g.cpu().numpy())
    return host


@pytest.mark.parametrize("custom_lut", [False, True])
@pytest.mark.parametrize("alpha", [0.5, 0.3, 0.0, 1.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_cam_overlay_against_the_restatement(shape, alpha, custom_lut):
    x, cam, lut, image, heat = _case(shape, custom_lut)
    got = _run_overlay(x, cam, alpha, lut)
    want = (image, heat, VR.blend_ref(image, heat, alpha))
    for g, r, name in zip(got, want, PICTURES):
        assert np.array_equal(g, r), f"{name}: {(g != r).sum()} of {r.size} bytes differ"
    if alpha == 0.0:
        assert np.array_equal(got[2], image)
    if alpha == 1.0:
        assert np.array_equal(got[2], heat)
    assert got[0].min() == 0 and got[0].max() == 255
    if not custom_lut:  # the exact 1.0 and 0.0 of the map take the table's two ends
        assert got[1][0, -1, -1].tolist() == [128, 0, 0]
        if shape[1] * shape[2] > 1:
            assert got[1][0, 0, 0].tolist() == [0, 0, 128]


def test_cam_overlay_own_buffers_unaligned_buffers_and_given_minmax():
    shape = (2, 5, 3, 37, 29)
    x, cam, _, image, heat = _case(shape, False)
    want = (image, heat, VR.blend_ref(image, heat, 0.5))
    xd, cd = torch.from_numpy(np.array(x)).to(DEV), torch.from_numpy(np.array(cam)).to(DEV)
    # the wrapper's own buffers
    got = ops.cam_overlay(xd, cd)
    for g, r in zip(got, want):
        assert g.shape == r.shape and np.array_equal(g.cpu().numpy(), r)
    # buffers that start 1, 2 and 3 bytes off a 16-byte boundary: the bytewise stores
    nbytes = image.size
    base = _poisoned(nbytes + 16)
    out = tuple(b[k + 1:k + 1 + nbytes + GUARD] for k, b in enumerate(base))
    got = ops.cam_overlay(xd, cd, out=out)
    for k, (g, r, b) in enumerate(zip(got, want, base)):
        assert g.data_ptr() == b.data_ptr() + k + 1 and g.data_ptr() % 16
        assert np.array_equal(g.cpu().numpy(), r)
        assert (b[:k + 1] == POISON).all().item() and (b[k + 1 + nbytes:] == POISON).all().item()
    # a caller's minmax replaces the image's own
    mm = np.array([[-40.0, 40.0], [-25.0, 30.0]], np.float32)  # wider than the data
    got = _run_overlay(x, cam, 0.3, minmax=mm)
    image2 = VR.image_ref(x, mm)
    assert np.array_equal(got[0], image2) and not np.array_equal(image2, image)
    assert np.array_equal(got[1], heat)
    assert np.array_equal(got[2], VR.blend_ref(image2, heat, 0.3))
    # an empty batch launches nothing
    empty = ops.cam_overlay(torch.empty(0, 3, 8, 8, device=DEV), torch.empty(0, 2, 2, device=DEV))
    assert all(e.shape == (0, 8, 8, 3) and e.dtype == torch.uint8 for e in empty)


def test_constant_image_gives_zeros():
    """max == min: an all-zero picture (the script's division gives NaN there), and the overlay
    is the blend of zeros with the heat map."""
    x, cam, _, _, heat = _case((2, 5, 3, 37, 29), False)
    x = np.array(x)
    x[1] = -1.25
    for alpha in (0.5, 0.3):
        image, heatmap, overlay = _run_overlay(x, cam, alpha)
        assert not image[1].any() and image[0].max() == 255
        assert np.array_equal(heatmap, heat)
        assert np.array_equal(overlay[1], VR.blend_ref(np.zeros_like(heat[1]), heat[1], alpha))
        assert np.array_equal(overlay, VR.overlay_ref(x, cam, alpha)[2])


def test_cam_overlay_rejects_bad_arguments():
    B, H, W = 2, 8, 8
    x = torch.randn(B, 3, H, W, device=DEV)
    cam = torch.rand(B, 2, 2, device=DEV)
    nbytes = B * H * W * 3
    out = _poisoned(nbytes)

    def refused(exc, *args, **kw):
        with pytest.raises(exc):
            ops.cam_overlay(*args, out=kw.pop("out", out), **kw)
        assert all((o == POISON).all().item() for o in out), "a refused call wrote"

    refused(ValueError, x.cpu(), cam)                                   # a host tensor
    refused(ValueError, x, cam.cpu())
    refused(TypeError, x.double(), cam)
    refused(ValueError, torch.randn(B, 4, H, W, device=DEV), cam)        # C != 3
    refused(ValueError, torch.randn(B, 1, H, W, device=DEV), cam)
    refused(ValueError, x, torch.rand(B + 1, 2, 2, device=DEV))          # batch mismatch
    refused(ValueError, x, torch.rand(2, 2, device=DEV))
    wide = torch.full((3, nbytes + GUARD, 2), POISON, dtype=torch.uint8, device=DEV)
    refused(ValueError, x, cam, out=tuple(wide[i, :, 0] for i in range(3)))  # non-contiguous
    assert (wide == POISON).all().item()
    refused(ValueError, x, cam, out=(out[0], out[1], out[2][:nbytes - 1]))   # too small
    refused(TypeError, x, cam, out=(out[0], out[1], out[2].view(torch.int8)))
    refused(ValueError, x, cam, lut=torch.zeros(255, 3, dtype=torch.uint8, device=DEV))
    refused(ValueError, x, cam, lut=torch.zeros(3, 256, dtype=torch.uint8, device=DEV))
    refused(TypeError, x, cam, lut=torch.zeros(256, 3, dtype=torch.int32, device=DEV))
    refused(ValueError, x, cam, lut=torch.zeros(256, 3, dtype=torch.uint8))
    refused(ValueError, x, cam, minmax=torch.zeros(B + 1, 2, device=DEV))
    # and the same buffers take a good call afterwards
    got = ops.cam_overlay(x, cam, out=out)
    want = VR.overlay_ref(x.cpu().numpy(), cam.cpu().numpy())
    assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, want))


# ------------------------------------------------------------------ training.gradcam_viz
def test_overlay_gradcam_on_image():
    rng = np.random.default_rng(8)
    cam = rng.random((7, 7), dtype=np.float32)
    cam[3, 3], cam[0, 6] = 1.0, 0.0
    u8 = rng.integers(0, 256, (37, 29, 3), dtype=np.uint8)
    u8[0, 0], u8[0, 1] = 0, 255
    for image, alpha in ((u8, 0.5), (u8, 0.3), (rng.random((37, 29, 3)), 0.5),
                         (rng.random((16, 16, 3), dtype=np.float32), 0.5),
                         (rng.random((8, 8, 3)) * 255, 0.5)):
        overlay, heatmap = V.overlay_gradcam_on_image(image, cam, alpha)
        want_overlay, want_heatmap = VR.overlay_on_image_ref(image, cam, alpha)
        assert overlay.dtype == heatmap.dtype == np.uint8
        assert overlay.shape == heatmap.shape == image.shape
        assert np.array_equal(heatmap, want_heatmap) and np.array_equal(overlay, want_overlay)
    # the image enters the blend as given: at alpha = 0 it comes back unchanged
    assert np.array_equal(V.overlay_gradcam_on_image(u8, cam, 0.0)[0], u8)


@functools.lru_cache(maxsize=None)
def _model(kind):
    """A randomly initialised model of a kind with non-trivial BatchNorm running statistics
    (Grad-CAM runs the model in eval mode), as test_gradcam_gpu.py::_pair sets them."""
    torch.manual_seed(KINDS.index(kind))
    model = V._build_model(kind)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(torch.randn(buf.shape, generator=gen) * 0.1)
            elif name.endswith("running_var"):
                buf.copy_(torch.rand(buf.shape, generator=gen) * 1.5 + 0.5)
    return model.to(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_visualize_batch(kind):
    from models.gradcam import GradCAM
    model = _model(kind)
    g = torch.Generator().manual_seed(17)
    rgb = (torch.randn(2, 3, 224, 224, generator=g) * 1.1).to(DEV)
    thermal = (torch.rand(2, 3, 224, 224, generator=g) * 2 - 1).to(DEV)
    inputs = {"rgb_only": {"rgb": rgb}, "thermal_only": {"thermal": thermal},
              "multimodal": {"rgb": rgb, "thermal": thermal}}[kind]
    model.train()
    res = V.visualize_batch(model, kind, **inputs)
    assert not model.training
    assert not any(m._forward_hooks for m in model.modules()), "hooks left behind"
    suffixes = ("_rgb", "_thermal") if kind == "multimodal" else ("",)
    assert set(res) == {"prediction", "confidence"} | {n + s for s in suffixes
                                                       for n in ("cam",) + PICTURES}
    assert all(isinstance(v, np.ndarray) for v in res.values())
    # prediction and confidence: softmax / argmax of a direct eval forward
    with torch.no_grad():
        probs = torch.softmax(model(*inputs.values()).float(), dim=1).cpu()
    assert res["prediction"].dtype == np.int64 and res["confidence"].dtype == np.float32
    assert res["prediction"].tolist() == probs.argmax(1).tolist()
    assert np.abs(res["confidence"] - probs.max(1).values.numpy()).max() <= 1e-6
    # the maps: a direct generate_cams call on the same model and inputs, bit for bit
    if kind == "rgb_only":
        encoders = [("", model, ["layer4"], rgb)]
    elif kind == "thermal_only":
        encoders = [("", model.vit, ["blocks"], thermal)]
    else:
        encoders = [("_rgb", model.resnet, ["layer4"], rgb),
                    ("_thermal", model.vit, ["blocks"], thermal)]
    for suffix, encoder, layers, x in encoders:
        grad_cam = GradCAM(encoder, layers)
        direct = grad_cam.generate_cams(x).cpu().numpy()
        grad_cam.remove()
        cam = res["cam" + suffix]
        assert cam.dtype == np.float32 and np.array_equal(cam, direct)
        assert cam.shape == ((2, 7, 7) if layers == ["layer4"] else (2, 224, 224))
        assert abs(cam.max() - 1.0) < 1e-6 and cam.min() >= 0.0
        # the pictures: the restatement applied to the inputs and the returned maps
        want = VR.overlay_ref(x.cpu().numpy(), cam)
        for name, r in zip(PICTURES, want):
            got = res[name + suffix]
            assert got.shape == (2, 224, 224, 3) and got.dtype == np.uint8
            assert np.array_equal(got, r), name + suffix
    with pytest.raises(ValueError):
        V.visualize_batch(model, "fusion", **inputs)
    with pytest.raises(ValueError):
        V.visualize_batch(model, kind)


def test_run_gradcam_visualization_on_a_synthetic_tree(tmp_path, capsys):
    pytest.importorskip("matplotlib")
    from PIL import Image
    from data import multimodal as MM
    from data import single_modality as SM
    rgb_dir, th_dir = DI.build_tree(str(tmp_path / "data"))
    random.seed(42)
    datasets = {"rgb_only": SM.RGBDataset(rgb_dir, "test", verbose=False),
                "thermal_only": SM.ThermalDataset(th_dir, "test", verbose=False),
                "multimodal": MM.MultimodalDataset(rgb_dir, th_dir, "test", verbose=False)}
    assert sorted(datasets["rgb_only"].labels) == [0, 0, 1, 1, 1]
    assert datasets["thermal_only"].labels == [0] * 4 and datasets["multimodal"].labels() == [0] * 4
    models = {kind: _model(kind) for kind in KINDS}
    out = tmp_path / "grad_cam_visualizations"
    # (two and one per class: seven figures; saving one takes most of this test's time)
    written = V.run_gradcam_visualization(models, datasets, str(out), num_healthy=2,
                                          num_ulcer=1)
    want = {"rgb_only": ["healthy_00.png", "healthy_01.png", "ulcer_00.png"],
            "thermal_only": ["healthy_00.png", "healthy_01.png"],
            "multimodal": ["healthy_00.png", "healthy_01.png"]}
    assert sorted(os.listdir(str(out))) == sorted(KINDS)
    for kind in KINDS:
        assert sorted(os.listdir(str(out / kind))) == want[kind]
    assert [os.path.relpath(p, str(out)) for p in written] == \
        [os.path.join(kind, name) for kind in KINDS for name in want[kind]]
    for p in written:
        with Image.open(p) as im:
            assert im.format == "PNG" and im.size[0] > 1000
    text = capsys.readouterr().out
    assert "Saved 3 RGB-only visualizations (2 healthy, 1 ulcer)" in text
    assert "Saved 2 Multimodal visualizations (2 healthy, 0 ulcer)" in text
    assert "Checkpoint not found" not in text
    assert not any(m._forward_hooks for model in models.values() for m in model.modules())
