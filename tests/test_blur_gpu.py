"""The GaussianBlur of the thermal-only train transform on the GPU (dfu_augment_blur,
k_augment_blur in csrc/augment.hip, through GT.GpuPreprocessor) against tests/blur_ref.py: the
pre-blur image from the PIL oracle, the blur in fp64, exact equality with round_half_even
outside a derived tie zone.  Output sizes cover every tap a reflection (2 x 2), exactly one
32 x 8 tile, one row and one column past a tile, and several tiles each way."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import blur_ref as BR
from data import gpu_transforms as GT
from data import single_modality as SM
from dfu_hip import _lib as L
from dfu_hip import ops

import data_inputs as DI  # noqa: E402  (oracle/, on the path through blur_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [(2, 2), (3, 5), (8, 32), (9, 33), (65, 40), (224, 224)]
RAGGED = [(37, 53), (240, 320), (90, 70), (31, 200), (224, 224)]  # source (h, w)


def _spec(size, **kw):
    """A bare GaussianBlur after whatever the parameters ask for (pack_params takes the ops,
    the angle and the affine from the AugParams), thermal normalisation."""
    kw.setdefault("rotation", 30)
    return GT.TransformSpec(size=size, mean=GT.THERMAL_MEAN, std=GT.THERMAL_STD,
                            blur=(0.1, 0.5), blur_p=None, **kw)


def _plain(spec):
    return dataclasses.replace(spec, blur=None, blur_p=0.0)


def _run(spec, imgs, params, views=None):
    out = GT.GpuPreprocessor(spec)(imgs, params, views)
    assert out.is_cuda and out.dtype == torch.float32
    assert out.shape == (len(params), 3) + tuple(spec.size)
    return out.cpu()


# ------------------------------------------------------------------------------ blur alone
@pytest.mark.parametrize("sigma", [0.37, 0.5])
@pytest.mark.parametrize("size", SIZES)
def test_blur_alone(size, sigma):
    """Sources at the output size (the resize is skipped, the noise of the fixture survives):
    at least half the values change, so agreement with the reference is not vacuous."""
    spec = _spec(size)
    seed = 12 if size == (3, 5) else 11  # 45 values: one in the tie zone is over the 1 % cap
    imgs = [BR.img(*size, seed), BR.img(*size, seed + 1)]
    params = [GT.AugParams(blur=sigma), GT.AugParams(blur=sigma, vflip=True)]
    out = _run(spec, imgs, params)
    for i in range(2):
        e = BR.check(out[i], imgs[i], spec, params[i], f"{size} sigma {sigma} image {i}")
        changed = (out[i] != e.plain).float().mean().item()
        print(f"\n[blur {size} sigma {sigma} image {i}] zone {e.zone:.4f} changed {changed:.3f}")
        assert changed >= 0.5


@pytest.mark.parametrize("size", SIZES)
def test_sigma_tenth_leaves_the_image_unchanged(size):
    """sigma = 0.1: the side weights are 1.9e-22, every sum rounds back to the centre pixel."""
    spec = _spec(size)
    imgs = [BR.img(h, w, 20 + i) for i, (h, w) in enumerate([size, RAGGED[0]])]
    params = [GT.AugParams(blur=0.1, hflip=True), GT.AugParams(blur=0.1, angle=-8.0)]
    assert GT.blur_weights(0.1)[1] == 1.0 and GT.blur_weights(0.1)[0] > 0
    out = _run(spec, imgs, params)
    same = _run(_plain(spec), imgs, params)  # dfu_augment_normalize
    for i in range(2):
        e = BR.check(out[i], imgs[i], spec, params[i], f"{size} image {i}")
        assert torch.equal(out[i], e.plain) and torch.equal(out[i], same[i])


# ---------------------------------------------------------------- after the other random ops
GEOMETRY = [
    GT.AugParams(hflip=True, angle=17.0, blur=0.5),
    GT.AugParams(affine=(6.0, (3, -2), 1.0, (0.0, 0.0)), blur=0.37),
    GT.AugParams(hflip=True, vflip=True, angle=17.0, affine=(-9.0, (5, 4), 0.85, (0.0, 0.0)),
                 blur=0.5),
]


@pytest.mark.parametrize("size", SIZES)
def test_blur_after_geometry(size):
    """The rotation's and the affine's black fill meets the image inside the frame: blurring
    before the maps, or reflecting the source instead of the augmented image, differs there."""
    spec = _spec(size)
    imgs = [BR.img(h, w, 30 + i) for i, (h, w) in enumerate(RAGGED[:3])]
    out = _run(spec, imgs, GEOMETRY)
    for i, p in enumerate(GEOMETRY):
        e = BR.check(out[i], imgs[i], spec, p, f"{size} case {i}")
        if min(size) >= 40:  # below that a translate by 5 leaves little but fill
            fill = (e.pre == 0).all(0)
            assert 0.01 <= fill.float().mean().item() <= 0.6, "the case should show fill"
            # the blur of the fill's rim: neither black nor the unblurred neighbour
            assert ((out[i] != e.plain).any(0) & ~fill).any()


COLOUR = [
    GT.AugParams(ops=[(GT.BRIGHTNESS, 1.2), (GT.CONTRAST, 0.75), (GT.SATURATION, 1.3)],
                 blur=0.5),
    GT.AugParams(ops=[(GT.SATURATION, 0.7), (GT.CONTRAST, 1.25), (GT.BRIGHTNESS, 0.9)],
                 hflip=True, angle=-12.0, affine=(4.0, (-3, 2), 1.1, (0.0, 0.0)), blur=0.37),
]


@pytest.mark.parametrize("size", [(9, 33), (65, 40), (224, 224)])
def test_blur_after_colour(size):
    """All three jitter ops in two orders: the contrast mean is of the pre-blur image."""
    spec = _spec(size, jitter=(0.3, 0.3, 0.3))
    imgs = [BR.img(h, w, 40 + i) for i, (h, w) in enumerate([size, RAGGED[1]])]
    out = _run(spec, imgs, COLOUR)
    for i, p in enumerate(COLOUR):
        BR.check(out[i], imgs[i], spec, p, f"{size} case {i}")


# ----------------------------------------------------------------------------- mixed batches
@pytest.mark.parametrize("size", [(9, 33), (65, 40)])
def test_mixed_batch_rows_are_independent(size):
    spec = _spec(size, jitter=(0.3, 0.3, 0.3))
    imgs = [BR.img(h, w, 50 + i) for i, (h, w) in enumerate(RAGGED)]
    params = [
        GT.AugParams(hflip=True, angle=6.0, blur=0.5),
        GT.AugParams(vflip=True, angle=-20.0, ops=[(GT.CONTRAST, 0.8)],
                     affine=(7.0, (2, 1), 0.9, (0.0, 0.0))),             # unblurred
        GT.AugParams(affine=(-15.0, (-3, 3), 1.15, (0.0, 0.0)), blur=0.37),
        GT.AugParams(angle=11.0),                                         # unblurred
        GT.AugParams(ops=[(GT.CONTRAST, 1.2), (GT.BRIGHTNESS, 0.8)], blur=0.45),
    ]
    out = _run(spec, imgs, params)
    plain = _run(_plain(spec), imgs, params)  # dfu_augment_normalize on the same records
    for i, p in enumerate(params):
        BR.check(out[i], imgs[i], spec, p, f"{size} row {i}")
        if p.blur is None:
            assert torch.equal(out[i], plain[i]), i
        else:
            assert not torch.equal(out[i], plain[i]), i
            alone = _run(spec, imgs[i:i + 1], [p])  # a batch of one: no cross-image dependence
            assert torch.equal(out[i], alone[0]), i


def test_views_path_rotate_flip():
    """views = 3 in the TTA Compose's order (rotation before the flips), one view of each image
    unblurred: those equal dfu_augment_views' output bitwise."""
    K, size = 3, (65, 40)
    spec = dataclasses.replace(_spec(size, rotation=15), order="rotate_flip")
    imgs = [BR.img(h, w, 60 + i) for i, (h, w) in enumerate(RAGGED[:2])]
    params = [
        GT.AugParams(hflip=True, angle=12.5, affine=(-7.0, (3, -2), 1.0, (0.0, 0.0)), blur=0.5),
        GT.AugParams(vflip=True, angle=-15.0, affine=(10.0, (-2, 2), 1.0, (0.0, 0.0))),
        GT.AugParams(hflip=True, vflip=True, angle=3.0, blur=0.37),
        GT.AugParams(angle=-4.0),
        GT.AugParams(vflip=True, angle=9.0, blur=0.3),
        GT.AugParams(hflip=True, angle=14.0, affine=(2.0, (1, 0), 1.0, (0.0, 0.0)), blur=0.45),
    ]
    out = _run(spec, imgs, params, views=K)
    plain = _run(_plain(spec), imgs, params, views=K)  # dfu_augment_views
    for v, p in enumerate(params):
        BR.check(out[v], imgs[v // K], spec, p, f"view {v}")
        if p.blur is None:
            assert torch.equal(out[v], plain[v]), v
    assert not torch.equal(out[0], plain[0]) and not torch.equal(out[2], plain[2])
    # without views the spec's order still holds (the preprocessor passes it on)
    one = _run(spec, imgs[:1], params[:1])
    assert torch.equal(one[0], out[0])


# ---------------------------------------------------------------------------- the C entry
def _blur_call(resized, rec, blur_k, out, H=None, W=None, view_src=None, order=0):
    n = resized.shape[0]
    mean = (ctypes.c_float * 3)(*GT.THERMAL_MEAN)
    std = (ctypes.c_float * 3)(*GT.THERMAL_STD)
    par = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    bk = torch.from_numpy(np.ascontiguousarray(blur_k, np.float32)).to(DEV)
    means = torch.empty(len(rec), dtype=torch.int32, device=DEV)
    vs = None if view_src is None else torch.tensor(view_src, dtype=torch.int32, device=DEV)
    rc = L.load().dfu_augment_blur(
        resized.data_ptr(), n, par.data_ptr(), None if vs is None else vs.data_ptr(),
        bk.data_ptr(), len(rec), order, resized.shape[1] if H is None else H,
        resized.shape[2] if W is None else W, mean, std, means.data_ptr(), out.data_ptr(),
        ops.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("size", [(3, 5), (9, 33)])
def test_direct_call_stays_inside_its_output(size):
    """out carved from a NaN-filled buffer with a sentinel row before and after: every value
    inside is written, nothing outside is."""
    H, W = size
    spec = _spec(size)
    imgs = [BR.img(H, W, 70 + i) for i in range(3)]
    params = [GT.AugParams(blur=0.5), GT.AugParams(hflip=True, angle=17.0),
              GT.AugParams(vflip=True, angle=-5.0, affine=(3.0, (1, -1), 0.9, (0.0, 0.0)),
                           blur=0.37)]
    blur_k = np.stack([GT.blur_weights(p.blur) if p.blur is not None else np.zeros(3, np.float32)
                       for p in params])
    resized = torch.from_numpy(np.stack(imgs)).to(DEV)
    buf = torch.full((len(imgs) + 2, 3 * H * W), float("nan"), device=DEV)
    out = buf[1:-1]
    assert _blur_call(resized, GT.pack_params(params, spec), blur_k, out) == 0
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all()
    assert not torch.isnan(out).any()
    for i, p in enumerate(params):
        BR.check(out[i].view(3, H, W), imgs[i], spec, p, f"{size} image {i}")
    # view_src: outputs in another order than the images, one index outside the batch -> fill
    buf.fill_(float("nan"))
    assert _blur_call(resized, GT.pack_params(params, spec), blur_k, out, view_src=[2, 7, 0]) == 0
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all()
    BR.check(out[0].view(3, H, W), imgs[2], spec, params[0], "view 0 of image 2")
    assert (out[1] == -1.0).all()  # (0 - 0.5) / 0.5
    BR.check(out[2].view(3, H, W), imgs[0], spec, params[2], "view 2 of image 0")
    # one pixel each way cannot be reflected
    assert _blur_call(resized, GT.pack_params(params, spec), blur_k, out, H=1) == L.DFU_E_INVALID
    assert _blur_call(resized, GT.pack_params(params, spec), blur_k, out, W=1) == L.DFU_E_INVALID
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all()


# ------------------------------------------------------------------------------ the loader
def test_thermal_only_loader_matches_reference(tmp_path):
    """The thermal-only script's train loader: every batch equals the reference recomputed from
    a second generator with the same seed."""
    _, th_dir = DI.build_tree(str(tmp_path))
    ds = SM.ThermalDataset(th_dir, "train", verbose=False)
    spec = GT.thermal_only_train_transform
    g = torch.Generator().manual_seed(7)
    loader = GT.GpuImageLoader(ds, 6, train=True, spec=spec, generator=g, num_threads=2)
    batches = list(loader)
    assert len(batches) == len(loader) == -(-len(ds) // 6) and len(ds) == 16
    g = torch.Generator().manual_seed(7)
    at, blurred = 0, 0
    for x, y in batches:
        assert x.is_cuda and x.shape[1:] == (3, 224, 224)
        assert y.tolist() == [ds.labels[i] for i in range(at, at + len(y))]
        x = x.cpu()
        for j in range(len(y)):
            p = GT.sample_params(spec, g)
            BR.check(x[j], GT.decode_rgb(ds.image_paths[at + j]), spec, p, f"sample {at + j}")
            blurred += p.blur is not None
        at += len(y)
    assert at == 16 and 0 < blurred < 16
