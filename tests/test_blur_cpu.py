"""Host side of the GaussianBlur of the thermal-only train transform (data/gpu_transforms.py;
notebooks/train_thermal_only.py:103-112): the weights, the spec's constants, the draw order, the
staging layout and the size check, and the reference of tests/blur_ref.py against torch's own
fp32 conv2d.  No GPU."""
import dataclasses

import numpy as np
import pytest
import torch

import blur_ref as BR
from data import gpu_transforms as GT
from dfu_hip import _lib as L


def _uniform(a, b, g):
    return float(torch.empty(1).uniform_(a, b, generator=g).item())


@pytest.mark.parametrize("sigma", [0.1, 0.25, 0.37, 0.5])
def test_blur_weights_are_torchvisions(sigma):
    """_get_gaussian_kernel1d(3, sigma), restated."""
    x = torch.linspace(-1, 1, steps=3)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    want = (pdf / pdf.sum()).numpy()
    got = GT.blur_weights(sigma)
    assert got.dtype == np.float32 and got.shape == (3,)
    assert got.tobytes() == want.tobytes()
    assert got[0] == got[2] and got[1] > got[0] > 0


def test_batched_weights_are_the_per_sample_expression():
    """The staging path computes a batch's weights in one set of torch calls: each row has the
    bits of torchvision's expression evaluated for that sigma alone, and rows where no blur was
    drawn are zero."""
    g = torch.Generator().manual_seed(9)
    sig = [float(torch.empty(1).uniform_(0.1, 0.5, generator=g).item()) for _ in range(2000)]
    sig += [0.1, 0.5, 0.37, 1 / 3]
    sig[5] = sig[17] = None
    rows = GT.blur_weight_rows(sig)
    assert rows.dtype == np.float32 and rows.shape == (len(sig), 3)
    x = torch.linspace(-1, 1, steps=3)
    for r, s_ in zip(rows, sig):
        if s_ is None:
            assert not r.any()
            continue
        pdf = torch.exp(-0.5 * (x / s_).pow(2))
        assert r.tobytes() == (pdf / pdf.sum()).numpy().tobytes(), s_
    assert GT.blur_weight_rows([]).shape == (0, 3)


def test_thermal_only_constants_carry_the_scripts_values():
    s, t = GT.thermal_only_train_transform, GT.thermal_train_transform
    assert s.blur == (0.1, 0.5) and s.blur_p == GT.AUG_PROB == 0.6 and s.blur_kernel == 3
    assert t.blur is None and GT.rgb_train_transform.blur is None
    assert dataclasses.replace(s, blur=None, blur_p=0.0) == t  # the thermal train spec + blur
    assert (s.hflip_p, s.vflip_p, s.rotation, s.jitter) == (0.5, 0.5, 30, None)
    assert s.affine == (20, (0.1, 0.1), (0.8, 1.2)) and s.affine_p == 0.6
    assert (s.mean, s.std, s.size) == (GT.THERMAL_MEAN, GT.THERMAL_STD, (224, 224))
    assert s.random and GT.TransformSpec(blur=(0.1, 0.5), blur_p=None).random
    assert not GT.TransformSpec().random
    with pytest.raises(NotImplementedError):
        GT.TransformSpec(blur=(0.1, 0.5), blur_kernel=5)


def test_thermal_only_draw_sequence():
    """train_thermal_only.py:103-112 in Compose order: the two flips, RandomRotation(30),
    RandomApply(RandomAffine), RandomApply(GaussianBlur): coin, then sigma."""
    spec = GT.thermal_only_train_transform
    g, h = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    blurred = 0
    for _ in range(40):
        p = GT.sample_params(spec, g)
        hflip = bool(torch.rand(1, generator=h) < 0.5)
        vflip = bool(torch.rand(1, generator=h) < 0.5)
        angle = _uniform(-30.0, 30.0, h)
        affine = None
        if not (0.6 < torch.rand(1, generator=h)):
            a = _uniform(-20.0, 20.0, h)
            tx = int(round(_uniform(-float(0.1 * 224), float(0.1 * 224), h)))
            ty = int(round(_uniform(-float(0.1 * 224), float(0.1 * 224), h)))
            affine = (a, (tx, ty), _uniform(0.8, 1.2, h), (0.0, 0.0))
        sigma = None
        if not (0.6 < torch.rand(1, generator=h)):
            sigma = _uniform(0.1, 0.5, h)
        assert (p.hflip, p.vflip, p.angle, p.affine, p.blur, p.ops) == \
            (hflip, vflip, angle, affine, sigma, [])
        assert sigma is None or 0.1 <= sigma <= 0.5
        assert torch.equal(g.get_state(), h.get_state())
        blurred += sigma is not None
    assert 0 < blurred < 40


def test_bare_blur_draws_no_coin():
    spec = GT.TransformSpec(blur=(0.2, 0.4), blur_p=None)
    g, h = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for _ in range(10):
        p = GT.sample_params(spec, g)
        assert p.blur == _uniform(0.2, 0.4, h)
        assert torch.equal(g.get_state(), h.get_state())
    # blur_p = 0: RandomApply never applies (0 < rand), and the coin is still drawn
    spec = GT.TransformSpec(blur=(0.2, 0.4), blur_p=0.0)
    p = GT.sample_params(spec, g)
    torch.rand(1, generator=h)
    assert p.blur is None and torch.equal(g.get_state(), h.get_state())


def _align(n, a=256):
    return (n + a - 1) // a * a


def _parent_layout(imgs, rec, view_src, spec):
    """The staging buffer as it was before blur_k existed: [descs | params, view_src | taps |
    pixels], 256-byte aligned sections, 4 spare bytes at the end."""
    OH, OW = spec.size
    desc = np.zeros(len(imgs), GT.RESIZE_DESC)
    taps, coef_len, src_len, tmp_len = [], 0, 0, 0
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        kh, bh, wh = GT.resize_taps(w, OW)
        kv, bv, wv = GT.resize_taps(h, OH)
        desc[i] = (src_len, tmp_len, coef_len, w, h, kh, kv)
        taps += [bh, wh, bv, wv]
        coef_len += bh.size + wh.size + bv.size + wv.size
        src_len += im.size
        tmp_len += h * OW * 3
    o_par = _align(desc.nbytes)
    o_coef = o_par + _align(rec.nbytes + view_src.nbytes)
    o_src = o_coef + _align(coef_len * 4)
    sections = [(0, desc.view(np.uint8)), (o_par, rec.view(np.uint8)),
                (o_par + rec.nbytes, view_src.view(np.uint8)),
                (o_coef, np.concatenate([t.ravel() for t in taps]).astype(np.int32).view(np.uint8)),
                (o_src, np.concatenate([im.ravel() for im in imgs]))]
    return o_src + src_len + 4, sections


@pytest.mark.parametrize("views", [None, 2])
def test_staging_without_blur_is_the_parents_layout(views):
    spec = dataclasses.replace(GT.thermal_train_transform, size=(12, 20))
    imgs = [BR.img(h, w, i) for i, (h, w) in enumerate([(9, 14), (30, 7), (12, 20)])]
    g = torch.Generator().manual_seed(1)
    params = [GT.sample_params(spec, g) for _ in range(len(imgs) * (views or 1))]
    st = GT.GpuPreprocessor(spec, device="cpu").stage(imgs, params, views)
    rec = GT.pack_params(params, spec)
    view_src = (np.repeat(np.arange(len(imgs), dtype=np.int32), views) if views
                else np.empty(0, np.int32))
    total, sections = _parent_layout(imgs, rec, view_src, spec)
    buf = st.dev.numpy()
    assert buf.size == total and st.o_blur is None
    for off, data in sections:
        assert buf[off:off + data.size].tobytes() == data.tobytes(), off
    # the same sections at the same offsets: what lies between them is padding either way
    assert (st.o_par, st.o_view) == (sections[1][0], sections[2][0])
    assert (st.o_coef, st.o_src) == (sections[3][0], sections[4][0])


@pytest.mark.parametrize("views", [None, 2])
def test_staging_with_blur_appends_the_weight_rows(views):
    spec = dataclasses.replace(GT.thermal_only_train_transform, size=(12, 20))
    plain = dataclasses.replace(spec, blur=None, blur_p=0.0)
    imgs = [BR.img(h, w, i) for i, (h, w) in enumerate([(9, 14), (30, 7), (12, 20)])]
    nv = len(imgs) * (views or 1)
    sig = [0.37, None, 0.5, None, 0.1, 0.25][:nv]
    params = [GT.AugParams(hflip=i % 2 == 0, angle=3.0 * i, blur=s) for i, s in enumerate(sig)]
    st = GT.GpuPreprocessor(spec, device="cpu").stage(imgs, params, views)
    base = GT.GpuPreprocessor(plain, device="cpu").stage(imgs, params, views)
    rec_bytes = nv * GT.AUG_PARAMS.itemsize + (nv * 4 if views else 0)
    assert st.o_par == base.o_par and st.o_view == base.o_view
    assert st.o_blur == st.o_par + _align(rec_bytes) and st.o_blur % 256 == 0
    assert st.o_coef == st.o_blur + _align(nv * 12)
    shift = st.o_coef - base.o_coef
    assert st.o_src == base.o_src + shift and st.dev.numel() == base.dev.numel() + shift
    a = st.dev.numpy()
    view_src = (np.repeat(np.arange(len(imgs), dtype=np.int32), views) if views
                else np.empty(0, np.int32))
    _, sections = _parent_layout(imgs, GT.pack_params(params, spec), view_src, spec)
    for off, data in sections:  # every other section unchanged; taps and pixels moved up
        off += shift if off >= base.o_coef else 0
        assert a[off:off + data.size].tobytes() == data.tobytes(), off
    rows = a[st.o_blur:st.o_blur + nv * 12].view(np.float32).reshape(nv, 3)
    for r, s in zip(rows, sig):
        want = GT.blur_weights(s) if s is not None else np.zeros(3, np.float32)
        assert r.tobytes() == want.tobytes() and (r[1] > 0) == (s is not None)


@pytest.mark.parametrize("size", [(1, 8), (8, 1), (1, 1)])
def test_blur_needs_two_pixels_each_way(size):
    with pytest.raises(ValueError):
        GT.GpuPreprocessor(GT.TransformSpec(size=size, blur=(0.1, 0.5), blur_p=None), device="cpu")
    GT.GpuPreprocessor(GT.TransformSpec(size=size), device="cpu")  # no blur: any size
    # the C entry answers before any launch (host code, no device needed)
    lib = L.load()
    buf = np.zeros(64, np.int64).ctypes.data  # non-NULL, never dereferenced
    f3 = (L.c_float * 3)(0.5, 0.5, 0.5)
    call = lambda **k: lib.dfu_augment_blur(  # noqa: E731
        buf, 1, buf, k.get("view_src", None), k.get("blur_k", buf), k.get("n_views", 1),
        k.get("order", 0), k.get("H", 4), k.get("W", 4), f3, f3, buf, buf, None)
    assert call(H=size[0], W=size[1]) == L.DFU_E_INVALID
    for bad in (dict(blur_k=None), dict(order=2), dict(n_views=0), dict(n_views=65536)):
        assert call(**bad) == L.DFU_E_INVALID, bad


@pytest.mark.parametrize("sigma", [0.3, 0.37, 0.5])
def test_reference_agrees_with_torch_conv2d(sigma):
    """torchvision's own evaluation -- fp32 conv2d of the reflect-padded image with the 2-D
    kernel mm(k[:, None], k[None, :]), torch.round, uint8 -- falls inside what blur_ref accepts,
    and so does a sequential row-major fp32 sum without FMA."""
    spec = GT.TransformSpec(size=(65, 40), mean=GT.THERMAL_MEAN, std=GT.THERMAL_STD)
    p = GT.AugParams(blur=sigma)
    e = BR.Expected(BR.img(65, 40, 4), spec, p)
    assert 0 < e.zone <= BR.ZONE_CAP or e.zone == 0
    k = torch.from_numpy(GT.blur_weights(sigma))
    k2 = torch.mm(k[:, None], k[None, :])
    x = torch.nn.functional.pad(e.pre.float()[None], (1, 1, 1, 1), mode="reflect")
    conv = torch.nn.functional.conv2d(x, k2.expand(3, 1, 3, 3), groups=3)[0]
    assert e.mismatches(BR.normalise(torch.round(conv).to(torch.uint8), spec)) == 0
    k2n, xn = k2.numpy(), x[0].numpy()
    acc = np.zeros((3, 65, 40), np.float32)
    for j in range(3):
        for i in range(3):
            acc = acc + k2n[j, i] * xn[:, j:j + 65, i:i + 40]
    assert acc.dtype == np.float32
    seq = torch.from_numpy(np.rint(acc)).to(torch.uint8)
    assert e.mismatches(BR.normalise(seq, spec)) == 0
    # and the blur is not a no-op on this image
    assert (e.lo != e.plain).float().mean().item() >= (0.5 if sigma >= 0.37 else 0.01)
