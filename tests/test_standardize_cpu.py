"""Host side of the aspect-preserving standardisation (data.gpu_transforms.letterbox_dims,
TransformSpec.standardize, GpuPreprocessor.stage; data.standardize) without a GPU: the geometry
against a table and against the script's plain expression, the refusals, that PIL's own letterbox
equals the two-pass model the kernels implement over the whole accepted domain, the staged
records, and the tree walk."""
import ctypes
import dataclasses

import numpy as np
import pytest
from PIL import Image

import standardize_ref as SR
from data import gpu_transforms as GT
from data import standardize as SZ
from dfu_hip import _lib as L

TR = SR.TR


@pytest.mark.parametrize("wh,out,pad", [
    ((640, 480), (224, 168), (0, 28)),
    ((480, 640), (168, 224), (28, 0)),
    ((55, 55), (223, 223), (0, 0)),
    ((40, 55), (162, 223), (31, 0)),
    ((300, 200), (224, 149), (0, 37)),
    ((1, 1), (224, 224), (0, 0)),
    ((224, 223), (224, 223), (0, 0)),
])
def test_letterbox_dims_table(wh, out, pad):
    assert GT.letterbox_dims(*wh, 224) == out + pad
    assert SR.dims(*wh, 224) == out + pad  # the helper's restatement agrees


def test_the_223_quirk_is_kept():
    """int(m * (224 / m)) is 223 for some longest edges m: the script's double rounding, which
    letterbox_dims must reproduce and not repair."""
    plain = [m for m in range(1, 5000) if int(m * (224 / m)) == 223]
    got = [m for m in range(1, 5000) if GT.letterbox_dims(m, m, 224)[0] == 223]
    assert got == plain and len(plain) == 392
    assert plain[:8] == [55, 71, 83, 95, 97, 107, 110, 111]
    for m in range(1, 5000):
        ow, oh, px, py = GT.letterbox_dims(m, m, 224)
        assert ow == oh and ow in (223, 224) and (px, py) == (0, 0)
    # the long side of a non-square image takes the same value, the strip is right or bottom
    assert GT.letterbox_dims(55, 40, 224) == (223, 162, 0, 31)


@pytest.mark.parametrize("wh,exc", [
    ((1, 1000), ValueError), ((3, 1000), ValueError),
    ((5, 1000), NotImplementedError), ((1000, 5), NotImplementedError),
    ((9, 1000), NotImplementedError),
])
def test_refusals(wh, exc):
    with pytest.raises(exc):
        GT.letterbox_dims(*wh, 224)
    if exc is ValueError:  # PIL refuses the same resize, so the script counts an error
        w, h, _, _ = SR.dims(*wh, 224)
        with pytest.raises(ValueError):
            Image.new("RGB", wh).resize((w, h), Image.BILINEAR)


def _domain_cases():
    """(w, h) over longest edges 60..4000 and short output sides 3..223 at their boundaries: for
    each pair the narrowest and the widest short source side that gives that output side, in
    both orientations.  The largest edges take the thin outputs only (a 4000 x 3980 source adds
    nothing but time)."""
    cases = []
    shorts, thin = (3, 4, 5, 17, 56, 112, 168, 220, 221, 222, 223), (3, 4, 5, 17)
    for long_edge in (60, 97, 111, 224, 225, 320, 640, 1000, 1500, 4000):
        scale = 224 / long_edge
        for s in shorts if long_edge <= 640 else thin:  # a short side no source gives: no case
            ms = [m for m in range(1, long_edge + 1) if int(m * scale) == s]
            for m in sorted({ms[0], ms[-1]}) if ms else ():
                cases += [(long_edge, m), (m, long_edge)]
    return list(dict.fromkeys(cases))  # a square source is its own other orientation


def test_pil_letterbox_stays_inside_the_modelled_domain():
    """With min(out_w, out_h) >= 3 PIL's resize is the horizontal-then-vertical two-pass
    resample the kernels implement (oracle/transforms_ref.resample_np), so PIL's letterbox
    equals resample_np + paste with zero differing bytes: the reference itself stays inside the
    condition letterbox_dims sets."""
    cases = _domain_cases()
    assert len(cases) >= 100 and len(set(cases)) == len(cases)
    assert any(w > h for w, h in cases) and any(h > w for w, h in cases)
    for k, (w, h) in enumerate(cases):
        ow, oh, px, py = GT.letterbox_dims(w, h, 224)
        assert min(ow, oh) >= 3
        im = SR.img(h, w, 1000 + k)
        want = np.zeros((224, 224, 3), np.uint8)
        want[py:py + oh, px:px + ow] = TR.resample_np(im, ow, oh)
        bad = int((SR.canvas(im) != want).sum())
        assert bad == 0, f"{w} x {h} -> {ow} x {oh}: {bad} bytes differ"
    print(f"\n[domain] {len(cases)} cases, 0 differing bytes")


def test_stage_packs_the_boxes_of_a_ragged_batch():
    spec = GT.standardized(GT.rgb_val_test_transform)
    sizes = [(48, 64), (64, 48), (55, 55), (55, 40), (1, 1), (224, 224), (20, 30)]  # (h, w)
    imgs = [SR.img(h, w, i) for i, (h, w) in enumerate(sizes)]
    st = GT.GpuPreprocessor(spec, device="cpu").stage(imgs)
    buf, n = st.dev.numpy(), len(imgs)
    desc = buf[:n * GT.RESIZE_DESC.itemsize].view(GT.RESIZE_DESC)
    assert st.o_box == desc.nbytes and st.o_par >= st.o_box + n * 16
    boxes = buf[st.o_box:st.o_box + n * 16].view(np.int32).reshape(n, 4)
    tmp_off = coef_off = 0
    for i, (h, w) in enumerate(sizes):
        ow, oh, px, py = GT.letterbox_dims(w, h, 224)
        assert tuple(boxes[i]) == (ow, oh, px, py)
        assert 0 < ow <= 224 and 0 < oh <= 224 and px + ow <= 224 and py + oh <= 224
        kh, bh, wh = GT.resize_taps(w, ow)
        kv, bv, wv = GT.resize_taps(h, oh)
        d = desc[i]
        assert (d["w"], d["h"], d["ksh"], d["ksv"]) == (w, h, kh, kv)
        assert (d["tmp_off"], d["coef_off"]) == (tmp_off, coef_off)
        taps = buf[st.o_coef:st.o_src].view(np.int32)[coef_off:]
        at = 0
        for a in (bh, wh, bv, wv):  # the taps of the image's own output sizes
            assert np.array_equal(taps[at:at + a.size], a.ravel())
            at += a.size
        tmp_off += h * ow * 3
        coef_off += at
    assert st.tmp_len == tmp_off
    # without the field nothing is added to the staging buffer
    plain = GT.GpuPreprocessor(GT.rgb_val_test_transform, device="cpu").stage(imgs)
    assert plain.o_box is None and plain.o_par == (desc.nbytes + 255) // 256 * 256


def test_stage_names_the_refused_image():
    pre = GT.GpuPreprocessor(GT.standardized(GT.thermal_val_test_transform), device="cpu")
    ok = SR.img(30, 40, 0)
    with pytest.raises(NotImplementedError, match="image 2 of the batch"):
        pre.stage([ok, ok, SR.img(1000, 5, 1), ok])
    with pytest.raises(ValueError, match="image 1 of the batch"):
        pre.stage([ok, SR.img(1000, 1, 2)])


def test_spec_field():
    with pytest.raises(NotImplementedError):
        GT.TransformSpec(standardize=224, size=(112, 112))
    with pytest.raises(NotImplementedError):
        GT.standardized(GT.rgb_train_transform, 256)
    with pytest.raises(ValueError):
        GT.TransformSpec(standardize=0, size=(0, 0))
    s = GT.standardized(GT.rgb_train_transform)
    assert s.standardize == 224
    assert dataclasses.replace(s, standardize=None) == GT.rgb_train_transform
    assert GT.rgb_train_transform.standardize is None
    assert GT.TransformSpec(size=(96, 96), standardize=96).standardize == 96


def test_entry_point_checks_its_arguments():
    """Host code: answered before any launch, no device needed."""
    lib, p = L.load(), ctypes.c_void_p(256)
    for args in [(None, p, p, p, 1, 224, p, p), (p, None, p, p, 1, 224, p, p),
                 (p, p, None, p, 1, 224, p, p), (p, p, p, None, 1, 224, p, p),
                 (p, p, p, p, 1, 224, None, p), (p, p, p, p, 1, 224, p, None),
                 (p, p, p, p, 0, 224, p, p), (p, p, p, p, 65536, 224, p, p),
                 (p, p, p, p, 1, 0, p, p), (p, p, p, p, 1, 26755, p, p)]:
        assert lib.dfu_letterbox_batch(*args, None) == L.DFU_E_INVALID, args


def _save(path, size, mode="RGB"):
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.new(mode, size, 7).save(path)


def test_tree_walk_and_verify(tmp_path):
    src = tmp_path / "raw"
    _save(src / "a.png", (224, 224))
    _save(src / "healthy" / "b.JPG", (224, 224))
    _save(src / "healthy" / "deep" / "c.Jpeg", (224, 224))     # mixed case: picked up here
    _save(src / "ulcer" / "d.TiF", (224, 224), "L")
    _save(src / "ulcer" / "e.bmp", (224, 200))                 # a wrong size
    (src / "ulcer" / "notes.txt").write_text("not an image")
    (src / "ulcer" / "dir.png").mkdir()                        # a directory with a suffix
    names = [p.relative_to(src).as_posix() for p in SZ.image_files(src)]
    assert names == ["a.png", "healthy/b.JPG", "healthy/deep/c.Jpeg", "ulcer/d.TiF", "ulcer/e.bmp"]
    ok, sizes = SZ.verify_standardization(src)
    assert ok is False and sizes == {(224, 224): 4, (224, 200): 1}
    (src / "ulcer" / "e.bmp").unlink()
    assert SZ.verify_standardization(src) == (True, {(224, 224): 4})
    assert SZ.verify_standardization(src, target_size=200) == (False, {(224, 224): 4})
    (src / "broken.png").write_bytes(b"\x89PNG no image")
    assert SZ.verify_standardization(src) == (False, {(224, 224): 4})
    assert SZ.verify_standardization(tmp_path / "raw" / "ulcer" / "dir.png") == (False, {})


def test_unreadable_and_refused_files_are_counted_before_any_gpu_work(tmp_path):
    """A tree whose every file fails on the host: counted, skipped, nothing reaches the device
    (this test has none)."""
    src, dst = tmp_path / "raw", tmp_path / "std"
    src.mkdir()
    (src / "broken.jpg").write_bytes(b"not a jpeg")
    _save(src / "thin" / "sliver.png", (5, 1000))      # letterbox_dims refuses: short side 1
    _save(src / "thin" / "line.png", (1, 1000))        # PIL's own ValueError: width 0
    assert SZ.standardize_tree(src, dst) == (0, 3)
    assert dst.is_dir() and not any(dst.iterdir())
    with pytest.raises(FileNotFoundError):
        SZ.standardize_tree(tmp_path / "absent", dst)
