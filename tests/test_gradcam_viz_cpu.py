"""The host side of the Grad-CAM visualisation pass (training/gradcam_viz.py, the tables of
dfu_hip.ops): tap tables, the colour table, sample selection, the figures, the file tree of
run_gradcam_visualization, and the numpy restatement (gradcam_viz_ref.py) against itself.  No
GPU."""
import os

import numpy as np
import pytest

import gradcam_viz_ref as VR
from dfu_hip import ops
from training import gradcam_viz as V


# ------------------------------------------------------------------------------ linear_taps
def test_linear_taps_7_to_224():
    i0, i1, w = ops.linear_taps(7, 224)
    assert i0.dtype == i1.dtype == np.int32 and w.dtype == np.float32
    assert i0.shape == i1.shape == w.shape == (224,)
    assert (w[:16] == 0).all() and (w[-16:] == 0).all()
    assert (i0[:16] == 0).all() and (i0[-16:] == 6).all() and (i1[-16:] == 6).all()
    assert w[16] == np.float32(0.015625) and i0[16] == 0 and i1[16] == 1
    assert w[207] == np.float32(0.984375) and i0[207] == 5 and i1[207] == 6
    # 32 output pixels per source pixel: the weight climbs by 1/32
    assert np.array_equal(w[16:48], (np.arange(32) * 2 + 1) / np.float32(64))


@pytest.mark.parametrize("n_in,n_out", [(1, 5), (5, 5), (3, 29), (224, 224), (7, 224), (5, 37),
                                        (29, 3)])
def test_linear_taps_against_the_restatement(n_in, n_out):
    got, want = ops.linear_taps(n_in, n_out), VR.taps_ref(n_in, n_out)
    for g, r in zip(got, want):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    i0, i1, w = got
    if n_in == 1:
        assert not i0.any() and not i1.any() and not w.any()
    if n_in == n_out:  # the identity (the ViT saliency map is already 224 x 224)
        assert np.array_equal(i0, np.arange(n_in)) and not w.any()
        assert np.array_equal(i1, np.minimum(np.arange(n_in) + 1, n_in - 1))


def test_linear_taps_stay_in_range():
    for n_in in range(1, 33):
        for n_out in range(1, 33):
            i0, i1, w = ops.linear_taps(n_in, n_out)
            assert i0.min() >= 0 and i1.max() <= n_in - 1 and (i0 <= i1).all()
            assert (i1 - i0 <= 1).all()
            assert (w >= 0).all() and (w < 1).all()
            assert np.array_equal(i0, VR.taps_ref(n_in, n_out)[0])
    with pytest.raises(ValueError):
        ops.linear_taps(0, 4)


# ---------------------------------------------------------------------------------- jet_lut
def test_jet_lut_anchors_and_ramps():
    lut = ops.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert np.array_equal(lut, VR.jet_ref())
    for i, rgb in ((0, (0, 0, 128)), (32, (0, 0, 255)), (64, (0, 128, 255)),
                   (128, (130, 255, 126)), (191, (255, 128, 0)), (255, (128, 0, 0))):
        assert tuple(lut[i]) == rgb, i
    # per channel: 0, a rising ramp, 255, a falling ramp, 0, around the centre 255 c / 4
    for k, centre in enumerate((191.25, 127.5, 63.75)):
        ch = lut[:, k].astype(int)
        up = ch[:int(centre) + 1]
        down = ch[int(centre) + 1:]
        assert (np.diff(up) >= 0).all() and (np.diff(down) <= 0).all()
        rising = up[(up > 0) & (up < 255)]
        falling = down[(down > 0) & (down < 255)]
        assert (np.diff(rising) > 0).all() and (np.diff(falling) < 0).all()
        assert ch.max() == 255
    assert lut[:, 0].min() == 0 and lut[:, 1].min() == 0 and lut[:, 2].min() == 0


# --------------------------------------------------------------------------- select_samples
def test_select_samples():
    # all of one class first (the single-modality datasets' order)
    labels = [0] * 8 + [1] * 7
    assert V.select_samples(labels) == [(i, 0, i) for i in range(5)] + \
        [(8 + i, 1, i) for i in range(5)]
    # fewer than five of a class
    labels = [0, 0, 0] + [1] * 9
    assert V.select_samples(labels) == [(0, 0, 0), (1, 0, 1), (2, 0, 2)] + \
        [(3 + i, 1, i) for i in range(5)]
    assert V.select_samples([1, 1]) == [(0, 1, 0), (1, 1, 1)]
    assert V.select_samples([]) == []
    # interleaved (the shuffled pair dataset): dataset order is kept, counters per class
    labels = [1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0]
    got = V.select_samples(labels)
    assert got == [(0, 1, 0), (1, 0, 0), (2, 1, 1), (3, 1, 2), (4, 0, 1), (5, 1, 3), (6, 1, 4),
                   (8, 0, 2), (9, 0, 3), (10, 0, 4)]
    assert [g[0] for g in got] == sorted(g[0] for g in got)
    assert V.select_samples(labels, num_healthy=1, num_ulcer=2) == [(0, 1, 0), (1, 0, 0),
                                                                    (2, 1, 1)]
    # tensors of labels count as their values
    import torch
    assert V.select_samples(torch.tensor([1, 0, 0])) == [(0, 1, 0), (1, 0, 0), (2, 0, 1)]


# ---------------------------------------------------------------------------------- figures
def _sample(kind, prediction, confidence, seed=0):
    rng = np.random.default_rng(seed)
    pic = lambda: rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)  # noqa: E731
    s = {"prediction": prediction, "confidence": confidence}
    for suffix in (("_rgb", "_thermal") if kind == "multimodal" else ("",)):
        s["cam" + suffix] = rng.random((7, 7), dtype=np.float32)
        for name in ("image", "heatmap", "overlay"):
            s[name + suffix] = pic()
    return s


def _titles(fig):
    return [ax.get_title() for ax in fig.axes]


@pytest.mark.parametrize("kind,original,suptitle", [
    ("rgb_only", "Original RGB Image", "RGB-Only Model Grad-CAM"),
    ("thermal_only", "Original Thermal Image", "Thermal-Only Model Grad-CAM")])
def test_single_modality_figures(kind, original, suptitle, tmp_path):
    pytest.importorskip("matplotlib")
    from PIL import Image
    for pred, conf, text in ((1, 0.98765, "Overlay\nPred: Ulcer (0.988)"),
                             (0, 0.5, "Overlay\nPred: Healthy (0.500)")):
        fig = V.FIGURES[kind](_sample(kind, pred, conf))
        assert len(fig.axes) == 3 and tuple(fig.get_size_inches()) == (15, 5)
        assert _titles(fig) == [original, "Grad-CAM Heatmap", text]
        assert fig.get_suptitle() == suptitle
        assert not any(ax.axison for ax in fig.axes)
        assert all(len(ax.images) == 1 for ax in fig.axes)
        path = tmp_path / f"{kind}_{pred}.png"
        fig.savefig(str(path), dpi=150, bbox_inches="tight")
        with Image.open(str(path)) as im:
            assert im.format == "PNG" and im.size[0] > 1000 and im.size[1] > 300


def test_multimodal_figure(tmp_path):
    pytest.importorskip("matplotlib")
    from PIL import Image
    for pred, conf, text in ((1, 0.75049, "Ulcer (Confidence: 0.750)"),
                             (0, 0.9996, "Healthy (Confidence: 1.000)")):
        fig = V.figure_multimodal(_sample("multimodal", pred, conf))
        assert len(fig.axes) == 6 and tuple(fig.get_size_inches()) == (18, 10)
        assert _titles(fig) == ["RGB Image", "RGB Grad-CAM", "RGB Overlay", "Thermal Image",
                                "Thermal Grad-CAM", "Thermal Overlay"]
        assert fig.get_suptitle() == f"Multimodal Fusion Grad-CAM\nPrediction: {text}"
        assert not any(ax.axison for ax in fig.axes)
        path = tmp_path / f"mm_{pred}.png"
        fig.savefig(str(path), dpi=150, bbox_inches="tight")
        with Image.open(str(path)) as im:
            assert im.format == "PNG" and im.size[0] > 1000 and im.size[1] > 600


def test_sample_at():
    batch = {"prediction": np.array([0, 1]), "confidence": np.array([0.25, 0.75], np.float32),
             "image": np.zeros((2, 4, 4, 3), np.uint8), "cam": np.ones((2, 7, 7), np.float32)}
    s = V.sample_at(batch, 1)
    assert s["prediction"] == 1 and isinstance(s["prediction"], int)
    assert s["confidence"] == 0.75 and isinstance(s["confidence"], float)
    assert s["image"].shape == (4, 4, 3) and s["cam"].shape == (7, 7)


# ------------------------------------------------------------------------------------ main
class _Labels:
    """A dataset as run_gradcam_visualization sees it: labels as a list (the single-modality
    sets) or a method (the pair set)."""

    def __init__(self, labels, method=False):
        self.labels = (lambda: list(labels)) if method else list(labels)


def _stub_pass(monkeypatch, calls):
    """visualize_batch replaced by a stub that returns synthetic pictures, and load_samples (the
    decode and the HIP preprocessing in front of it) by one that passes the indices through."""
    def load_samples(dataset, kind, indices, device="cuda"):
        return (list(indices), None) if kind == "rgb_only" else (
            (None, list(indices)) if kind == "thermal_only" else (list(indices), list(indices)))

    def visualize_batch(model, kind, rgb=None, thermal=None):
        idx = rgb if rgb is not None else thermal
        calls.append((model, kind, list(idx)))
        B = len(idx)
        one = _sample(kind, 0, 0.5)
        out = {k: np.stack([v] * B) for k, v in one.items() if k not in ("prediction",
                                                                         "confidence")}
        out["prediction"] = np.arange(B) % 2
        out["confidence"] = np.linspace(0.5, 1, B, dtype=np.float32)
        return out

    monkeypatch.setattr(V, "load_samples", load_samples)
    monkeypatch.setattr(V, "visualize_batch", visualize_batch)


def test_run_writes_the_tree(monkeypatch, tmp_path, capsys):
    pytest.importorskip("matplotlib")
    from PIL import Image
    calls = []
    _stub_pass(monkeypatch, calls)
    single = [0] * 6 + [1] * 7
    mixed = [1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1]
    datasets = {"rgb_only": _Labels(single), "thermal_only": _Labels(single),
                "multimodal": _Labels(mixed, method=True)}
    m_rgb, m_th, m_mm = object(), object(), object()  # models, not checkpoint paths
    models = {"rgb_only": m_rgb, "thermal_only": m_th, "multimodal": m_mm}
    out = tmp_path / "grad_cam_visualizations"
    written = V.run_gradcam_visualization(models, datasets, str(out), device="cpu")
    names = [f"healthy_{i:02d}.png" for i in range(5)] + [f"ulcer_{i:02d}.png" for i in range(5)]
    assert sorted(os.listdir(str(out))) == ["multimodal", "rgb_only", "thermal_only"]
    for kind in V.KINDS:
        assert sorted(os.listdir(str(out / kind))) == names
    assert len(written) == 30 and all(os.path.isfile(p) for p in written)
    assert [os.path.relpath(p, str(out)) for p in written[:10]] == \
        [os.path.join("rgb_only", n) for n in names]
    with Image.open(written[0]) as im:
        assert im.format == "PNG"
    # one pass per model, over the selected samples in dataset order
    assert calls == [(m_rgb, "rgb_only", [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]),
                     (m_th, "thermal_only", [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]),
                     (m_mm, "multimodal", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])]
    # the pair set's files follow its interleaved order: sample 0 is ulcer_00, sample 1 healthy_00
    mm = [os.path.basename(p) for p in written[20:]]
    assert mm[:5] == ["ulcer_00.png", "healthy_00.png", "healthy_01.png", "ulcer_01.png",
                      "ulcer_02.png"]
    text = capsys.readouterr().out
    assert "GRAD-CAM VISUALIZATION FOR DFU MODELS" in text
    assert "Will visualize 5 healthy + 5 ulcer samples per model" in text
    assert "VISUALIZING RGB-ONLY MODEL" in text and "VISUALIZING MULTIMODAL FUSION MODEL" in text
    assert text.count("Saved healthy_00.png") == 3
    assert "Saved 10 Thermal-only visualizations (5 healthy, 5 ulcer)" in text
    assert "GRAD-CAM VISUALIZATION COMPLETE" in text and "Checkpoint not found" not in text


def test_run_stops_short_and_skips(monkeypatch, tmp_path, capsys):
    pytest.importorskip("matplotlib")
    calls = []
    _stub_pass(monkeypatch, calls)
    datasets = {k: _Labels([0, 0, 0] + [1] * 6) for k in V.KINDS}
    missing = tmp_path / "checkpoints_thermal_only" / "best_model.pt"
    m_rgb = object()
    models = {"rgb_only": m_rgb, "thermal_only": str(missing)}  # no fusion entry at all
    out = tmp_path / "out"
    written = V.run_gradcam_visualization(models, datasets, str(out), device="cpu")
    assert sorted(os.listdir(str(out))) == ["rgb_only"]
    assert sorted(os.listdir(str(out / "rgb_only"))) == \
        ["healthy_00.png", "healthy_01.png", "healthy_02.png"] + \
        [f"ulcer_{i:02d}.png" for i in range(5)]
    assert len(written) == 8 and calls == [(m_rgb, "rgb_only", [0, 1, 2, 3, 4, 5, 6, 7])]
    text = capsys.readouterr().out
    assert f"Checkpoint not found: {missing}" in text
    assert text.count("Checkpoint not found") == 2
    assert "Saved 8 RGB-only visualizations (3 healthy, 5 ulcer)" in text
    # other sample counts
    written = V.run_gradcam_visualization({"rgb_only": m_rgb}, datasets, str(tmp_path / "two"),
                                          num_healthy=1, num_ulcer=2, device="cpu")
    assert [os.path.basename(p) for p in written] == ["healthy_00.png", "ulcer_00.png",
                                                      "ulcer_01.png"]


# ------------------------------------------------------------- the restatement against itself
def test_blend_at_one_half_is_the_rounded_mean():
    """At alpha = 0.5 both products are exact, so the blend is (image + heat) / 2 rounded to
    nearest, ties to the even neighbour: all 256 x 256 value pairs."""
    image, heat = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8),
                              indexing="ij")
    got = VR.blend_ref(image, heat, 0.5).astype(int)
    s = image.astype(int) + heat
    up = (s + 1) // 2
    ties = s % 2 == 1
    assert np.array_equal(got[~ties], up[~ties]) and np.array_equal(got[~ties], s[~ties] // 2)
    even = np.where(up % 2 == 0, up, up - 1)
    assert np.array_equal(got[ties], even[ties]) and (got[ties] % 2 == 0).all()
    assert ties.sum() == 256 * 128
    # the ends of alpha pick one side exactly
    assert np.array_equal(VR.blend_ref(image, heat, 0.0), image)
    assert np.array_equal(VR.blend_ref(image, heat, 1.0), heat)


def test_restatement_pieces():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(2, 3, 6, 5)).astype(np.float32)
    x[1] = 0.25  # a constant image: zeros, not the script's NaN
    image = VR.image_ref(x)
    assert image.shape == (2, 6, 5, 3) and image.dtype == np.uint8
    assert image[0].min() == 0 and image[0].max() == 255 and not image[1].any()
    # a map already at the image's size passes through the identity taps unchanged
    cam = rng.random((2, 6, 5), dtype=np.float32)
    assert np.array_equal(VR.resize_ref(cam, 6, 5), cam)
    # a constant map stays constant under any resize (the weights sum to one in fp32)
    for value in (0.0, 0.5, 1.0):
        assert (VR.resize_ref(np.full((1, 7, 7), value, np.float32), 224, 224) == value).all()
    heat = VR.heatmap_ref(np.array([[[0.0, 1.0]]], np.float32), 1, 2)
    assert heat[0, 0, 0].tolist() == [0, 0, 128] and heat[0, 0, 1].tolist() == [128, 0, 0]
    # every uint8 u comes back from the (0, 255) scaling that overlay_gradcam_on_image uses
    u = np.arange(256, dtype=np.float32).reshape(1, 1, 16, 16).repeat(3, 1) + np.float32(0.5)
    back = VR.image_ref(u, np.array([[0, 255]], np.float32))
    assert np.array_equal(back[0, :, :, 0].ravel(), np.arange(256))


# ------------------------------------------------------------------- the C entry points
def test_c_entry_points_refuse_bad_arguments():
    """DFU_CHECK_ARG on every argument: a refused call returns DFU_E_INVALID before any launch
    (so no GPU is needed) and leaves its reason in dfu_last_error_string."""
    import ctypes

    from dfu_hip import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(64)  # a non-null address; a refused call never reads it
    p = ctypes.addressof(buf)

    def refused(rc, word):
        assert rc == L.DFU_E_INVALID
        assert word in lib.dfu_last_error_string().decode()

    refused(lib.dfu_image_minmax(None, 1, 4, p, None), "dfu_image_minmax")
    refused(lib.dfu_image_minmax(p, 1, 4, None, None), "dfu_image_minmax")
    for B, n in ((0, 4), (-1, 4), (65536, 4), (1, 0), (1, -3)):
        refused(lib.dfu_image_minmax(p, B, n, p, None), f"B = {B}, n = {n}")
    good = [p, p, p, 1, 8, 8, 2, 2, p, p, p, p, p, p, p, 0.5, p, p, p, None]
    for k in (0, 1, 2, 8, 9, 10, 11, 12, 13, 14, 16, 17, 18):  # every pointer but the stream
        args = list(good)
        args[k] = None
        refused(lib.dfu_cam_overlay(*args), "dfu_cam_overlay: null")
    for k in (3, 4, 5, 6, 7):                                   # B, H, W, h, w
        for bad in (0, -2):
            args = list(good)
            args[k] = bad
            refused(lib.dfu_cam_overlay(*args), "bad shape")
    args = list(good)
    args[3:6] = [1 << 11, 1 << 10, 1 << 10]                     # B * H * W * 3 >= 2^31
    refused(lib.dfu_cam_overlay(*args), "below 2^31")
    args = list(good)
    args[3], args[6], args[7] = 2, 1 << 15, 1 << 15             # B * h * w >= 2^31
    refused(lib.dfu_cam_overlay(*args), "below 2^31")
