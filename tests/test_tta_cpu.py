"""Host side of the test-time augmentation evaluation (training/tta.py, data/gpu_transforms.py):
the TTA Compose's parameter draws, the pair-count AUC formula, the metric assembly from the
device's counts vector and the clean-vs-TTA verdict.  No GPU."""
import dataclasses
import math

import numpy as np
import pytest
import torch
from sklearn.metrics import accuracy_score, confusion_matrix, f1_score, roc_auc_score

from data import gpu_transforms as GT
from training import tta as T


def _uniform(a, b, g):
    return float(torch.empty(1).uniform_(a, b, generator=g).item())


@pytest.mark.parametrize("spec", [GT.rgb_tta_transform, GT.thermal_tta_transform])
def test_tta_draw_sequence(spec):
    """test_time_augmentation.py:145-167 in Compose order: RandomRotation(15), the two flips, a
    bare RandomAffine(10, translate=(0.05, 0.05)) -- no RandomApply coin, no scale draw."""
    assert spec.order == "rotate_flip" and spec.size == (224, 224) and spec.affine_p is None
    g, h = torch.Generator().manual_seed(123), torch.Generator().manual_seed(123)
    for _ in range(20):
        p = GT.sample_params(spec, g)
        angle = _uniform(-15.0, 15.0, h)
        hflip = bool(torch.rand(1, generator=h) < 0.5)
        vflip = bool(torch.rand(1, generator=h) < 0.5)
        a = _uniform(-10.0, 10.0, h)
        tx = int(round(_uniform(-float(0.05 * 224), float(0.05 * 224), h)))
        ty = int(round(_uniform(-float(0.05 * 224), float(0.05 * 224), h)))
        assert (p.angle, p.hflip, p.vflip) == (angle, hflip, vflip)
        assert p.affine == (a, (tx, ty), 1.0, (0.0, 0.0)) and p.ops == []
        assert abs(tx) <= 11 and abs(ty) <= 11
    # both generators are in the same state: nothing else was drawn
    assert torch.equal(g.get_state(), h.get_state())


def test_tta_constants_carry_the_scripts_values():
    r, t = GT.rgb_tta_transform, GT.thermal_tta_transform
    for s in (r, t):
        assert (s.hflip_p, s.vflip_p, s.rotation, s.jitter) == (0.5, 0.5, 15, None)
        assert s.affine == (10, (0.05, 0.05), None) and s.random
    assert (r.mean, r.std) == (GT.IMAGENET_MEAN, GT.IMAGENET_STD)
    assert (t.mean, t.std) == (GT.THERMAL_MEAN, GT.THERMAL_STD)


@dataclasses.dataclass(frozen=True)
class _OldSpec:
    """TransformSpec as it was before `order` and the None conventions existed."""
    size: tuple = (224, 224)
    hflip_p: float = 0.0
    vflip_p: float = 0.0
    rotation: float = 0.0
    jitter: tuple = None
    jitter_p: float = 0.0
    affine: tuple = None
    affine_p: float = 0.0


def _old_sample(spec, g):
    """The draw sequence of the train scripts' Compose, restated: flips, rotation angle,
    RandomApply(ColorJitter), RandomApply(RandomAffine with a scale range)."""
    H, W = spec.size
    out = []
    if spec.hflip_p:
        out.append(bool(torch.rand(1, generator=g) < spec.hflip_p))
    if spec.vflip_p:
        out.append(bool(torch.rand(1, generator=g) < spec.vflip_p))
    if spec.rotation:
        out.append(_uniform(-float(spec.rotation), float(spec.rotation), g))
    if spec.jitter is not None and not (spec.jitter_p < torch.rand(1, generator=g)):
        out.append(torch.randperm(4, generator=g).tolist())
        out += [_uniform(max(0.0, 1 - v), 1 + v, g) for v in spec.jitter]
    if spec.affine is not None and not (spec.affine_p < torch.rand(1, generator=g)):
        deg, (tx, ty), (s0, s1) = spec.affine
        out.append(_uniform(-float(deg), float(deg), g))
        out.append(int(round(_uniform(-float(tx * W), float(tx * W), g))))
        out.append(int(round(_uniform(-float(ty * H), float(ty * H), g))))
        out.append(_uniform(s0, s1, g))
    return out


@pytest.mark.parametrize("spec", [GT.rgb_train_transform, GT.thermal_train_transform,
                                  GT.rgb_val_test_transform])
def test_train_spec_draws_unchanged(spec):
    """The same generator state after every sample with and without the new fields present, and
    the same values (the new fields default to the old behaviour)."""
    assert spec.order == "flip_rotate"
    old = _OldSpec(**{f.name: getattr(spec, f.name) for f in dataclasses.fields(_OldSpec)})
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for _ in range(40):
        p = GT.sample_params(spec, g)
        o = _old_sample(old, h)
        assert torch.equal(g.get_state(), h.get_state())
        got = ([p.hflip] if spec.hflip_p else []) + ([p.vflip] if spec.vflip_p else []) + \
              ([p.angle] if spec.rotation else [])
        if p.ops:
            got += [None] + [None] * 3  # order and factors: checked through the generator state
        if p.affine is not None:
            got += [p.affine[0], p.affine[1][0], p.affine[1][1], p.affine[2]]
        assert len(got) == len(o)
        assert all(a == b for a, b in zip(got, o) if a is not None)


def test_bad_order_is_refused():
    with pytest.raises(ValueError):
        GT.sample_params(GT.TransformSpec(rotation=5, order="rotate"))
    with pytest.raises(ValueError):
        GT.GpuPairLoader(None, 2, views=0)


def pair_count_auc(prob, labels):
    """(greater + ties / 2) / (pos * neg) over (label-1 i, label-0 j) pairs: the counts
    dfu_binary_eval_counts produces.  Returns (auc, greater, ties)."""
    prob, labels = np.asarray(prob), np.asarray(labels)
    p, q = prob[labels == 1][:, None], prob[labels == 0][None, :]
    greater, ties = int((p > q).sum()), int((p == q).sum())
    den = p.size * q.size
    return ((greater + 0.5 * ties) / den if den else float("nan")), greater, ties


@pytest.mark.parametrize("n,levels", [(2, 2), (50, 4), (257, 16), (1000, 16), (400, 0)])
def test_pair_count_auc_equals_sklearn(n, levels):
    rng = np.random.default_rng(n)
    labels = rng.integers(0, 2, n)
    labels[0], labels[1] = 0, 1
    prob = rng.random(n).astype(np.float32)
    if levels:
        prob = (np.floor(prob * levels) / levels).astype(np.float32)  # heavy ties
    auc, _, _ = pair_count_auc(prob, labels)
    assert abs(auc - roc_auc_score(labels, prob)) <= 1e-12


def _counts(pred, prob, labels):
    pred, labels = np.asarray(pred), np.asarray(labels)
    tn = int(((pred == 0) & (labels == 0)).sum())
    fp = int(((pred == 1) & (labels == 0)).sum())
    fn = int(((pred == 0) & (labels == 1)).sum())
    tp = int(((pred == 1) & (labels == 1)).sum())
    _, greater, ties = pair_count_auc(prob, labels)
    return [tn, fp, fn, tp, greater, ties]


@pytest.mark.parametrize("seed", range(4))
def test_metric_assembly_equals_sklearn(seed):
    rng = np.random.default_rng(seed)
    n = 60 + 17 * seed
    labels = rng.integers(0, 2, n)
    prob = (np.floor(rng.random(n) * 8) / 8).astype(np.float32)
    pred = (rng.random(n) < 0.3 + 0.4 * labels).astype(np.int64)
    r = T.metrics_from_counts(_counts(pred, prob, labels), pred, prob, labels)
    assert r["accuracy"] == accuracy_score(labels, pred)
    assert abs(r["f1"] - f1_score(labels, pred)) <= 1e-15
    assert abs(r["auc"] - roc_auc_score(labels, prob)) <= 1e-12
    cm = confusion_matrix(labels, pred)
    assert np.array_equal(r["confusion_matrix"], cm)
    tn, fp, fn, tp = cm.ravel()
    assert r["sensitivity"] == tp / (tp + fn) and r["specificity"] == tn / (tn + fp)
    assert set(r) == {"accuracy", "f1", "auc", "sensitivity", "specificity", "confusion_matrix",
                      "predictions", "probabilities", "labels"}
    assert np.array_equal(r["predictions"], pred) and np.array_equal(r["labels"], labels)
    assert np.array_equal(r["probabilities"], prob)


def test_metric_assembly_nan_cases():
    # only positives: no pairs and no negatives
    r = T.metrics_from_counts([0, 0, 1, 3, 0, 0], [0, 1, 1, 1], [.1, .9, .8, .7], [1, 1, 1, 1])
    assert math.isnan(r["auc"]) and math.isnan(r["specificity"])
    assert r["sensitivity"] == 0.75 and r["accuracy"] == 0.75 and r["f1"] == 6 / 7
    # only negatives, none predicted positive: F1 is sklearn's 0
    r = T.metrics_from_counts([3, 0, 0, 0, 0, 0], [0, 0, 0], [.1, .2, .3], [0, 0, 0])
    assert math.isnan(r["auc"]) and math.isnan(r["sensitivity"])
    assert r["specificity"] == 1.0 and r["accuracy"] == 1.0 and r["f1"] == 0.0
    # nothing at all
    r = T.metrics_from_counts([0] * 6, [], [], [])
    assert all(math.isnan(r[k]) for k in ("accuracy", "auc", "sensitivity", "specificity"))
    assert r["f1"] == 0.0 and r["confusion_matrix"].tolist() == [[0, 0], [0, 0]]


@pytest.mark.parametrize("clean,tta,verdict", [
    (0.90, 0.86, "ROBUST"), (0.90, 0.94, "ROBUST"),          # |drop| 0.04 on either side
    (0.90, 0.84, "MODERATE"), (0.80, 0.86, "MODERATE"),      # 0.06
    (0.90, 0.76, "MODERATE"),                                # 0.14
    (0.90, 0.74, "NOT ROBUST"), (0.70, 0.86, "NOT ROBUST"),  # 0.16
    (0.50, 0.50, "ROBUST"),
])
def test_compare_tta_verdict(clean, tta, verdict):
    c = {"accuracy": clean, "f1": 0.8}
    t = {"accuracy": tta, "f1": 0.7}
    r = T.compare_tta(c, t)
    assert r["verdict"] == verdict
    assert r["acc_drop"] == clean - tta and r["f1_drop"] == 0.8 - 0.7


def test_compare_tta_thresholds_are_strict():
    """The script's tests are `abs(acc_drop) < 0.05` and `< 0.15`: a drop of exactly the
    threshold falls into the next class."""
    assert T.compare_tta({"accuracy": 0.05, "f1": 0}, {"accuracy": 0.0, "f1": 0})["verdict"] == \
        "MODERATE"
    assert T.compare_tta({"accuracy": 0.15, "f1": 0}, {"accuracy": 0.0, "f1": 0})["verdict"] == \
        "NOT ROBUST"


def test_format_tta_comparison_reports_both_runs():
    labels = np.array([0, 0, 1, 1, 1, 0])
    prob = np.array([.1, .6, .7, .4, .9, .2], np.float32)
    clean = T.metrics_from_counts(_counts(prob > .5, prob, labels), prob > .5, prob, labels)
    pred2 = np.array([1, 1, 1, 0, 0, 0])
    tta = T.metrics_from_counts(_counts(pred2, prob, labels), pred2, prob, labels)
    text = T.format_tta_comparison(clean, tta, "Multimodal Fusion", num_tta=5)
    assert "Multimodal Fusion" in text and "NOT ROBUST" in text
    assert f"{clean['accuracy']:.4f}" in text and f"{tta['accuracy']:.4f}" in text
    assert f"{clean['auc']:.4f}" in text and str(tta["confusion_matrix"]) in text


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument validation is host code: it answers DFU_E_INVALID without a device."""
    from dfu_hip import _lib as L
    lib = L.load()
    buf = (np.zeros(64, np.int64)).ctypes.data  # a non-NULL pointer that is never dereferenced
    f3 = (L.c_float * 3)(0.5, 0.5, 0.5)
    views = lambda **k: lib.dfu_augment_views(  # noqa: E731
        k.get("img", buf), k.get("n_images", 1), buf, k.get("view_src", buf), k.get("n_views", 1),
        k.get("order", 0), k.get("H", 4), k.get("W", 4), f3, f3, buf, buf, None)
    for bad in (dict(order=2), dict(order=-1), dict(view_src=None), dict(img=None),
                dict(n_images=0), dict(n_views=0), dict(n_views=65536), dict(H=0), dict(W=-1)):
        assert views(**bad) == L.DFU_E_INVALID, bad
    assert views(order=2) == L.DFU_E_INVALID and b"order 2" in lib.dfu_last_error_string()
    for C in (0, 3, -1):
        assert lib.dfu_tta_reduce(buf, 1, 1, C, buf, buf, None) == L.DFU_E_INVALID
    assert lib.dfu_tta_reduce(None, 1, 1, 1, buf, buf, None) == L.DFU_E_INVALID
    assert lib.dfu_tta_reduce(buf, 0, 1, 1, buf, buf, None) == L.DFU_E_INVALID
    assert lib.dfu_tta_reduce(buf, 1, 0, 2, buf, buf, None) == L.DFU_E_INVALID
    assert lib.dfu_binary_eval_counts(buf, buf, buf, 0, buf, None) == L.DFU_E_INVALID
    assert lib.dfu_binary_eval_counts(buf, buf, buf, 1 << 24, buf, None) == L.DFU_E_INVALID
    assert lib.dfu_binary_eval_counts(buf, None, buf, 4, buf, None) == L.DFU_E_INVALID
    assert lib.dfu_binary_eval_counts(buf, buf, buf, 4, None, None) == L.DFU_E_INVALID
