"""Extended medical metrics evaluation on the GPU (notebooks/extended_metrics.py):
  * dfu_binary_curve (ops.binary_curve) against a numpy restatement of scikit-learn's
    _binary_clf_curve and against the recorded fixtures, exact integers and thresholds;
  * its validity rules, and the entries it must leave untouched;
  * training.metrics.evaluate_extended end to end, with the fusion head and the fusion model."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import data_inputs as DI  # noqa: E402

import metrics_ref as MR  # noqa: E402
from data import gpu_transforms as GT  # noqa: E402
from data import multimodal as MM  # noqa: E402
from dfu_hip import ops  # noqa: E402
from training import metrics as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = MR.load_cases()
GUARD = 64
POISON_F, POISON_I = -7.5, -123456789


def run_curve(prob, labels):
    """ops.binary_curve into poisoned buffers of n + GUARD entries.  Returns (thresholds[:K],
    tps[:K], fps[:K]) on the host after checking that every entry at index >= K, the guard
    included, is untouched."""
    prob = np.asarray(prob, np.float32)
    labels = np.asarray(labels, np.int64)
    n = prob.shape[0]
    out = (torch.full((n + GUARD,), POISON_F, dtype=torch.float32, device=DEV),
           torch.full((n + GUARD,), POISON_I, dtype=torch.int64, device=DEV),
           torch.full((n + GUARD,), POISON_I, dtype=torch.int64, device=DEV))
    thr, tps, fps, k = ops.binary_curve(torch.from_numpy(prob).to(DEV),
                                        torch.from_numpy(labels).to(DEV), out=out)
    assert thr.data_ptr() == out[0].data_ptr() and k.dtype == torch.int32 and k.shape == (1,)
    assert all(t.is_cuda for t in (thr, tps, fps, k))
    K = int(k.item())
    assert 0 <= K <= n
    thr, tps, fps = thr.cpu().numpy(), tps.cpu().numpy(), fps.cpu().numpy()
    assert (thr[K:] == POISON_F).all() and (tps[K:] == POISON_I).all() and \
        (fps[K:] == POISON_I).all(), "entries at index >= K were written"
    return thr[:K], tps[:K], fps[:K]


def check_curve(prob, labels, want=None):
    got = run_curve(prob, labels)
    want = MR.clf_curve_ref(labels, prob) if want is None else want
    assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]))
    for g, w, what in zip(got, want, ("thresholds", "tps", "fps")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    return got


def _scores(n, sixteenths, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 2, n)
    prob = np.clip(rng.normal(0.4 + 0.2 * labels, 0.25), 0, 1).astype(np.float32)
    if sixteenths:
        prob = (np.round(prob * 16) / 16).astype(np.float32)
    return prob, labels


# the edges of the 256-sample tile and of the grid; n = 1000 continuous and in sixteenths
@pytest.mark.parametrize("n,sixteenths", [(1, False), (2, False), (255, False), (256, True),
                                          (257, False), (513, True), (1000, False),
                                          (1000, True)])
def test_binary_curve_against_numpy(n, sixteenths):
    prob, labels = _scores(n, sixteenths, 10 * n + sixteenths)
    thr, tps, fps = check_curve(prob, labels)
    assert (np.diff(thr) < 0).all()  # strictly descending
    assert tps[-1] == (labels == 1).sum() and fps[-1] == (labels == 0).sum()
    if sixteenths and n > 100:
        assert len(thr) <= 17
    # the wrapper's own buffers: same answer
    t2, p2, f2, k = ops.binary_curve(torch.from_numpy(prob).to(DEV),
                                     torch.from_numpy(labels).to(DEV))
    K = int(k.item())
    assert t2.shape == p2.shape == f2.shape == (n,) and K == len(thr)
    assert np.array_equal(t2[:K].cpu().numpy(), thr) and np.array_equal(p2[:K].cpu().numpy(), tps)
    assert np.array_equal(f2[:K].cpu().numpy(), fps)


@pytest.mark.parametrize("name", sorted(CASES))
def test_binary_curve_against_the_fixtures(name):
    c = CASES[name]["binary_clf_curve"]
    want = (np.array(c["thresholds"], np.float32), np.array(c["tps"], np.int64),
            np.array(c["fps"], np.int64))
    check_curve(CASES[name]["y_probs"], CASES[name]["y_true"], want)


def test_validity_rules():
    """Other labels and a NaN score are left out of every count and are no threshold; -0.0 and
    0.0 are one score."""
    prob, labels = _scores(300, True, 3)
    labels[[5, 17, 256, 299]] = (2, -1, 7, 1 << 40)
    prob[40] = np.nan
    prob[[0, 100, 257]] = (-0.0, 0.0, -0.0)
    prob[[1, 101]] = (0.0, -0.0)
    labels[[0, 100, 257, 1, 101]] = (1, 0, 1, 0, 2)
    thr, tps, fps = check_curve(prob, labels)
    ok = ((labels == 0) | (labels == 1)) & ~np.isnan(prob)
    assert ok.sum() == 300 - 6
    assert tps[-1] == (labels[ok] == 1).sum() and fps[-1] == (labels[ok] == 0).sum()
    assert (thr == 0).sum() == 1 and thr[-1] == 0  # one zero threshold, the lowest score
    assert not np.isnan(thr).any()
    # a score held only by invalid samples is no threshold
    prob2 = np.array([0.5, 0.9, 0.25, 0.9, np.nan], np.float32)
    labels2 = np.array([1, 3, 0, -2, 1])
    thr, tps, fps = check_curve(prob2, labels2)
    assert thr.tolist() == [0.5, 0.25] and tps.tolist() == [1, 1] and fps.tolist() == [0, 1]


@pytest.mark.parametrize("n", [1, 300])
def test_single_class_and_no_valid_sample(n):
    prob, _ = _scores(n, True, n)
    thr, tps, fps = check_curve(prob, np.ones(n, np.int64))
    assert (fps == 0).all() and tps[-1] == n
    thr, tps, fps = check_curve(prob, np.zeros(n, np.int64))
    assert (tps == 0).all() and fps[-1] == n
    for labels in (np.full(n, 2), np.full(n, -1)):
        assert len(run_curve(prob, labels)[0]) == 0  # K = 0, nothing written
    assert len(run_curve(np.full(n, np.nan, np.float32), np.ones(n, np.int64))[0]) == 0


def test_empty_input_launches_nothing():
    thr, tps, fps, k = ops.binary_curve(torch.empty(0, device=DEV),
                                        torch.empty(0, dtype=torch.int64, device=DEV))
    assert thr.shape == tps.shape == fps.shape == (0,) and k.tolist() == [0]
    assert thr.dtype == torch.float32 and tps.dtype == fps.dtype == torch.int64
    with pytest.raises(ValueError):
        ops.binary_curve(torch.zeros(4, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------ end to end
def _host_metrics(res):
    """medical_metrics recomputed on the host from the returned per-sample arrays."""
    y, d, p = res["y_true"], res["y_pred"], res["y_probs"]
    return M.medical_metrics(MR.counts_ref(y, d, p), MR.clf_curve_ref(y, p))


def _same_metrics(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "confusion_matrix":
            assert np.array_equal(a[k], b[k])
        elif isinstance(a[k], float) and math.isnan(a[k]):
            assert math.isnan(b[k]), k
        else:
            assert a[k] == b[k], k


class _FeatureLoader:
    """Batches of ([B, 2816] features, [B] labels) on the device."""

    def __init__(self, feats, labels, sizes):
        self.batches, s = [], 0
        for b in sizes:
            self.batches.append((feats[s:s + b], labels[s:s + b]))
            s += b

    def __iter__(self):
        return iter(self.batches)


def _head_forward(m, f):
    return m(f[:, :2048].contiguous(), f[:, 2048:].contiguous())


@pytest.mark.parametrize("num_classes", [2, 1])
def test_evaluate_extended_with_the_fusion_head(num_classes, tmp_path):
    from models.fusion import MLPFusion
    torch.manual_seed(num_classes)
    head = MLPFusion(num_classes=num_classes).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(21, 2816, generator=g).to(DEV)
    labels = torch.randint(0, 2, (21,), generator=g)
    labels[:2] = torch.tensor([0, 1])
    loader = _FeatureLoader(feats, labels.to(DEV), (8, 8, 5))
    path = tmp_path / "results.pt"
    res = M.evaluate_extended(head, loader, forward=_head_forward, results_path=str(path))
    assert not head.training
    assert set(res) == {"y_true", "y_pred", "y_probs", "metrics"}
    assert res["y_true"].tolist() == labels.tolist() and res["y_true"].dtype == np.int64
    assert res["y_probs"].dtype == np.float32 and res["y_probs"].shape == (21,)
    # the per-sample arrays are ops.tta_reduce's of the whole set
    with torch.no_grad():
        per_batch = [ops.tta_reduce(_head_forward(head, f), 1) for f, _ in loader]
    assert np.array_equal(res["y_probs"], torch.cat([p for p, _ in per_batch]).cpu().numpy())
    assert np.array_equal(res["y_pred"], torch.cat([d for _, d in per_batch]).cpu().numpy())
    assert 0 < res["y_probs"].min() and res["y_probs"].max() < 1
    m = res["metrics"]
    _same_metrics(m, _host_metrics(res))
    assert m["tn"] + m["fp"] + m["fn"] + m["tp"] == 21 and not math.isnan(m["auc_roc"])
    saved = torch.load(str(path), weights_only=False)
    assert set(saved) == set(res)
    for k in ("y_true", "y_pred", "y_probs"):
        assert np.array_equal(saved[k], res[k]) and saved[k].dtype == res[k].dtype
    _same_metrics(saved["metrics"], m)


def test_evaluate_extended_refuses_nan_and_other_widths():
    feats = torch.zeros(4, 2816, device=DEV)
    labels = torch.tensor([0, 1, 0, 1], device=DEV)
    loader = _FeatureLoader(feats, labels, (4,))
    nan_logits = lambda m, f: torch.full((f.shape[0], 2), float("nan"), device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="Input contains NaN"):
        M.evaluate_extended(torch.nn.Identity(), loader, forward=nan_logits)
    with pytest.raises(ValueError):
        M.evaluate_extended(torch.nn.Identity(), loader,
                            forward=lambda m, f: torch.zeros(f.shape[0], 3, device=DEV))


def test_fusion_model_run_and_the_three_model_driver(tmp_path):
    from models.fusion import MultimodalFusionModel
    from training import loop
    from training import tta as T
    rgb_dir, th_dir = DI.build_tree(str(tmp_path / "data"))
    random.seed(42)
    ds = MM.MultimodalDataset(rgb_dir, th_dir, "val", verbose=False)
    assert len(ds) == 8 and sorted(set(ds.labels())) == [0, 1]
    torch.manual_seed(0)
    model = MultimodalFusionModel(num_classes=2, dropout=0.7).to(DEV)
    entries = {"Multimodal": (model, GT.GpuPairLoader(ds, 3, num_threads=2), None)}
    out = tmp_path / "extended_metrics"
    try:
        import matplotlib  # noqa: F401
        plots = True
    except ImportError:
        plots = False
    all_results, text = M.run_extended_evaluation(entries, str(out), plots=plots)
    assert list(all_results) == ["Multimodal"] and not model.training
    m = all_results["Multimodal"]
    assert "EXTENDED MEDICAL METRICS: Multimodal" in text and "SUMMARY COMPARISON" in text
    assert f"{m['f1']:.4f}" in text and f"{m['auc_roc']:.4f}" in text
    figures = ["confusion_matrix_Multimodal.png", "pr_curve_Multimodal.png",
               "roc_curve_Multimodal.png"] if plots else []
    assert sorted(os.listdir(str(out / "Multimodal"))) == sorted(figures + ["results.pt"])
    res = torch.load(str(out / "Multimodal" / "results.pt"), weights_only=False)
    assert res["y_true"].tolist() == ds.labels()
    _same_metrics(res["metrics"], m)
    _same_metrics(m, _host_metrics(res))
    ref = loop.metrics_from_confusion(m["confusion_matrix"], 0.0, 1)
    assert m["accuracy"] == ref["acc"] and m["f1"] == ref["f1"]
    counts = ops.binary_eval_counts(*(torch.from_numpy(res[k]).to(DEV)
                                      for k in ("y_probs", "y_pred", "y_true"))).tolist()
    assert counts == MR.counts_ref(res["y_true"], res["y_pred"], res["y_probs"])
    auc = T.metrics_from_counts(counts, res["y_pred"], res["y_probs"], res["y_true"])["auc"]
    assert abs(m["auc_roc"] - auc) <= 1e-12
