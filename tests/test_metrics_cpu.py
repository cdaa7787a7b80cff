"""Host side of the extended medical metrics evaluation (training/metrics.py) against the
reference's MedicalMetricsCalculator and scikit-learn 1.7.2 as recorded in
tests/golden/extended_metrics.json (tools/gen_metrics_golden.py): the formulas, the two curves,
the report text, the plots and the argument checks of the binding.  No GPU, no scikit-learn."""
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR
from dfu_hip import _lib as L
from dfu_hip import ops
from training import metrics as M

CASES = MR.load_cases()
NAMES = sorted(CASES)
INT_KEYS = ("tn", "fp", "fn", "tp")
FLOAT_KEYS = ("accuracy", "precision", "recall", "f1", "sensitivity", "specificity", "ppv", "npv",
              "fpr", "fnr", "auc_roc", "auc_pr", "mcc", "kappa", "balanced_accuracy",
              "f_harmonic")
# fp64 arithmetic on exact integers, values in [-1, 1]; the longest sum is a 600-term trapezoid,
# about 600 * 1.1e-16
TOL = 1e-12


def _curve(case):
    c = case["binary_clf_curve"]
    return (np.array(c["thresholds"], np.float32), np.array(c["tps"], np.int64),
            np.array(c["fps"], np.int64))


def _metrics(case):
    return M.medical_metrics(MR.counts_ref(case["y_true"], case["y_pred"], case["y_probs"]),
                             _curve(case))


def test_fixture_holds_the_cases_of_the_issue():
    assert len(CASES) == 8
    sizes = sorted(len(c["y_true"]) for c in CASES.values())
    assert sizes == [2, 7, 30, 40, 64, 64, 257, 600]
    assert len(CASES["n30_every_score_identical"]["binary_clf_curve"]["tps"]) == 1
    assert not any(CASES["n40_every_prediction_0"]["y_pred"])
    assert CASES["n64_fully_inverted"]["metrics"]["auc_roc"] == 0.0
    assert CASES["n64_perfect_separation"]["metrics"]["auc_roc"] == 1.0
    for c in CASES.values():  # fp32 values, held exactly
        p = np.array(c["y_probs"])
        assert np.array_equal(p, p.astype(np.float32).astype(np.float64))
        # the numpy restatement the GPU tests compare with is the recorded curve
        t, tps, fps = MR.clf_curve_ref(c["y_true"], c["y_probs"])
        rt, rtps, rfps = _curve(c)
        assert np.array_equal(t, rt) and np.array_equal(tps, rtps) and np.array_equal(fps, rfps)


@pytest.mark.parametrize("name", NAMES)
def test_formulas_match_the_reference_calculator(name):
    case = CASES[name]
    want, got = case["metrics"], _metrics(case)
    assert set(got) == set(want)
    for k in INT_KEYS:
        assert isinstance(got[k], int) and got[k] == want[k], k
    assert got["confusion_matrix"].dtype == np.int64
    assert got["confusion_matrix"].tolist() == want["confusion_matrix"]
    assert got["classification_report"] == want["classification_report"]
    for k in FLOAT_KEYS:
        d = abs(got[k] - want[k])
        print(f"[{name}] {k}: {got[k]!r} vs {want[k]!r} (|d| = {d:.1e})")
        assert d <= TOL, k


@pytest.mark.parametrize("name", NAMES)
def test_curves_match_sklearn(name):
    case = CASES[name]
    fpr, tpr, thr = M.roc_curve(_curve(case))
    want = case["roc_curve"]
    assert len(fpr) == len(tpr) == len(thr) == len(want["thresholds"])
    assert thr[0] == math.inf and (fpr[0], tpr[0]) == (0.0, 0.0)
    assert np.array_equal(thr, np.array(want["thresholds"]))
    assert np.abs(fpr - np.array(want["fpr"])).max() <= TOL
    assert np.abs(tpr - np.array(want["tpr"])).max() <= TOL

    precision, recall, thr = M.precision_recall_curve(_curve(case))
    want = case["precision_recall_curve"]
    assert len(precision) == len(recall) == len(thr) + 1 == len(want["precision"])
    assert (precision[-1], recall[-1]) == (1.0, 0.0)
    assert np.array_equal(thr, np.array(want["thresholds"]))
    assert np.abs(precision - np.array(want["precision"])).max() <= TOL
    assert np.abs(recall - np.array(want["recall"])).max() <= TOL


@pytest.mark.parametrize("name", NAMES)
def test_auc_roc_equals_the_pair_count_auc(name):
    case = CASES[name]
    tn, fp, fn, tp, greater, ties = MR.counts_ref(case["y_true"], case["y_pred"],
                                                  case["y_probs"])
    auc = (greater + ties / 2) / ((fn + tp) * (tn + fp))
    assert abs(_metrics(case)["auc_roc"] - auc) <= TOL


def test_no_curve_gives_none():
    m = M.medical_metrics([3, 1, 2, 4, 0, 0])
    assert m["auc_roc"] is None and m["auc_pr"] is None
    assert m["sensitivity"] == 4 / 6 and m["specificity"] == 3 / 4
    assert "N/A (need probabilities)" in M.format_report(m, "x")


def test_single_class_gives_nan():
    # only negatives: thresholds 0.75 > 0.5 > 0.25, no positive at any of them
    curve = (np.array([0.75, 0.5, 0.25], np.float32), np.zeros(3, np.int64),
             np.array([1, 3, 4], np.int64))
    m = M.medical_metrics([3, 1, 0, 0, 0, 0], curve)
    assert math.isnan(m["auc_roc"]) and math.isnan(m["auc_pr"])
    assert m["confusion_matrix"].tolist() == [[3, 1], [0, 0]]
    assert m["accuracy"] == 0.75 and m["specificity"] == 0.75
    assert m["sensitivity"] == 0 and m["recall"] == 0.0 and m["f1"] == 0.0 and m["mcc"] == 0.0
    # only positives
    curve = (np.array([0.75, 0.25], np.float32), np.array([2, 3], np.int64),
             np.zeros(2, np.int64))
    m = M.medical_metrics([0, 0, 1, 2, 0, 0], curve)
    assert math.isnan(m["auc_roc"]) and abs(m["auc_pr"] - 1.0) <= TOL
    assert m["sensitivity"] == 2 / 3 and m["specificity"] == 0 and m["precision"] == 1.0


def test_zero_counts_give_the_empty_loader_dictionary():
    empty = (np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    m = M.medical_metrics([0] * 6, empty)
    assert set(m) == set(CASES["n2_one_of_each"]["metrics"])
    assert m["confusion_matrix"].tolist() == [[0, 0], [0, 0]]
    assert all(m[k] == 0 for k in INT_KEYS)
    for k in ("accuracy", "auc_roc", "auc_pr", "mcc", "kappa"):
        assert math.isnan(m[k]), k
    for k in ("precision", "recall", "f1", "sensitivity", "specificity", "ppv", "npv", "fpr",
              "fnr", "balanced_accuracy", "f_harmonic"):
        assert m[k] == 0, k
    assert "Healthy" in m["classification_report"] and "Ulcer" in m["classification_report"]
    M.format_report(m, "empty")  # formats without raising

    class Loader(list):
        pass

    res = M.evaluate_extended(torch.nn.Identity(), Loader())  # no batch: no device work
    assert set(res) == {"y_true", "y_pred", "y_probs", "metrics"}
    assert res["y_true"].shape == res["y_pred"].shape == res["y_probs"].shape == (0,)
    assert res["y_probs"].dtype == np.float32 and math.isnan(res["metrics"]["auc_roc"])
    assert res["metrics"]["tn"] == 0


def test_report_and_summary_text():
    results = {"RGB-Only": _metrics(CASES["n257_random_20pct_positive"]),
               "Thermal-Only": _metrics(CASES["n600_sixteenths_heavy_ties"]),
               "Multimodal": _metrics(CASES["n7_ties_across_classes"])}
    for name, m in results.items():
        text = M.format_report(m, name)
        assert f"EXTENDED MEDICAL METRICS: {name}" in text
        for k in ("accuracy", "precision", "recall", "f1", "sensitivity", "specificity", "ppv",
                  "npv", "balanced_accuracy", "auc_roc", "auc_pr", "mcc", "kappa", "fpr", "fnr"):
            assert f"{m[k]:.4f}" in text, k
        assert f"TN: {m['tn']:4d}  FP: {m['fp']:4d}" in text
        assert f"FN: {m['fn']:4d}  TP: {m['tp']:4d}" in text
        assert m["classification_report"] in text
    text = M.format_summary(results)
    assert "SUMMARY COMPARISON" in text
    for name, m in results.items():
        for k in ("f1", "sensitivity", "specificity"):
            assert f"  {name:20s}: {m[k]:.4f}" in text


def test_plots_write_png_files(tmp_path):
    pytest.importorskip("matplotlib")
    case = CASES["n600_sixteenths_heavy_ties"]
    m = _metrics(case)
    paths = [M.plot_confusion_matrix(m["confusion_matrix"], "Multimodal", tmp_path),
             M.plot_roc_curve(_curve(case), "Multimodal", tmp_path),
             M.plot_precision_recall_curve(_curve(case), "Multimodal", str(tmp_path))]
    assert [p.split("/")[-1] for p in paths] == [
        "confusion_matrix_Multimodal.png", "roc_curve_Multimodal.png", "pr_curve_Multimodal.png"]
    for p in paths:
        with open(p, "rb") as f:
            data = f.read()
        assert len(data) > 1000 and data[:8] == b"\x89PNG\r\n\x1a\n"


def test_plots_name_the_missing_package(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name.split(".")[0] == "matplotlib":
            raise ImportError("No module named 'matplotlib'")
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.raises(ImportError, match="matplotlib package"):
        M.plot_roc_curve(_curve(CASES["n2_one_of_each"]), "x", ".")


def test_binary_curve_rejects_host_tensors_and_bad_arguments():
    prob, labels = torch.zeros(8), torch.zeros(8, dtype=torch.int64)
    with pytest.raises((ValueError, TypeError)):
        ops.binary_curve(prob, labels)
    with pytest.raises((ValueError, TypeError)):
        ops.binary_curve(prob.double(), labels)
    # argument validation is host code: DFU_E_INVALID without a device
    lib = L.load()
    buf = np.zeros(64, np.int64).ctypes.data  # non-NULL, never dereferenced
    call = lambda n=4, **k: lib.dfu_binary_curve(  # noqa: E731
        *[k.get(a, buf) for a in ("prob", "labels")], n,
        *[k.get(a, buf) for a in ("thresholds", "tps", "fps", "k_out", "workspace")], None)
    for bad in (dict(n=0), dict(n=-1), dict(n=1 << 20), dict(prob=None), dict(labels=None),
                dict(thresholds=None), dict(tps=None), dict(fps=None), dict(k_out=None),
                dict(workspace=None)):
        assert call(**bad) == L.DFU_E_INVALID, bad
    assert b"dfu_binary_curve" in lib.dfu_last_error_string()
