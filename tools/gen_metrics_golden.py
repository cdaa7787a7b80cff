"""Generates tests/golden/extended_metrics.json: the REFERENCE's MedicalMetricsCalculator
(notebooks/extended_metrics.py) and scikit-learn's curve functions run on small synthetic
prediction sets, on the CPU.  The calculator is extracted from the reference checkout with `ast`
at run time and executed with only the names it uses in scope (the script builds datasets and
models at import time, so it is not imported whole); this file holds none of its text.

Recorded per case: y_true, y_pred, y_probs (fp32 values; a JSON double holds them exactly), every
metric of the calculator, roc_curve(y_true, y_probs), precision_recall_curve(y_true, y_probs)
and _binary_clf_curve's (fps, tps, thresholds).  The ROC's first threshold is inf, written as
JSON's Infinity extension (Python's json reads it back).

Usage:  python tools/gen_metrics_golden.py <reference checkout>
Needs scikit-learn (the fixtures were recorded with 1.7.2); the tests need only the JSON file.
"""
import ast
import json
import os
import sys

import numpy as np
import sklearn
from sklearn import metrics as SM
from sklearn.metrics._ranking import _binary_clf_curve

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "extended_metrics.json")
SCRIPT = os.path.join("notebooks", "extended_metrics.py")
CALCULATOR = "MedicalMetricsCalculator"
SKLEARN_NAMES = ["accuracy_score", "f1_score", "precision_score", "recall_score",
                 "confusion_matrix", "classification_report", "roc_auc_score", "roc_curve",
                 "precision_recall_curve", "auc", "matthews_corrcoef", "cohen_kappa_score"]


def extract_calculator(reference):
    path = os.path.join(reference, SCRIPT)
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == CALCULATOR]
    assert len(body) == 1, [n.name for n in body]
    ns = {"np": np}
    ns.update({name: getattr(SM, name) for name in SKLEARN_NAMES})
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns[CALCULATOR]


def cases():
    """name -> (y_true int64, y_pred int64, y_probs fp32)."""
    rng = np.random.default_rng(20240607)
    out = {}

    def add(name, y, prob, pred=None):
        y = np.asarray(y, np.int64)
        prob = np.asarray(prob, np.float32)
        pred = (prob > 0.5).astype(np.int64) if pred is None else np.asarray(pred, np.int64)
        assert y.shape == prob.shape == pred.shape and set(y.tolist()) == {0, 1}
        out[name] = (y, pred, prob)

    add("n2_one_of_each", [0, 1], [0.25, 0.75])
    add("n7_ties_across_classes", [0, 1, 0, 1, 1, 0, 1], [.5, .5, .25, .75, .25, .75, .5],
        pred=[1, 0, 0, 1, 0, 1, 1])
    y = (rng.random(257) < 0.2).astype(np.int64)
    y[:2] = (0, 1)
    add("n257_random_20pct_positive", y, np.clip(rng.normal(0.35 + 0.3 * y, 0.2), 0.0, 1.0))
    y = rng.integers(0, 2, 600)
    p = np.clip(rng.normal(0.4 + 0.2 * y, 0.25), 0.0, 1.0)
    add("n600_sixteenths_heavy_ties", y, np.round(p * 16) / 16)
    y = rng.integers(0, 2, 40)
    y[:2] = (0, 1)
    add("n40_every_prediction_0", y, rng.random(40) * 0.5, pred=np.zeros(40))
    y = rng.integers(0, 2, 30)
    y[:2] = (1, 0)
    add("n30_every_score_identical", y, np.full(30, 0.5), pred=rng.integers(0, 2, 30))
    y = np.r_[np.zeros(32), np.ones(32)][rng.permutation(64)]
    sep = np.where(y == 1, 0.55 + 0.4 * rng.random(64), 0.05 + 0.4 * rng.random(64))
    add("n64_perfect_separation", y, sep)
    add("n64_fully_inverted", y, 1.0 - sep.astype(np.float32))
    return out


def plain(v):
    """numpy values -> JSON types."""
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


def main(reference):
    calc = extract_calculator(reference)
    res = {"sklearn_version": sklearn.__version__, "cases": {}}
    for name, (y, pred, prob) in cases().items():
        m = calc(y, pred, prob).get_all_metrics()
        fpr, tpr, roc_t = SM.roc_curve(y, prob)
        precision, recall, pr_t = SM.precision_recall_curve(y, prob)
        fps, tps, clf_t = _binary_clf_curve(y, prob)
        res["cases"][name] = {
            "y_true": y.tolist(), "y_pred": pred.tolist(),
            "y_probs": prob.astype(np.float64).tolist(),
            "metrics": {k: plain(v) for k, v in m.items()},
            "roc_curve": {"fpr": fpr.tolist(), "tpr": tpr.tolist(),
                          "thresholds": roc_t.astype(np.float64).tolist()},
            "precision_recall_curve": {"precision": precision.tolist(),
                                       "recall": recall.tolist(),
                                       "thresholds": pr_t.astype(np.float64).tolist()},
            "binary_clf_curve": {"fps": np.asarray(fps, np.int64).tolist(),
                                 "tps": np.asarray(tps, np.int64).tolist(),
                                 "thresholds": clf_t.astype(np.float64).tolist()},
        }
    with open(OUT, "w") as f:
        json.dump(res, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
