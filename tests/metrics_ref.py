"""Shared by test_metrics_cpu.py and test_metrics_gpu.py: the recorded fixture cases and numpy
restatements of the device's count vector and of scikit-learn's _binary_clf_curve."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "extended_metrics.json")


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def counts_ref(y_true, y_pred, y_probs):
    """{tn, fp, fn, tp, greater, ties} as dfu_binary_eval_counts defines them."""
    y, d, s = np.asarray(y_true), np.asarray(y_pred), np.asarray(y_probs)
    p, q = s[y == 1][:, None], s[y == 0][None, :]
    return [int(((d == 0) & (y == 0)).sum()), int(((d != 0) & (y == 0)).sum()),
            int(((d == 0) & (y == 1)).sum()), int(((d != 0) & (y == 1)).sum()),
            int((p > q).sum()), int((p == q).sum())]


def clf_curve_ref(y_true, y_probs):
    """_binary_clf_curve over the valid samples (label 0 or 1, score not NaN): a stable sort by
    descending score, one threshold per distinct score, cumulative counts of either class.
    Returns (thresholds fp32, tps int64, fps int64)."""
    y, s = np.asarray(y_true), np.asarray(y_probs, dtype=np.float32)
    ok = ((y == 0) | (y == 1)) & ~np.isnan(s)
    y, s = y[ok], s[ok]
    if not y.size:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.argsort(s, kind="stable")[::-1]
    y, s = y[order], s[order]
    last = np.r_[np.nonzero(np.diff(s))[0], y.size - 1]  # the last sample of every tie group
    tps = np.cumsum(y == 1)[last].astype(np.int64)
    return s[last], tps, (1 + last - tps).astype(np.int64)
