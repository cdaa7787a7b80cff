"""The reference's extended medical metrics evaluation (notebooks/extended_metrics.py) on the HIP
modules: sensitivity, specificity, PPV / NPV, MCC, Cohen's kappa, balanced accuracy, ROC-AUC,
PR-AUC, the ROC and precision-recall curves, the printed report and the plots.

Reference shape (:581-642 three copies of one loop, :374-490 MedicalMetricsCalculator, :497-574
plots, :649-867 main):
  model.eval(); no_grad
  for batch: softmax(output)[:, 1].cpu(), argmax(output).cpu()     <- two syncs per batch
  sklearn on the host: confusion_matrix, accuracy / precision / recall / f1, classification_report,
  roc_auc_score, precision_recall_curve + auc, matthews_corrcoef, cohen_kappa_score,
  roc_curve / precision_recall_curve again for each plot.

Here dfu_tta_reduce (views = 1) gives the probability and decision of every batch on the device
(the batch loop is evalpass.predict), dfu_binary_eval_counts the confusion and pair counts and
dfu_binary_curve the distinct thresholds with their true / false positive counts, and the host
reads once at the end (evalpass.read_once).  Every metric is then fp64 arithmetic on those
integers (numpy; scikit-learn is not needed), following scikit-learn 1.7.2's definitions:
zero_division=0, the ROC with collinear points dropped, the PR-AUC as the trapezoid area of
precision over recall (the script's auc(recall, precision), not average precision).

Single process only: the pass is not sharded over data-parallel ranks.
"""
import math
import os

import numpy as np
import torch

from dfu_hip import ops

from .evalpass import (GUARD_ZERO, NAN, SKLEARN_ZERO, confusion_2x2, f1_binary, predict, ratio,
                       read_once)

TARGET_NAMES = ("Healthy", "Ulcer")   # extended_metrics.py:410


def _curve_arrays(curve):
    thresholds, tps, fps = curve
    thresholds = np.asarray(thresholds, dtype=np.float64)
    tps, fps = np.asarray(tps, dtype=np.int64), np.asarray(fps, dtype=np.int64)
    if not (thresholds.shape == tps.shape == fps.shape and thresholds.ndim == 1):
        raise ValueError("curve: (thresholds[:K], tps[:K], fps[:K]) of one length")
    return thresholds, tps, fps


def _trapezoid(x, y):
    """sklearn.metrics.auc: the trapezoid area under y over a monotonic x, either direction."""
    if x.shape[0] < 2:
        return NAN
    dx = np.diff(x)
    return abs(float(np.sum(dx * (y[1:] + y[:-1]) / 2.0)))


def roc_curve(curve):
    """(fpr, tpr, thresholds) as sklearn.metrics.roc_curve returns them for the samples behind
    `curve` = (thresholds[:K], tps[:K], fps[:K]): points collinear with both neighbours are
    dropped (drop_intermediate), the curve starts at (0, 0) with threshold inf.  A rate whose
    class has no sample is nan."""
    thresholds, tps, fps = _curve_arrays(curve)
    if tps.shape[0] > 2:
        keep = np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True]
        thresholds, tps, fps = thresholds[keep], tps[keep], fps[keep]
    tps, fps = np.r_[0, tps].astype(np.float64), np.r_[0, fps].astype(np.float64)
    thresholds = np.r_[np.inf, thresholds]
    fpr = fps / fps[-1] if fps[-1] > 0 else np.full(fps.shape, np.nan)
    tpr = tps / tps[-1] if tps[-1] > 0 else np.full(tps.shape, np.nan)
    return fpr, tpr, thresholds


def precision_recall_curve(curve):
    """(precision, recall, thresholds) as sklearn.metrics.precision_recall_curve returns them:
    thresholds ascending, precision and recall one longer, ending in (precision 1, recall 0).
    Without a positive sample the recall is 1 everywhere, as sklearn defines it."""
    thresholds, tps, fps = _curve_arrays(curve)
    ps = tps + fps
    precision = np.zeros(tps.shape, dtype=np.float64)
    np.divide(tps, ps, out=precision, where=ps != 0)
    if tps.shape[0] and tps[-1] > 0:
        recall = tps / tps[-1]
    else:
        recall = np.ones(tps.shape, dtype=np.float64)
    return np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0], thresholds[::-1].copy()


def classification_report(tn, fp, fn, tp):
    """sklearn.metrics.classification_report(y_true, y_pred, target_names=['Healthy', 'Ulcer'],
    zero_division=0) as text, from the confusion counts."""
    n = tn + fp + fn + tp
    # sklearn 1.7.2 counts in floating point when no prediction at all is correct, and then
    # prints the supports as "32.0": the text follows it there too
    as_support = float if n and tn + tp == 0 else int
    # per class: hits, predicted as the class, members of the class
    rows = []
    for name, hit, pred, true in ((TARGET_NAMES[0], tn, tn + fn, tn + fp),
                                  (TARGET_NAMES[1], tp, tp + fp, tp + fn)):
        rows.append((name, ratio(hit, pred, SKLEARN_ZERO), ratio(hit, true, SKLEARN_ZERO),
                     ratio(2.0 * hit, true + pred, SKLEARN_ZERO), as_support(true)))
    vals = np.array([r[1:4] for r in rows], dtype=np.float64)
    support = np.array([r[4] for r in rows], dtype=np.float64)
    macro = vals.mean(axis=0)
    weighted = (vals * support[:, None]).sum(axis=0) / n if n else np.zeros(3)
    width = len("weighted avg")
    row_fmt = "{:>{width}s} " + " {:>9.2f}" * 3 + " {:>9}\n"
    text = ("{:>{width}s} " + " {:>9}" * 4).format("", "precision", "recall", "f1-score",
                                                   "support", width=width) + "\n\n"
    for r in rows:
        text += row_fmt.format(*r, width=width)
    text += "\n"
    text += ("{:>{width}s} " + " {:>9}" * 2 + " {:>9.2f} {:>9}\n").format(
        "accuracy", "", "", ratio(2.0 * (tn + tp), 2 * n, SKLEARN_ZERO), as_support(n),
        width=width)
    text += row_fmt.format("macro avg", *macro, as_support(n), width=width)
    text += row_fmt.format("weighted avg", *weighted, as_support(n), width=width)
    return text


def medical_metrics(counts, curve=None):
    """MedicalMetricsCalculator's dictionary (:385-445) from `counts` = {tn, fp, fn, tp, greater,
    ties} (ops.binary_eval_counts, on the host) and `curve` = the host copy of
    (thresholds[:K], tps[:K], fps[:K]) (ops.binary_curve); without a curve auc_roc and auc_pr
    are None, as the calculator without probabilities.

    precision, recall and f1 are 0 where undefined (zero_division=0); sensitivity, specificity,
    ppv, npv, fpr, fnr and f_harmonic are the integer 0 where the calculator's guard gives it.
    Where the reference cannot answer the value is nan (the convention of training.tta.
    metrics_from_counts): auc_roc unless both classes are present, auc_pr without a positive
    sample, accuracy, mcc and kappa without any sample, kappa when the chance agreement is 1."""
    tn, fp, fn, tp = (int(c) for c in list(counts)[:4])
    n, pos, neg = tn + fp + fn + tp, fn + tp, tn + fp
    m = {"confusion_matrix": confusion_2x2(tn, fp, fn, tp),
         "tn": tn, "fp": fp, "fn": fn, "tp": tp,
         "accuracy": ratio(tn + tp, n, NAN),
         "precision": ratio(tp, tp + fp, SKLEARN_ZERO),
         "recall": ratio(tp, pos, SKLEARN_ZERO),
         "f1": f1_binary(tp, fp, fn),
         "classification_report": classification_report(tn, fp, fn, tp),
         "sensitivity": ratio(tp, tp + fn, GUARD_ZERO),
         "specificity": ratio(tn, tn + fp, GUARD_ZERO),
         "ppv": ratio(tp, tp + fp, GUARD_ZERO),
         "npv": ratio(tn, tn + fn, GUARD_ZERO),
         "fpr": ratio(fp, fp + tn, GUARD_ZERO),
         "fnr": ratio(fn, fn + tp, GUARD_ZERO)}
    if curve is None:
        m["auc_roc"] = m["auc_pr"] = None
    else:
        fpr, tpr, _ = roc_curve(curve)
        m["auc_roc"] = _trapezoid(fpr, tpr) if pos and neg else NAN
        precision, recall, _ = precision_recall_curve(curve)
        m["auc_pr"] = _trapezoid(recall, precision) if pos else NAN
    # Matthews: covariance of the two labelings over the product of their deviations; 0 when
    # either labeling is constant (sklearn)
    pred1, pred0 = tp + fp, tn + fn
    cov_tp = (tn + tp) * n - (neg * pred0 + pos * pred1)
    cov_tt = n * n - (neg * neg + pos * pos)
    cov_pp = n * n - (pred0 * pred0 + pred1 * pred1)
    if not n:
        m["mcc"] = NAN
    else:
        m["mcc"] = cov_tp / math.sqrt(cov_tt * cov_pp) if cov_tt * cov_pp else 0.0
    # Cohen: 1 - observed disagreement / disagreement expected from the marginals
    expected = (pred0 * pos + pred1 * neg) / n if n else 0.0
    m["kappa"] = 1.0 - (fp + fn) / expected if expected else NAN
    sens, spec = m["sensitivity"], m["specificity"]
    m["balanced_accuracy"] = (sens + spec) / 2
    m["f_harmonic"] = 2 * (sens * spec) / (sens + spec) if (sens + spec) > 0 else 0
    return m


def _evaluate(model, loader, forward=None):
    """evaluate_extended's pass: (result dict, host curve triple)."""
    out = predict(model, loader, forward)
    if out is None:
        empty = (np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
        return {"y_true": np.zeros(0, np.int64), "y_pred": np.zeros(0, np.int64),
                "y_probs": np.zeros(0, np.float32),
                "metrics": medical_metrics([0] * 6, empty)}, empty
    prob, pred, y = out
    counts = ops.binary_eval_counts(prob, pred, y)
    thresholds, tps, fps, k = ops.binary_curve(prob, y)
    # the pass's one device -> host read (curve entries past K are not meaningful: cut below)
    host = read_once((("counts", counts), ("k", k), ("pred", pred), ("y", y), ("prob", prob),
                      ("thresholds", thresholds), ("tps", tps), ("fps", fps)))
    if np.isnan(host["prob"]).any():
        raise ValueError("Input contains NaN")
    K = int(host["k"][0])
    curve = (host["thresholds"][:K], host["tps"][:K], host["fps"][:K])
    return {"y_true": host["y"], "y_pred": host["pred"], "y_probs": host["prob"],
            "metrics": medical_metrics(host["counts"], curve)}, curve


def evaluate_extended(model, loader, forward=None, results_path=None):
    """One evaluate_* call of the script plus its MedicalMetricsCalculator: `loader` yields
    (*inputs, labels [B]); forward(model, *inputs) defaults to model(*inputs) and gives [B, 2]
    (softmax[:, 1] and argmax) or [B, 1] (sigmoid, > 0.5).  The model runs in eval mode under
    no_grad; the host reads the device once, after the last batch.  Returns {'y_true', 'y_pred',
    'y_probs', 'metrics'} (numpy arrays and medical_metrics' dictionary), the layout of the
    script's results.pt; with results_path it is also saved there (torch.save).  A NaN
    probability raises ValueError("Input contains NaN"), as sklearn does in the script; an empty
    loader gives zero counts and nan values.

    Single process only: the pass is not sharded over data-parallel ranks."""
    res, _ = _evaluate(model, loader, forward)
    if results_path is not None:
        torch.save(res, results_path)
    return res


def _f4(v):
    return "N/A" if v is None else f"{v:.4f}"


def format_report(metrics, model_name="Model"):
    """MedicalMetricsCalculator.print_report (:450-490) as text."""
    m = metrics
    bar = "=" * 70
    lines = ["", bar, f"EXTENDED MEDICAL METRICS: {model_name}", bar,
             "", "BASIC CLASSIFICATION METRICS:",
             f"  Accuracy:       {_f4(m['accuracy'])}",
             f"  Precision:      {_f4(m['precision'])}",
             f"  Recall:         {_f4(m['recall'])}",
             f"  F1-Score:       {_f4(m['f1'])}",
             "", "MEDICAL IMAGING METRICS (CRITICAL):",
             f"  Sensitivity:    {_f4(m['sensitivity'])}  <- Detect ulcers",
             f"  Specificity:    {_f4(m['specificity'])}  <- Identify healthy",
             f"  PPV:            {_f4(m['ppv'])}  <- Precision for positive",
             f"  NPV:            {_f4(m['npv'])}  <- Precision for negative",
             f"  Balanced Acc:   {_f4(m['balanced_accuracy'])}  <- (Sens+Spec)/2",
             "", "CONFUSION MATRIX:",
             f"  TN: {m['tn']:4d}  FP: {m['fp']:4d}",
             f"  FN: {m['fn']:4d}  TP: {m['tp']:4d}",
             "", "CURVE METRICS:"]
    if m["auc_roc"] is not None:
        lines += [f"  ROC-AUC:        {_f4(m['auc_roc'])}",
                  f"  PR-AUC:         {_f4(m['auc_pr'])}"]
    else:
        lines += ["  ROC-AUC:        N/A (need probabilities)",
                  "  PR-AUC:         N/A (need probabilities)"]
    lines += ["", "AGREEMENT METRICS:",
              f"  MCC:            {_f4(m['mcc'])}  <- Good for imbalanced",
              f"  Kappa Score:    {_f4(m['kappa'])}  <- Inter-rater agreement",
              "", "ERROR RATES:",
              f"  FPR:            {_f4(m['fpr'])}  <- Type I error",
              f"  FNR:            {_f4(m['fnr'])}  <- Type II error (CRITICAL)",
              "", "CLASSIFICATION REPORT:", m["classification_report"]]
    return "\n".join(lines)


def format_summary(all_results):
    """The closing comparison of the script's main (:848-863): F1, sensitivity and specificity
    of every model, `all_results` mapping a model name to its metrics dictionary."""
    bar = "=" * 70
    lines = ["", bar, "SUMMARY COMPARISON", bar]
    for title, key in (("F1-Scores:", "f1"), ("Sensitivity (Detect Ulcers):", "sensitivity"),
                       ("Specificity (Identify Healthy):", "specificity")):
        lines += ["", title] + [f"  {name:20s}: {m[key]:.4f}" for name, m in all_results.items()]
    lines += ["", bar]
    return "\n".join(lines)


def _figure():
    """A (Figure, Axes) pair on an Agg canvas of its own: matplotlib's object API, so no pyplot
    state and no global backend is touched."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError as e:
        raise ImportError("the plots of training.metrics need the matplotlib package, which is "
                          "not installed (the metrics and the report do not need it)") from e
    fig = Figure(figsize=(8, 6))
    FigureCanvasAgg(fig)
    return fig, fig.add_subplot(111)


def _save(fig, output_dir, filename):
    fig.tight_layout()
    path = os.path.join(str(output_dir), filename)
    fig.savefig(path, dpi=300, bbox_inches="tight")
    return path


def plot_confusion_matrix(confusion_matrix, model_name, output_dir):
    """The script's confusion-matrix figure (:497-527) -> confusion_matrix_{model_name}.png in
    output_dir; returns the path."""
    cm = np.asarray(confusion_matrix)
    fig, ax = _figure()
    im = ax.imshow(cm, cmap="Blues", interpolation="nearest")
    fig.colorbar(im)
    ax.set_xticks(np.arange(2))
    ax.set_yticks(np.arange(2))
    ax.set_xticklabels(list(TARGET_NAMES))
    ax.set_yticklabels(list(TARGET_NAMES))
    for i in range(cm.shape[0]):
        for j in range(cm.shape[1]):
            ax.text(j, i, int(cm[i, j]), ha="center", va="center",
                    color="white" if cm[i, j] > cm.max() / 2 else "black",
                    fontsize=14, fontweight="bold")
    ax.set_ylabel("True Label")
    ax.set_xlabel("Predicted Label")
    ax.set_title(f"Confusion Matrix: {model_name}")
    return _save(fig, output_dir, f"confusion_matrix_{model_name}.png")


def plot_roc_curve(curve, model_name, output_dir):
    """The script's ROC figure (:530-551) from the device's curve -> roc_curve_{model_name}.png
    in output_dir; returns the path."""
    fpr, tpr, _ = roc_curve(curve)
    fig, ax = _figure()
    ax.plot(fpr, tpr, color="darkorange", lw=2, label=f"ROC (AUC={_trapezoid(fpr, tpr):.4f})")
    ax.plot([0, 1], [0, 1], color="navy", lw=2, linestyle="--", label="Random")
    ax.set_xlim([0.0, 1.0])
    ax.set_ylim([0.0, 1.05])
    ax.set_xlabel("False Positive Rate")
    ax.set_ylabel("True Positive Rate")
    ax.set_title(f"ROC Curve: {model_name}")
    ax.legend(loc="lower right")
    ax.grid(alpha=0.3)
    return _save(fig, output_dir, f"roc_curve_{model_name}.png")


def plot_precision_recall_curve(curve, model_name, output_dir):
    """The script's precision-recall figure (:554-574) from the device's curve ->
    pr_curve_{model_name}.png in output_dir; returns the path."""
    precision, recall, _ = precision_recall_curve(curve)
    fig, ax = _figure()
    ax.plot(recall, precision, color="green", lw=2,
            label=f"PR (AUC={_trapezoid(recall, precision):.4f})")
    ax.set_xlabel("Recall")
    ax.set_ylabel("Precision")
    ax.set_title(f"Precision-Recall Curve: {model_name}")
    ax.legend(loc="lower left")
    ax.grid(alpha=0.3)
    ax.set_xlim([0.0, 1.0])
    ax.set_ylim([0.0, 1.05])
    return _save(fig, output_dir, f"pr_curve_{model_name}.png")


def run_extended_evaluation(entries, output_dir, plots=True):
    """The script's main (:649-867) without its hard-coded paths: `entries` maps a model name to
    (model, loader, forward) (forward may be None).  Each model is evaluated
    (evaluate_extended), its result saved to <output_dir>/<name>/results.pt and, with `plots`,
    its three figures written beside it.  Returns (all_results: name -> metrics dictionary,
    text: every model's report followed by the summary comparison)."""
    all_results, text = {}, []
    for name, (model, loader, forward) in entries.items():
        out = os.path.join(str(output_dir), name)
        os.makedirs(out, exist_ok=True)
        res, curve = _evaluate(model, loader, forward)
        torch.save(res, os.path.join(out, "results.pt"))
        if plots:
            plot_confusion_matrix(res["metrics"]["confusion_matrix"], name, out)
            plot_roc_curve(curve, name, out)
            plot_precision_recall_curve(curve, name, out)
        all_results[name] = res["metrics"]
        text.append(format_report(res["metrics"], name))
    text.append(format_summary(all_results))
    return all_results, "\n".join(text)
