"""The reference's test-time augmentation robustness evaluation (notebooks/
test_time_augmentation.py) on the HIP modules, shaped for a GPU.

Reference loop shape (:191-258 RGB-only, :261-328 thermal-only, :331-401 fusion — three copies
of one function):
  model.eval(); no_grad
  for batch of PIL images: for image: for aug in range(num_tta):
      transform the PIL image (tta or clean Compose), .to(device), model at batch 1,
      torch.sigmoid(output).cpu()                          <- one forward and one sync per view
      pred = prob > 0.5
    sample pred = mean(view preds) > 0.5 (majority vote), sample prob = mean(view probs)
  accuracy_score, f1_score, roc_auc_score(labels, probs), confusion_matrix -> sensitivity,
  specificity
  print_tta_comparison (:404-441): clean (num_tta=1, no augmentation) against TTA (5 views),
  ROBUST / MODERATE / NOT ROBUST on |accuracy drop| < 0.05 / < 0.15.

Here each image is decoded, copied and resized once, its K views are gathered on the device from
the one resized image (data.gpu_transforms, views=K; dfu_augment_views), the model runs once per
loader batch over all batch * K rows, dfu_tta_reduce gives the per-sample mean probability and
vote (the batch loop is evalpass.predict), dfu_binary_eval_counts the confusion and AUC pair
counts, and the host reads once at the end (evalpass.read_once).  A [N, 1] model output is the
script's sigmoid head; a [N, 2] output (this repository's softmax heads) takes softmax[:, 1] and
the argmax per view.

Single process only: the pass is not sharded over data-parallel ranks.
"""
import numpy as np
import torch

from dfu_hip import ops

from .evalpass import NAN, confusion_2x2, f1_binary, predict, ratio, read_once

ROBUST_BELOW = 0.05     # test_time_augmentation.py:430
MODERATE_BELOW = 0.15   # :432
_SHAPE_ERROR = ("model output {shape} for {samples} samples of {views} views: "
                "expected [N, 1] or [N, 2]")


def metrics_from_counts(counts, predictions, probabilities, labels):
    """The script's result dict (:239-258) from {tn, fp, fn, tp, greater, ties}: accuracy, binary
    F1 of class 1 (0 when undefined, as sklearn reports), AUC-ROC = (greater + ties / 2) /
    (pos * neg), sensitivity tp / (tp + fn), specificity tn / (tn + fp), the confusion matrix
    [[tn, fp], [fn, tp]].  A metric whose denominator is 0 is nan (the script would raise or
    divide by zero)."""
    tn, fp, fn, tp, greater, ties = (int(c) for c in counts)
    n, pos, neg = tn + fp + fn + tp, fn + tp, tn + fp
    return {
        "accuracy": ratio(tn + tp, n, NAN),
        "f1": f1_binary(tp, fp, fn),
        "auc": ratio(greater + 0.5 * ties, pos * neg, NAN),
        "sensitivity": ratio(tp, pos, NAN),
        "specificity": ratio(tn, neg, NAN),
        "confusion_matrix": confusion_2x2(tn, fp, fn, tp),
        "predictions": np.asarray(predictions),
        "probabilities": np.asarray(probabilities),
        "labels": np.asarray(labels),
    }


def evaluate_tta(model, loader, num_tta=5, use_augmentation=True, forward=None,
                 results_path=None):
    """One evaluate_*_with_tta call of the script: `loader` (a GpuPairLoader / GpuImageLoader
    of data.gpu_transforms built with views=num_tta and, for use_augmentation, rgb_tta_transform
    / thermal_tta_transform, else the val-test transforms) yields (*inputs [B * num_tta, ...],
    labels [B]); forward(model, *inputs) defaults to model(*inputs).  num_tta and
    use_augmentation must say what the loader does.  Returns the script's dict
    (metrics_from_counts); with results_path it is also saved there (torch.save)."""
    if num_tta < 1:
        raise ValueError(f"num_tta = {num_tta}")
    views = getattr(loader, "views", None)
    if views is not None and views != num_tta:
        raise ValueError(f"the loader yields {views} views per sample, num_tta = {num_tta}: "
                         f"build it with views=num_tta")
    specs = [p.spec for p in (getattr(loader, a, None) for a in ("rgb", "thermal", "pre"))
             if p is not None]
    if specs and any(s.random for s in specs) != bool(use_augmentation):
        raise ValueError(f"use_augmentation = {use_augmentation}, but the loader's transforms "
                         f"are {'random' if specs[0].random else 'not random'}")
    out = predict(model, loader, forward, num_tta, _SHAPE_ERROR)
    if out is None:
        res = metrics_from_counts([0] * 6, np.zeros(0, np.int64), np.zeros(0, np.float32),
                                  np.zeros(0, np.int64))
    else:
        prob, pred, y = out
        counts = ops.binary_eval_counts(prob, pred, y)
        host = read_once((("counts", counts), ("pred", pred), ("y", y), ("prob", prob)))
        res = metrics_from_counts(host["counts"], host["pred"], host["prob"], host["y"])
    if results_path is not None:
        torch.save(res, results_path)
    return res


def compare_tta(clean, tta):
    """print_tta_comparison's robustness figures (:424-435): the accuracy and F1 drops from the
    clean to the TTA evaluation and the verdict on |accuracy drop|."""
    acc_drop = clean["accuracy"] - tta["accuracy"]
    f1_drop = clean["f1"] - tta["f1"]
    if abs(acc_drop) < ROBUST_BELOW:
        verdict = "ROBUST"
    elif abs(acc_drop) < MODERATE_BELOW:
        verdict = "MODERATE"
    else:
        verdict = "NOT ROBUST"
    return {"acc_drop": acc_drop, "f1_drop": f1_drop, "verdict": verdict}


_VERDICT_TEXT = {
    "ROBUST": "ROBUST: accuracy holds under the augmented views",
    "MODERATE": "MODERATE: accuracy moves noticeably under the augmented views",
    "NOT ROBUST": "NOT ROBUST: accuracy changes by 15 points or more under the augmented views",
}


def format_tta_comparison(clean, tta, model_name, num_tta=5):
    """The clean-vs-TTA report of print_tta_comparison (:404-441) as text: the five metrics of
    both evaluations, the drops, the verdict and the two confusion matrices."""
    c = compare_tta(clean, tta)
    bar = "=" * 70
    lines = [bar, f"Test-time augmentation: {model_name}", bar]
    for title, m in (("clean (1 view, no augmentation)", clean),
                     (f"TTA ({num_tta} augmented views)", tta)):
        lines += ["", title] + [f"  {name:<12}{m[key]:.4f}" for name, key in (
            ("accuracy", "accuracy"), ("F1", "f1"), ("AUC-ROC", "auc"),
            ("sensitivity", "sensitivity"), ("specificity", "specificity"))]
    lines += ["", "clean - TTA",
              f"  accuracy    {c['acc_drop']:.4f} ({c['acc_drop'] * 100:.2f}%)",
              f"  F1          {c['f1_drop']:.4f}",
              "", _VERDICT_TEXT[c["verdict"]],
              "", "confusion matrix, clean:", str(clean["confusion_matrix"]),
              "confusion matrix, TTA:", str(tta["confusion_matrix"])]
    return "\n".join(lines)
