"""What the evaluation passes of training.loop, training.tta, training.metrics and
training.gradcam_viz share, in one place: the single device -> host read (read_once), the batch
loop that turns a loader into per-sample probabilities and decisions on the device (predict),
and the formulas on confusion counts with their three conventions for an empty denominator.

Imports numpy, torch and dfu_hip.ops only; the four modules above import from here.
"""
import numpy as np
import torch

from dfu_hip import ops


# ------------------------------------------------------------------------ the host read
def read_once(named):
    """One device -> host copy of several tensors: `named` is an iterable of (name, tensor),
    the result {name: numpy array} with each tensor's own dtype and shape, every array a copy of
    its own.  Tensors already on the host and tensors without elements are taken as well."""
    named = sorted(named, key=lambda kv: -kv[1].element_size())  # keeps every offset aligned
    flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for _, t in named]).cpu().numpy()
    out, at = {}, 0
    for name, t in named:
        nbytes = t.numel() * t.element_size()
        dtype = torch.empty(0, dtype=t.dtype).numpy().dtype
        out[name] = flat[at:at + nbytes].view(dtype).reshape(tuple(t.shape)).copy()
        at += nbytes
    return out


# ------------------------------------------------------------------------ the batch loop
def call_model(model, *inputs):
    """The default `forward` of every pass: model(rgb, thermal) for the fusion model, model(x)
    otherwise."""
    return model(*inputs)


SHAPE_ERROR = "model output {shape} for {samples} samples: expected [B, 1] or [B, 2]"


def predict(model, loader, forward=None, views=1, shape_error=SHAPE_ERROR):
    """The model over `loader` in eval mode under no_grad: every batch is (*inputs [B * views,
    ...], labels [B]), forward(model, *inputs) (default call_model) gives [B * views, 1] or
    [B * views, 2], and ops.tta_reduce reduces the views of a sample.  Returns (prob fp32 [n],
    pred int64 [n], labels int64 [n]) on the device, or None when the loader yields nothing.
    Any other output shape raises ValueError(shape_error.format(shape=, samples=, views=))."""
    forward = forward or call_model
    model.eval()
    probs, preds, ys = [], [], []
    with torch.no_grad():
        for batch in loader:
            *inputs, labels = batch
            out = forward(model, *inputs)
            if out.dim() != 2 or out.shape[1] not in (1, 2) or \
                    out.shape[0] != labels.shape[0] * views:
                raise ValueError(shape_error.format(shape=tuple(out.shape),
                                                    samples=labels.shape[0], views=views))
            prob, pred = ops.tta_reduce(out, views)
            probs.append(prob)
            preds.append(pred)
            ys.append(labels)
    if not ys:
        return None
    return torch.cat(probs), torch.cat(preds), torch.cat(ys).long()


# ------------------------------------------------------------------- the count formulas
# What a ratio is when its denominator is 0, one name per convention:
NAN = float("nan")  # the reference script would raise or divide by zero (training.tta)
SKLEARN_ZERO = 0.0  # scikit-learn's zero_division=0
GUARD_ZERO = 0      # the reference calculator's own guard (extended_metrics.py:421-426): an int


def ratio(num, den, zero):
    """num / den, or `zero` (NAN, SKLEARN_ZERO, GUARD_ZERO) when the denominator, a count, is
    0."""
    return num / den if den else zero


def f1_binary(tp, fp, fn):
    """Binary F1 of the positive class, 2 tp / (2 tp + fp + fn); 0.0 when undefined, as
    f1_score reports it."""
    return ratio(2 * tp, 2 * tp + fp + fn, SKLEARN_ZERO)


def confusion_2x2(tn, fp, fn, tp):
    """sklearn's confusion_matrix layout, row = label, column = prediction: int64 [[tn, fp],
    [fn, tp]]."""
    return np.array([[tn, fp], [fn, tp]], dtype=np.int64)
