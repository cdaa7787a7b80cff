"""training.evalpass on the GPU: every evaluation pass reads the device exactly once (the
test phase twice: its metrics and its per-sample arrays), and what it returns is what the same
ops calls give when read back directly.  No model runs: the model is torch.nn.Identity() and
the loaders hold ready logits on the device."""
import contextlib
import math

import numpy as np
import pytest
import torch

from dfu_hip import ops
from training import loop
from training import metrics as M
from training import tta as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (3, 2)                       # two batches
LABELS = ([0, 1, 1], [1, 0])


def _batches(C, views=1):
    """[(logits [B * views, C], labels [B])] on the device, a few logits exactly tied."""
    g = torch.Generator().manual_seed(10 * C + views)
    out = []
    for b, y in zip(SIZES, LABELS):
        x = torch.randn(b * views, C, generator=g) * 2
        x[0] = 0.0
        out.append((x.to(DEV), torch.tensor(y, device=DEV)))
    return out


def _is_host(target):
    if isinstance(target, torch.Tensor):
        return not target.is_cuda
    if isinstance(target, (str, torch.device)):
        return torch.device(target).type == "cpu"
    return False


@contextlib.contextmanager
def host_reads(monkeypatch):
    """Counts the calls of Tensor.cpu / .item / .tolist / .to(a host target) on a device tensor
    inside the block: yields the list of their names."""
    calls = []

    def counting(name, real, to_host):
        def wrapper(self, *a, **k):
            if self.is_cuda and to_host(a, k):
                calls.append(name)
            return real(self, *a, **k)
        return wrapper

    def to_host(a, k):
        return any(_is_host(v) for v in list(a[:1]) + [k.get("device"), k.get("other")])
    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist"):
            mp.setattr(torch.Tensor, name, counting(name, getattr(torch.Tensor, name),
                                                    lambda a, k: True))
        mp.setattr(torch.Tensor, "to", counting("to", torch.Tensor.to, to_host))
        yield calls


def test_the_counter_counts_what_it_should(monkeypatch):
    t = torch.arange(3, device=DEV)
    with host_reads(monkeypatch) as calls:
        t.cpu(), t[0].item(), t.tolist(), t.to("cpu"), t.to(torch.device("cpu")), t.to(device="cpu")
        t.to(torch.zeros(1))
        t.to(DEV), t.to(torch.float32), t.cpu().cpu(), t.cpu().tolist(), t.long(), t + 1
    assert calls == ["cpu", "item", "tolist", "to", "to", "to", "to", "cpu", "cpu"]
    with host_reads(monkeypatch) as calls:
        pass
    assert calls == [] and t.cpu().tolist() == [0, 1, 2]


def _same(a, b, where=""):
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), where
    elif isinstance(a, float) and math.isnan(a):
        assert math.isnan(b), where
    else:
        assert a == b, where


def _f32_bits_equal(got, dev):
    want = dev.cpu().numpy()
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("C", [2, 1])
def test_evaluate_tta_reads_once(C, monkeypatch):
    views = 2
    batches = _batches(C, views)
    with host_reads(monkeypatch) as calls:
        res = T.evaluate_tta(torch.nn.Identity(), batches, num_tta=views)
    assert calls == ["cpu"]
    reduced = [ops.tta_reduce(x, views) for x, _ in batches]
    prob, pred = torch.cat([p for p, _ in reduced]), torch.cat([d for _, d in reduced])
    y = torch.cat([y for _, y in batches])
    counts = ops.binary_eval_counts(prob, pred, y).tolist()
    _same(res, T.metrics_from_counts(counts, pred.cpu().numpy(), prob.cpu().numpy(),
                                     y.cpu().numpy()))
    assert res["predictions"].dtype == res["labels"].dtype == np.int64
    assert res["labels"].tolist() == sum(LABELS, [])
    _f32_bits_equal(res["probabilities"], prob)


@pytest.mark.parametrize("C", [2, 1])
def test_evaluate_extended_reads_once(C, monkeypatch):
    batches = _batches(C)
    with host_reads(monkeypatch) as calls:
        res = M.evaluate_extended(torch.nn.Identity(), batches)
    assert calls == ["cpu"]
    reduced = [ops.tta_reduce(x, 1) for x, _ in batches]
    prob, pred = torch.cat([p for p, _ in reduced]), torch.cat([d for _, d in reduced])
    y = torch.cat([y for _, y in batches])
    counts = ops.binary_eval_counts(prob, pred, y).tolist()
    thr, tps, fps, k = ops.binary_curve(prob, y)
    K = int(k.item())
    curve = tuple(t[:K].cpu().numpy() for t in (thr, tps, fps))
    _same(res, {"y_true": y.cpu().numpy(), "y_pred": pred.cpu().numpy(),
                "y_probs": prob.cpu().numpy(), "metrics": M.medical_metrics(counts, curve)})
    assert res["y_true"].dtype == res["y_pred"].dtype == np.int64
    _f32_bits_equal(res["y_probs"], prob)


def _accumulate(batches, criterion):
    """ops.metrics_accumulate over the batches, read back tensor by tensor."""
    conf = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    loss_sum = torch.zeros((1,), dtype=torch.float64, device=DEV)
    nb = torch.zeros((1,), dtype=torch.int64, device=DEV)
    for x, y in batches:
        ops.metrics_accumulate(x, y, criterion(x, y), conf, loss_sum, nb)
    return loop.metrics_from_confusion(conf.cpu(), float(loss_sum.cpu()[0]), int(nb.cpu()[0]))


def test_device_metrics_result_reads_once(monkeypatch):
    batches, crit = _batches(2), torch.nn.CrossEntropyLoss()
    met = loop.DeviceMetrics(2, DEV)
    for x, y in batches:
        met.update(x, y, crit(x, y))
    with host_reads(monkeypatch) as calls:
        res = met.result()
    assert calls == ["cpu"]  # three on the parent tree: one .cpu() per accumulator
    want = _accumulate(batches, crit)
    _same(res, want)
    assert res["n"] == 5 and res["batches"] == 2 and res["loss"] > 0


def test_the_test_phase_reads_twice(monkeypatch):
    batches, crit = _batches(2), torch.nn.CrossEntropyLoss()
    with host_reads(monkeypatch) as calls:
        res = loop.evaluate(torch.nn.Identity(), batches, crit, log=None, device=DEV)
    # its metrics (DeviceMetrics.result) and its per-sample arrays; six on the parent tree
    assert calls == ["cpu", "cpu"]
    logits = torch.cat([x for x, _ in batches])
    probs = ops.softmax_rows(logits)[:, 1].contiguous()
    preds = ops.argmax_rows(logits)
    r = _accumulate(batches, crit)
    assert list(res) == ["test_preds", "test_labels", "test_probs", "test_acc", "test_f1",
                         "test_loss"]
    assert (res["test_acc"], res["test_f1"], res["test_loss"]) == (r["acc"], r["f1"], r["loss"])
    for key in ("test_preds", "test_labels", "test_probs"):
        assert type(res[key]) is list and len(res[key]) == 5
    assert all(type(v) is np.int64 for v in res["test_preds"] + res["test_labels"])
    assert all(type(v) is np.float32 for v in res["test_probs"])
    assert res["test_preds"] == preds.tolist() and res["test_labels"] == sum(LABELS, [])
    _f32_bits_equal(np.array(res["test_probs"]), probs)
