"""Test-time augmentation evaluation on the GPU (notebooks/test_time_augmentation.py):
  * dfu_augment_views through GT.GpuPreprocessor(views=K) against a chain of PIL calls in the TTA
    Compose's order (resize -> rotate -> transpose -> transpose -> transform), bit for bit;
  * dfu_tta_reduce (ops.tta_reduce) against torch on the CPU;
  * dfu_binary_eval_counts (ops.binary_eval_counts) against numpy, exact integers;
  * training.tta.evaluate_tta end to end on a synthetic tree with the fusion model."""
import ctypes
import dataclasses
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import data_inputs as DI  # noqa: E402
import transforms_ref as TR  # noqa: E402

from data import gpu_transforms as GT  # noqa: E402
from data import multimodal as MM  # noqa: E402
from dfu_hip import _lib as L  # noqa: E402
from dfu_hip import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

SRC_SIZES = [(1, 1), (37, 53), (224, 224), (480, 640)]  # (h, w)
K = 3


def _img(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(x / (5 + 3 * c) + c) * np.cos(y / (11 + c))
                  for c in range(3)], -1)
    return np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)


def pil_tta_view(img, spec, p):
    """One view as torchvision's PIL backend runs the TTA Compose (test_time_augmentation.py:
    147-155): Resize, RandomRotation, the two flips, RandomAffine, ToTensor, Normalize."""
    H, W = spec.size
    im = Image.fromarray(np.ascontiguousarray(img, np.uint8), "RGB")
    if im.size != (W, H):
        im = im.resize((W, H), Image.BILINEAR)
    if spec.rotation:
        im = im.rotate(p.angle, Image.NEAREST, expand=False, center=None, fillcolor=(0, 0, 0))
    if p.hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if p.vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    if p.affine is not None:
        angle, tr, scale, shear = p.affine
        m = TR.inverse_affine_matrix([W * 0.5, H * 0.5], angle, tr, scale, shear)
        im = im.transform((W, H), Image.AFFINE, m, Image.NEAREST, fillcolor=(0, 0, 0))
    t = torch.from_numpy(np.array(im, np.uint8, copy=True)).permute(2, 0, 1).contiguous()
    t = t.float().div(255)
    return t.sub_(torch.as_tensor(spec.mean, dtype=torch.float32).view(-1, 1, 1)).div_(
        torch.as_tensor(spec.std, dtype=torch.float32).view(-1, 1, 1))


EXPLICIT = [
    GT.AugParams(hflip=True, angle=12.5, affine=(-7.0, (3, -2), 1.0, (0.0, 0.0))),
    GT.AugParams(vflip=True, angle=-15.0, affine=(10.0, (-11, 11), 1.0, (0.0, 0.0))),
    GT.AugParams(hflip=True, vflip=True, angle=0.0, affine=(0.25, (0, 0), 1.0, (0.0, 0.0))),
    GT.AugParams(angle=3.0, affine=None),
]


@pytest.mark.parametrize("size", [(224, 224), (20, 28)])
@pytest.mark.parametrize("base", ["rgb", "thermal"])
def test_views_match_pil_bitwise(base, size):
    spec = dataclasses.replace(GT.rgb_tta_transform if base == "rgb" else GT.thermal_tta_transform,
                               size=size)
    imgs = [_img(h, w, 7 + i) for i, (h, w) in enumerate(SRC_SIZES)]
    g = torch.Generator().manual_seed(31)
    params = []
    for i in range(len(imgs)):  # per image: one explicit view, then sampled ones
        params += [EXPLICIT[i]] + [GT.sample_params(spec, g) for _ in range(K - 1)]
    out = GT.GpuPreprocessor(spec)(imgs, params, views=K).cpu()
    assert out.shape == (len(imgs) * K, 3) + size and out.dtype == torch.float32
    for i, im in enumerate(imgs):
        for v in range(K):
            ref = pil_tta_view(im, spec, params[i * K + v])
            bad = (out[i * K + v] != ref).sum().item()
            assert bad == 0, f"image {i} {im.shape} view {v} {params[i * K + v]}: {bad} differ"


def test_flip_rotate_identity_views_equal_augment_normalize():
    """order = FLIP_ROTATE with view_src[v] = v is dfu_augment_normalize, colour ops included."""
    spec = GT.rgb_train_transform
    imgs = [_img(h, w, 40 + i) for i, (h, w) in enumerate(SRC_SIZES + [(90, 70), (300, 200)])]
    g = torch.Generator().manual_seed(2)
    params = [GT.sample_params(spec, g) for _ in imgs]
    params[0] = GT.AugParams(hflip=True, angle=-9.0, ops=[(1, 0.8), (2, 1.25), (0, 0.9)],
                             affine=(5.0, (4, -6), 1.1, (0.0, 0.0)))
    assert sum(1 for p in params if any(op == GT.CONTRAST for op, _ in p.ops)) >= 2
    pre = GT.GpuPreprocessor(spec)
    a = pre(imgs, params)
    b = pre(imgs, params, views=1)
    assert a.shape == b.shape and torch.equal(a, b)
    # and K views of one image under the train order: each equals the one-image result
    c = pre(imgs[1:2], params[:3], views=3)
    for v in range(3):
        assert torch.equal(c[v], pre(imgs[1:2], [params[v]])[0])


def test_the_two_orders_differ():
    p = GT.AugParams(hflip=True, angle=10.0)
    tta = dataclasses.replace(GT.rgb_tta_transform, affine=None)
    train_order = dataclasses.replace(tta, order="flip_rotate")
    im = _img(224, 224, 3)
    a = GT.GpuPreprocessor(tta)([im], [p], views=1)
    b = GT.GpuPreprocessor(train_order)([im], [p], views=1)
    assert not torch.equal(a, b)
    assert torch.equal(a[0].cpu(), pil_tta_view(im, tta, p))
    assert torch.equal(b[0].cpu(), TR.reference_transform(im, tta.size, tta.mean, tta.std, True,
                                                          False, 10.0))
    # without views the spec's order still holds (the preprocessor takes the views path itself)
    assert torch.equal(GT.GpuPreprocessor(tta)([im], [p]), a)


def _views_call(resized, rec, view_src, order, out, means, n_views=None, null_src=False):
    n, H, W, _ = resized.shape
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    std = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    par = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    vs = torch.tensor(view_src, dtype=torch.int32, device=DEV)
    rc = L.load().dfu_augment_views(
        resized.data_ptr(), n, par.data_ptr(), None if null_src else vs.data_ptr(),
        len(view_src) if n_views is None else n_views, order, H, W, mean, std, means.data_ptr(),
        out.data_ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_views_index_outside_the_batch_gives_fill_and_bad_args_are_refused():
    H, W, n = 12, 10, 2
    g = torch.Generator().manual_seed(0)
    resized = torch.randint(1, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    spec = dataclasses.replace(GT.thermal_tta_transform, size=(H, W))
    src = [-1, 1, n, 0, 2 ** 31 - 1]
    params = [GT.AugParams(hflip=True, ops=[(GT.CONTRAST, 0.5)])] + [GT.AugParams()] * 4
    rec = GT.pack_params(params, spec)
    out = torch.full((len(src), 3, H, W), 7.0, device=DEV)
    means = torch.empty(len(src), dtype=torch.int32, device=DEV)
    assert _views_call(resized, rec, src, 1, out, means) == 0
    plain = resized.cpu().permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)  # as ToTensor
    for v, s in enumerate(src):
        want = plain[s] if 0 <= s < n else torch.full((3, H, W), -1.0)  # (0 - 0.5) / 0.5
        assert torch.equal(out[v].cpu(), want), v
    for kw in (dict(order=2), dict(order=-1), dict(null_src=True), dict(n_views=0)):
        order = kw.pop("order", 0)
        assert _views_call(resized, rec, src, order, out, means, **kw) == L.DFU_E_INVALID, kw


# ------------------------------------------------------------------------- dfu_tta_reduce
def _logits(rows, C, seed):
    """|x| >= 1e-3 everywhere except a sprinkling of exact zeros (p = 0.5, vote 0)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 3
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 1e-3).copysign(x), x)
    zero = torch.rand(rows, generator=g) < 0.15
    x[zero] = 0.0
    x[0] = 0.0
    return x


def _reduce_ref(x, views):
    """The reduction on the CPU: fp32 view probabilities, their sequential fp32 sum / views, and
    the integer majority vote."""
    if x.shape[1] == 1:
        p = torch.sigmoid(x[:, 0])
        vote = p > 0.5
    else:
        p = torch.softmax(x, 1)[:, 1]
        vote = x.argmax(1) == 1
    p, vote = p.view(-1, views), vote.view(-1, views)
    s = torch.zeros(p.shape[0], dtype=torch.float32)
    for v in range(views):
        s = s + p[:, v]
    return s / torch.tensor(float(views)), (2 * vote.sum(1) > views).long()


@pytest.mark.parametrize("views", [1, 2, 5, 8])
@pytest.mark.parametrize("samples", [1, 3, 65])
@pytest.mark.parametrize("C", [1, 2])
def test_tta_reduce_against_torch(C, samples, views):
    x = _logits(samples * views, C, 100 * C + 10 * samples + views)
    prob, pred = ops.tta_reduce(x.to(DEV), views)
    rp, rd = _reduce_ref(x, views)
    assert prob.dtype == torch.float32 and pred.dtype == torch.int64
    assert prob.shape == pred.shape == (samples,)
    assert torch.equal(pred.cpu(), rd)
    # p in (0, 1): ulp <= 6e-8, a few ulp from exp, at most `views` from the sum
    d = (prob.cpu() - rp).abs().max().item()
    print(f"\n[tta_reduce C={C} samples={samples} views={views}] max |prob - torch| {d:.2e}")
    assert d <= 1e-6


@pytest.mark.parametrize("C", [1, 2])
def test_tta_reduce_tied_votes_and_zeros(C):
    """2 of 4 votes is 0, 3 of 4 is 1; 1 of 2 is 0; an all-zero logit row votes 0 with p 0.5."""
    views = 4
    signs = torch.tensor([[1, 1, -1, -1], [1, -1, 1, 1], [-1, -1, -1, -1], [1, 1, 1, 1],
                          [0, 0, 0, 0], [1, 0, 1, 0], [1, 1, 1, 0]], dtype=torch.float32)
    x1 = (signs * 2.0).reshape(-1, 1)
    x = x1 if C == 1 else torch.cat([torch.zeros_like(x1), x1], 1)
    prob, pred = ops.tta_reduce(x.to(DEV), views)
    assert pred.tolist() == [0, 1, 0, 1, 0, 0, 1]
    assert prob[4].item() == 0.5
    rp, rd = _reduce_ref(x, views)
    assert torch.equal(pred.cpu(), rd) and (prob.cpu() - rp).abs().max().item() <= 1e-6
    two = torch.tensor([[3.0], [-3.0]]) if C == 1 else torch.tensor([[0.0, 3.0], [3.0, 0.0]])
    assert ops.tta_reduce(two.to(DEV), 2)[1].tolist() == [0]
    assert ops.tta_reduce(two.to(DEV), 1)[1].tolist() == [1, 0]


def test_tta_reduce_refuses_other_widths():
    with pytest.raises(L.DfuError) as e:
        ops.tta_reduce(torch.zeros(4, 3, device=DEV), 2)
    assert e.value.code == L.DFU_E_INVALID
    with pytest.raises(ValueError):
        ops.tta_reduce(torch.zeros(5, 1, device=DEV), 2)


# ----------------------------------------------------------------- dfu_binary_eval_counts
def _counts_ref(prob, pred, labels):
    p, q = prob[labels == 1][:, None], prob[labels == 0][None, :]
    return [int(((pred == 0) & (labels == 0)).sum()), int(((pred == 1) & (labels == 0)).sum()),
            int(((pred == 0) & (labels == 1)).sum()), int(((pred == 1) & (labels == 1)).sum()),
            int((p > q).sum()), int((p == q).sum())]


@pytest.mark.parametrize("n", [1, 2, 255, 257, 1000])
def test_binary_eval_counts_against_numpy(n):
    rng = np.random.default_rng(n)
    prob = (rng.integers(0, 17, n) / 16).astype(np.float32)  # sixteenths: ties are common
    pred = rng.integers(0, 2, n)
    for labels in (rng.integers(0, 2, n), np.ones(n, np.int64), np.zeros(n, np.int64)):
        t = [torch.from_numpy(a).to(DEV) for a in (prob, pred, labels)]
        counts = ops.binary_eval_counts(*t)
        want = _counts_ref(prob, pred, labels)
        assert counts.dtype == torch.int64 and counts.tolist() == want, (n, labels[:8])
        if labels.all() or not labels.any():
            assert want[4] == want[5] == 0  # one class only: no pairs
        ops.binary_eval_counts(*t, counts=counts)  # adds to the caller's vector
        assert counts.tolist() == [2 * c for c in want]


def test_binary_eval_counts_gives_sklearn_auc():
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(9)
    n = 700
    labels = rng.integers(0, 2, n)
    prob = np.clip(rng.normal(0.4 + 0.2 * labels, 0.2), 0, 1).astype(np.float32)
    prob[::5] = np.round(prob[::5], 1)
    c = ops.binary_eval_counts(torch.from_numpy(prob).to(DEV),
                               torch.from_numpy((prob > 0.5).astype(np.int64)).to(DEV),
                               torch.from_numpy(labels).to(DEV)).tolist()
    auc = (c[4] + 0.5 * c[5]) / ((c[2] + c[3]) * (c[0] + c[1]))
    assert abs(auc - roc_auc_score(labels, prob)) <= 1e-12


# ------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def fusion():
    from models.fusion import MultimodalFusionModel
    torch.manual_seed(0)
    return MultimodalFusionModel(num_classes=2, dropout=0.7).to(DEV)


@pytest.fixture()
def val_pairs(tmp_path):
    rgb_dir, th_dir = DI.build_tree(str(tmp_path))
    random.seed(42)
    ds = MM.MultimodalDataset(rgb_dir, th_dir, "val", verbose=False)
    assert len(ds) == 8 and sorted(set(ds.labels())) == [0, 1]
    return ds


def test_evaluate_tta_end_to_end(fusion, val_pairs, tmp_path):
    from sklearn.metrics import confusion_matrix, roc_auc_score

    from training import tta as T
    ds, B = val_pairs, 3  # batches of 3, 3, 2 samples
    g = torch.Generator().manual_seed(7)
    loader = GT.GpuPairLoader(ds, B, rgb_spec=GT.rgb_tta_transform,
                              thermal_spec=GT.thermal_tta_transform, views=K, generator=g,
                              num_threads=2)
    seen = []

    def fwd(m, rgb, th):
        assert rgb.shape == th.shape and rgb.shape[0] % K == 0 and rgb.shape[1:] == (3, 224, 224)
        out = m(rgb, th)
        seen.append(out.detach().float().clone())
        return out

    path = tmp_path / "tta_results.pt"
    res = T.evaluate_tta(fusion, loader, num_tta=K, use_augmentation=True, forward=fwd,
                         results_path=str(path))
    assert len(seen) == len(loader) == 3 and not fusion.training

    # the same model on the PIL views, stacked in the same row order, same draws
    g = torch.Generator().manual_seed(7)
    ref_logits = []
    with torch.no_grad():
        for s in range(0, len(ds), B):
            r, t = [], []
            for i in range(s, min(s + B, len(ds))):
                for _ in range(K):  # per sample and per view: RGB parameters, then thermal
                    pr = GT.sample_params(GT.rgb_tta_transform, g)
                    pt = GT.sample_params(GT.thermal_tta_transform, g)
                    r.append(pil_tta_view(GT.decode_rgb(ds.pairs[i][0]), GT.rgb_tta_transform, pr))
                    t.append(pil_tta_view(GT.decode_rgb(ds.pairs[i][1]),
                                          GT.thermal_tta_transform, pt))
            ref_logits.append(fusion(torch.stack(r).to(DEV), torch.stack(t).to(DEV)).float())
    for a, b in zip(seen, ref_logits):
        assert torch.equal(a, b)
    x = torch.cat(ref_logits).cpu()
    rp, rd = _reduce_ref(x, K)
    labels = np.array(ds.labels())
    assert np.array_equal(res["labels"], labels)
    assert np.array_equal(res["predictions"], rd.numpy())
    assert np.array_equal(res["confusion_matrix"], confusion_matrix(labels, rd.numpy(),
                                                                    labels=[0, 1]))
    assert res["probabilities"].dtype == np.float32
    assert np.abs(res["probabilities"] - rp.numpy()).max() <= 1e-6
    got = res["probabilities"]
    p, q = got[labels == 1][:, None], got[labels == 0][None, :]
    assert res["auc"] == ((p > q).sum() + 0.5 * (p == q).sum()) / (p.size * q.size)
    assert abs(res["auc"] - roc_auc_score(labels, got)) <= 1e-12
    assert res["accuracy"] == (rd.numpy() == labels).mean()
    saved = torch.load(str(path), weights_only=False)
    assert set(saved) == set(res) and np.array_equal(saved["predictions"], res["predictions"])


def test_clean_single_view_equals_the_test_phase(fusion, val_pairs):
    from dfu_hip import nn as hnn
    from training import loop
    from training import tta as T
    ds = val_pairs
    clean = T.evaluate_tta(fusion, GT.GpuPairLoader(ds, 4, views=1, num_threads=2), num_tta=1,
                           use_augmentation=False)
    test = loop.evaluate(fusion, GT.GpuPairLoader(ds, 4, num_threads=2), hnn.CrossEntropyLoss(),
                         log=None, device=DEV)
    assert clean["predictions"].tolist() == [int(v) for v in test["test_preds"]]
    assert clean["labels"].tolist() == [int(v) for v in test["test_labels"]] == ds.labels()
    assert np.abs(clean["probabilities"] - np.array(test["test_probs"])).max() <= 1e-6
    assert clean["accuracy"] == test["test_acc"] and clean["f1"] == test["test_f1"]
    # the loader and the arguments must agree
    with pytest.raises(ValueError):
        T.evaluate_tta(fusion, GT.GpuPairLoader(ds, 4), num_tta=5, use_augmentation=False)
    with pytest.raises(ValueError):
        T.evaluate_tta(fusion, GT.GpuPairLoader(ds, 4, views=2), num_tta=2, use_augmentation=True)
