"""training.evalpass without a GPU: the single host read on host tensors of mixed dtypes, the
ratio conventions and count formulas, the empty pass, and the module's import rule (numpy, torch
and dfu_hip.ops only; nothing from the modules that import it)."""
import ast
import math

import numpy as np
import torch

from training import evalpass as E


def test_read_once_returns_every_tensor_as_its_own_typed_copy():
    g = torch.Generator().manual_seed(3)
    named = [  # not in the order of the element sizes; odd byte counts before wider types
        ("i64", torch.randint(-2 ** 40, 2 ** 40, (2, 2), generator=g)),
        ("f64", torch.rand(1, generator=g, dtype=torch.float64)),
        ("f32", torch.randn(5, generator=g)),
        ("u8", torch.randint(0, 256, (3, 4, 3), generator=g, dtype=torch.uint8)),
        ("i32", torch.tensor([-7], dtype=torch.int32)),
        ("none", torch.empty((0,), dtype=torch.float32)),
    ]
    want = {name: t.clone().numpy() for name, t in named}
    got = E.read_once(iter(named))
    assert list(want) == sorted(got, key=list(want).index) and len(got) == len(want)
    for name, w in want.items():
        assert got[name].dtype == w.dtype and got[name].shape == w.shape, name
        assert np.array_equal(got[name], w), name
    # independent copies: writing into one changes no other, and no tensor
    for name in want:
        got[name].view(np.uint8)[...] ^= 0xFF
        for other, t in named:
            if other != name:
                assert np.array_equal(got[other], want[other]), (name, other)
            assert np.array_equal(t.numpy(), want[other]), (name, other)
        got[name].view(np.uint8)[...] ^= 0xFF


def test_ratio_conventions():
    assert math.isnan(E.ratio(3, 0, E.NAN))
    z = E.ratio(3, 0, E.SKLEARN_ZERO)
    assert z == 0.0 and type(z) is float
    z = E.ratio(3, 0, E.GUARD_ZERO)
    assert z == 0 and type(z) is int
    for zero in (E.NAN, E.SKLEARN_ZERO, E.GUARD_ZERO):
        q = E.ratio(3, 7, zero)
        assert q == 3 / 7 and type(q) is float
        assert E.ratio(0, 7, zero) == 0.0


def test_f1_binary_and_confusion_2x2():
    z = E.f1_binary(0, 0, 0)
    assert z == 0.0 and type(z) is float
    assert E.f1_binary(3, 1, 2) == 6 / 9 and E.f1_binary(0, 4, 0) == 0.0
    cm = E.confusion_2x2(1, 2, 3, 4)
    assert cm.dtype == np.int64 and cm.tolist() == [[1, 2], [3, 4]]  # [[tn, fp], [fn, tp]]


def test_predict_on_an_empty_loader_is_none_and_launches_nothing(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("ops.tta_reduce was called")
    monkeypatch.setattr(E.ops, "tta_reduce", refuse)
    model = torch.nn.Identity().train()
    assert E.predict(model, []) is None and E.predict(model, iter(()), views=5) is None
    assert not model.training
    assert E.call_model(model, 4) == 4


def test_evalpass_imports_none_of_the_modules_that_import_it():
    with open(E.__file__) as f:
        tree = ast.parse(f.read())
    seen = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            base = ("training" if node.level else "") + ("." + node.module if node.module else "")
            seen |= {base.lstrip(".")} | {(base + "." + a.name).lstrip(".") for a in node.names}
        elif isinstance(node, ast.Import):
            seen |= {a.name for a in node.names}
    assert {"numpy", "torch", "dfu_hip"} <= seen
    assert {s.split(".")[0] for s in seen} == {"numpy", "torch", "dfu_hip"}, seen
    assert {s for s in seen if s.startswith("dfu_hip")} == {"dfu_hip", "dfu_hip.ops"}, seen
