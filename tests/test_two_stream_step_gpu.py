"""The encoders run on two streams (models.fusion: the ViT on a side stream).  Every kernel of
the step is deterministic (split-K through fp32 slabs, BN statistics by fixed-order merges), so
two training steps with concurrent branches must match two serialized steps BITWISE -- logits,
loss, every gradient and every updated parameter.  A missing stream join or a buffer shared
across streams shows up here as a mismatch.  A failed HIP-graph capture of the step must leave
a process that still runs eager steps (checked in a child process, so a recovery failure cannot
leave this session's streams capturing)."""
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def oracle_state():
    """The oracle's initial weights, built once for every run of this module."""
    torch.manual_seed(0)
    ref = R.MultimodalFusionModel(num_classes=2, dropout=0.0)
    return {k: v.clone() for k, v in ref.state_dict().items()}


def _run(state, concurrent, steps=2):
    from dfu_hip import nn as hnn
    from dfu_hip.optim import FusedAdamW
    from models.fusion import MultimodalFusionModel
    m = MultimodalFusionModel(num_classes=2, dropout=0.0, concurrent_branches=concurrent)
    m.load_state_dict(state)
    m = m.to(DEV).train()
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    rgb, th, y = R.synthetic_batch(8, seed=3)
    rgb, th, y = rgb.to(DEV), th.to(DEV), y.to(DEV)
    crit = hnn.CrossEntropyLoss(weight=torch.tensor([2.0, 2.0], device=DEV))
    outs, grads = [], None
    for _ in range(steps):
        opt.zero_grad()
        out = m(rgb, th)
        loss = crit(out, y)
        loss.backward()
        if grads is None:
            torch.cuda.synchronize()
            grads = {n: p.grad.clone() for n, p in m.named_parameters()}
        opt.step()
        outs.append((out.detach().clone(), loss.detach().clone()))
    torch.cuda.synchronize()
    return outs, grads, {n: p.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("dgelu_colsum", [2, 0])
def test_concurrent_branches_bitwise_equal_to_serial(monkeypatch, oracle_state, dgelu_colsum):
    """functional._DGELU_COLSUM: 2 (the default) takes fc1.bias's gradient from the dGELU
    epilogue's column sums in both schedules, 0 from a colsum pass in both.

    The tile plan is pinned (functional._NO_T192, the DFU_GEMM_NO_T192 switch): a ViT that runs
    alone otherwise takes the 192 x 256 tile for its GEMMs to 768 columns (functional._t768),
    the two-stream step the tuned plan, and the two plans sum K in different orders.  With the
    default plans the serial step's input-gradient GEMMs round differently and every vit.*
    gradient behind them differs (138 of 313 parameters, first vit.cls_token, by up to 1 % of
    its largest element), while each schedule stays bitwise reproducible run to run; that is a
    choice of kernel, not of stream order, so it is taken out of the comparison."""
    from dfu_hip import functional as Fn
    monkeypatch.setattr(Fn, "_DGELU_COLSUM", dgelu_colsum)
    monkeypatch.setattr(Fn, "_NO_T192", True)
    o1, g1, p1 = _run(oracle_state, True)
    o0, g0, p0 = _run(oracle_state, False)
    assert torch.equal(o1[0][0], o0[0][0]) and torch.equal(o1[0][1], o0[0][1]), \
        "logits / loss differ at step 0"
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, f"gradients differ after step 1: {len(bad)} of {len(g0)}: {bad[:8]}"
    assert torch.equal(o1[1][0], o0[1][0]) and torch.equal(o1[1][1], o0[1][1]), \
        "logits / loss differ at step 1"
    bad = [n for n in p0 if not torch.equal(p0[n], p1[n])]
    assert not bad, f"parameters differ after two steps: {len(bad)} of {len(p0)}: {bad[:8]}"


CHILD = textwrap.dedent(r'''
    import json
    import torch
    from oracle import torch_ref as R
    from dfu_hip import functional as Fn
    from dfu_hip import graphs
    from dfu_hip import nn as hnn
    from models.fusion import MultimodalFusionModel
    DEV = "cuda"
    res = {}
    torch.manual_seed(0)
    m = MultimodalFusionModel(num_classes=2, dropout=0.0).to(DEV).train()
    rgb, th, y = R.synthetic_batch(4, seed=3)
    rgb, th, y = rgb.to(DEV), th.to(DEV), y.to(DEV)
    crit = hnn.CrossEntropyLoss(weight=torch.tensor([2.0, 2.0], device=DEV))
    out = {}

    def step():
        m.zero_grad(set_to_none=False)
        loss = crit(m(rgb, th), y)
        loss.backward()
        Fn.join_grad_streams()
        out["loss"] = loss
        return loss
    ref = step().detach().clone()
    torch.cuda.synchronize()

    def bad():
        step()
        raise ValueError("forced failure inside the capture")

    msgs = []
    prev = torch.cuda.current_stream()
    g = graphs.try_capture(bad, log=msgs.append)
    res["failed_capture_returns_none"] = g is None
    res["log"] = msgs[:1]
    res["stream_restored"] = bool(torch.cuda.current_stream() == prev)
    res["not_capturing"] = not torch.cuda.is_current_stream_capturing()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    got = step().detach().clone()
    e1.record()
    torch.cuda.synchronize()
    res["event_ms_positive"] = bool(e0.elapsed_time(e1) > 0)
    res["eager_equal"] = bool(torch.equal(got, ref))
    g = graphs.try_capture(step, log=msgs.append)
    res["good_step_captures"] = g is not None
    if g is not None:
        g.replay()
        torch.cuda.synchronize()
        res["replay_equal"] = bool(torch.equal(out["loss"], ref))
    print("RESULT " + json.dumps(res))
''')


def test_failed_capture_recovers_to_eager():
    """A failed HIP-graph capture -- here a Python ValueError raised inside the captured step
    after its forward and backward were enqueued (it touches no GPU memory and launches
    nothing) -- must leave a process that runs eager steps and HIP-event timing normally (the
    capture stream once stayed current and bench.py crashed in elapsed_time), with the same
    results as before the attempt, and a good step must still capture afterwards."""
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "dfu-multimodal_amd"), root,
                                         env.get("PYTHONPATH", "")])
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0 and line, f"child exited {p.returncode} (a crash, not an exception)"
    res = json.loads(line[0][len("RESULT "):])
    assert res["failed_capture_returns_none"], res
    assert res["log"] and "graph capture failed" in res["log"][0], res
    assert res["stream_restored"] and res["not_capturing"], res
    assert res["event_ms_positive"] and res["eager_equal"], res
    assert res["good_step_captures"] and res["replay_equal"], res
