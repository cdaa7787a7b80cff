"""Train-mode dropout on the MI355X (dfu_dropout_fwd / dfu_dropout_bwd, hnn.Dropout, DropoutFn)
against the host restatement of its mask stream (dropout_ref.py), from the kernels up to a
captured training step.

The mask is a pure function of (seed, offset + i, p), so masks are compared bit for bit
everywhere.  Values are compared bit for bit too: y = x * scale is one fp32 multiply by
scale = 1 / (1 - p), hipcc's fp32 division is correctly rounded by default and the build sets no
fast-math flag, and the bf16 path rounds that fp32 product to nearest even, as torch's CPU cast
does (a bf16 NaN may carry any payload: same_bits).  Only the head-training test has a
tolerance: the one tests/test_golden_gpu.py uses for the same head with dropout off (fp32
reassociation against an fp64 reference)."""
import numpy as np
import pytest
import torch

import dropout_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
P_TOP = float(np.nextafter(np.float32(1), np.float32(0)))
SEEDS = (0, 1234, 2**63 + 12345, 2**64 - 1)
SIZES = (1, 63, 64, 255, 257, 4097)


def _ops():
    from dfu_hip import ops
    return ops


def bits(t):
    """The tensor's bit pattern as a numpy integer array (NaNs and signed zeros compare)."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]).numpy()


def same_bits(got, ref, what):
    """Bit-for-bit equality.  One exception, bf16 only: where the reference is NaN the result
    must be a NaN, of any encoding.  IEEE 754 leaves a NaN's payload open, and the two casts
    use that freedom: from the fp32 NaN 0x7fc00000 torch's CPU cast (the reference) makes
    0xffff, the hardware's v_cvt_pk_bf16_f32 keeps the quiet NaN 0x7fc0 (both measured;
    test_special_values_kept_and_dropped prints the latter).  fp32 NaNs pass through the
    multiply unchanged and are compared bitwise like everything else."""
    g, r = bits(got).reshape(-1), bits(ref).reshape(-1)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    differ = g != r
    if got.dtype == BF16:
        both_nan = (torch.isnan(got.detach().cpu()) & torch.isnan(ref.detach().cpu())).numpy()
        differ &= ~both_nan.reshape(-1)
    bad = np.flatnonzero(differ)
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} differ, first at {bad[0]}: "
                           f"{int(g[bad[0]]) & 0xFFFFFFFF:#x} vs {int(r[bad[0]]) & 0xFFFFFFFF:#x}")


def inputs(n, dtype, seed):
    """Random normal values of mixed sign with 0.0, -0.0, inf, -inf, nan and the largest finite
    value planted at scattered positions (as many as fit)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g).to(dtype)
    special = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), torch.finfo(dtype).max,
               -torch.finfo(dtype).max]
    reps = max(1, min(32, n // 16))
    pos = torch.randperm(n, generator=g)[:min(n - 1, reps * len(special))] if n > 1 else []
    for j, i in enumerate(pos):
        x[i] = special[j % len(special)]
    return x


def forward(x, p, seed, start):
    """One dfu_dropout_fwd call from counter `start`; checks mask, y and the advanced offset
    against the restatement and returns (y, mask, keep)."""
    n = x.numel()
    off = torch.tensor(start, dtype=torch.int64, device=DEV)
    y, mask = _ops().dropout_fwd(x.to(DEV), p, seed, off)
    k = R.keep(seed, start, n, p)
    what = f"n={n} {x.dtype} p={p} seed={seed:#x} start={start}"
    assert mask.dtype == torch.uint8 and mask.shape == x.shape
    assert np.array_equal(mask.cpu().numpy().reshape(-1), k.astype(np.uint8)), "mask " + what
    same_bits(y, R.apply_torch(x, k, p), "y " + what)
    if x.dtype == F32:  # the numpy float32 reference, independent of torch's CPU multiply
        same_bits(y, torch.from_numpy(R.apply_f32(x.numpy(), k, p)).view(x.shape), "y/np " + what)
    assert off.item() == start + n, what
    return y, mask, k


# ------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("p", [0.0, 0.3, 0.5, 0.7, P_TOP])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_forward_sizes(dtype, p):
    """Mask and y bitwise at sizes below, at and past the wave and block sizes, in both types,
    for every p class: 0 (all kept, y == x bitwise), the three the models use, and the largest
    p < 1 (threshold 2^32 - 256, scale 2^24)."""
    for j, n in enumerate(SIZES):
        x = inputs(n, dtype, seed=100 + n)
        y, mask, k = forward(x, p, SEEDS[j % len(SEEDS)], start=0)
        if p == 0.0:
            assert k.all()
            same_bits(y, x, f"p=0 identity n={n}")


@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: f"{s:#x}")
def test_forward_seeds(seed):
    """The whole 64-bit seed reaches the kernel: 2^63 + 12345 and 2^64 - 1 would change under a
    signed or 32-bit conversion on the ctypes path."""
    for dtype in (F32, BF16):
        forward(inputs(4097, dtype, seed=7), 0.7, seed, start=0)
    low = R.keep(seed & 0xFFFFFFFF, 0, 4097, 0.7)
    if seed >> 32:
        assert not np.array_equal(low, R.keep(seed, 0, 4097, 0.7))


def test_special_values_kept_and_dropped():
    """inf, nan, -0.0 and the largest finite value at kept AND dropped positions: a dropped
    position is exactly +0.0 whatever x was (no 0 * inf = nan), a kept -0.0 stays -0.0."""
    for dtype in (F32, BF16):
        x = inputs(4097, dtype, seed=11)
        y, mask, k = forward(x, 0.5, 1234, start=0)
        yc = y.cpu()
        for sel in (torch.isinf(x), torch.isnan(x), (x == 0) & torch.signbit(x)):
            idx = np.flatnonzero(sel.numpy())
            assert k[idx].any() and not k[idx].all(), "specials must land on both sides"
        dropped = torch.from_numpy(~k)
        assert (bits(yc)[dropped.numpy()] == 0).all()
        kept_nan = torch.isnan(x) & ~dropped
        assert torch.isnan(yc[kept_nan]).all()
        print(f"{dtype}: NaN encodings written:",
              sorted({hex(int(b) & 0xFFFFFFFF) for b in bits(yc)[kept_nan.numpy()]}))


def test_grid_stride_wrap():
    """n = 65536 * 256 + 257: the grid cap of the elementwise launches times the block size plus
    a ragged tail, so 257 threads take a second grid-stride pass."""
    n = 65536 * 256 + 257
    x = torch.randn(n, generator=torch.Generator().manual_seed(5))
    y, mask, k = forward(x, 0.7, 1234, start=0)
    assert abs(k.mean() - 0.3) < 5 * np.sqrt(0.21 / n)


@pytest.mark.parametrize("start,n", [(2**32 - 5, 16), (2**40 + 3, 257)],
                         ids=["cross-2^32", "2^40+3"])
def test_offset_is_64_bit(start, n):
    """offset_dev is read and used as a 64-bit counter: a call whose counters cross 2^32, and
    one far above it, match the restatement and differ from the truncated counter's mask."""
    for dtype in (F32, BF16):
        forward(inputs(n, dtype, seed=3), 0.5, 1234, start)
    truncated = np.concatenate([R.keep(1234, (start + i) & 0xFFFFFFFF, 1, 0.5)
                                for i in range(n)])
    assert not np.array_equal(R.keep(1234, start, n, 0.5), truncated)
    assert not np.array_equal(R.keep(1234, start, n, 0.5), R.keep(1234, 0, n, 0.5))


@pytest.mark.parametrize("p,counter", [(0.3, 219697988), (P_TOP, 206537224),
                                       (P_TOP, 473203049)])
def test_threshold_is_inclusive(p, counter):
    """keep is hash >= threshold: under seed 1234 these counters (found by a host search over
    the restatement) hash to exactly floor(p * 2^32), so the element is kept -- at the largest
    p, where nearly everything is dropped, as the only one of its call.  A kernel comparing
    with > differs from the restatement in one element per 2^32, i.e. only here."""
    assert int(R.hash_u32(1234, counter, 1)[0]) == R.threshold(p)
    for dtype in (F32, BF16):
        x = torch.arange(1, 17).to(dtype)
        y, mask, k = forward(x, p, 1234, start=counter - 7)
        assert k[7] and mask[7].item() == 1 and y[7].item() != 0


def test_continuity():
    """Two calls of 1000 and 777 elements on one offset buffer draw the masks of one call of
    1777 from the same start."""
    ops = _ops()
    seed, p, start = 2**63 + 12345, 0.7, 12345
    x = inputs(1777, F32, seed=9).to(DEV)
    off = torch.tensor(start, dtype=torch.int64, device=DEV)
    y1, m1 = ops.dropout_fwd(x[:1000].contiguous(), p, seed, off)
    assert off.item() == start + 1000
    y2, m2 = ops.dropout_fwd(x[1000:].contiguous(), p, seed, off)
    assert off.item() == start + 1777
    off1 = torch.tensor(start, dtype=torch.int64, device=DEV)
    y, m = ops.dropout_fwd(x, p, seed, off1)
    assert torch.equal(torch.cat([m1, m2]), m)
    same_bits(torch.cat([y1, y2]), y, "two calls vs one")
    assert np.array_equal(m.cpu().numpy(), R.keep(seed, start, 1777, p).astype(np.uint8))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_backward(dtype):
    """dx = where(mask, dy * scale, +0) bitwise with the forward's own mask and a dy that has
    inf and nan of its own; any non-zero mask byte means keep."""
    ops = _ops()
    for n, p in ((1, 0.5), (257, 0.3), (4097, 0.7), (4097, P_TOP), (255, 0.0)):
        x = inputs(n, dtype, seed=21)
        _, mask, k = forward(x, p, 1234, start=77)
        dy = inputs(n, dtype, seed=22 + n)
        dx = ops.dropout_bwd(dy.to(DEV), mask, p)
        assert dx.dtype == dtype
        same_bits(dx, R.apply_torch(dy, k, p), f"dx n={n} p={p}")
        if dtype == F32:
            same_bits(dx, torch.from_numpy(R.apply_f32(dy.numpy(), k, p)), f"dx/np n={n} p={p}")
        dx2 = ops.dropout_bwd(dy.to(DEV), mask * 2, p)
        same_bits(dx2, dx, f"mask bytes 0/2 n={n} p={p}")
        # the mask decides, not dy: another mask gives another dx
        other = torch.from_numpy(R.keep(99, 0, n, 0.5).astype(np.uint8)).to(DEV)
        same_bits(ops.dropout_bwd(dy.to(DEV), other, p),
                  R.apply_torch(dy, other.cpu().numpy().astype(bool), p), "dx, foreign mask")


def test_refusals():
    from dfu_hip import _lib as L
    ops = _ops()
    x = torch.ones(8, device=DEV)
    off = torch.tensor(5, dtype=torch.int64, device=DEV)
    mask = torch.ones(8, dtype=torch.uint8, device=DEV)
    for p in (1.0, -0.1):
        with pytest.raises(L.DfuError, match="dfu_dropout_fwd: bad args") as e:
            ops.dropout_fwd(x, p, 1234, off)
        assert e.value.code == L.DFU_E_INVALID
        with pytest.raises(L.DfuError, match="dfu_dropout_bwd: bad args") as e:
            ops.dropout_bwd(x, mask, p)
        assert e.value.code == L.DFU_E_INVALID
    with pytest.raises(L.DfuError, match="dfu_dropout_fwd: bad args") as e:
        ops.dropout_fwd(x, 0.5, 1234, None)
    assert e.value.code == L.DFU_E_INVALID
    assert off.item() == 5
    # n = 0 with valid pointers (an empty torch tensor's pointer is null, so straight through
    # the C entry points): OK, nothing written, nothing drawn
    y = torch.full((8,), 7.0, device=DEV)
    s = ops.stream_ptr()
    assert L.load().dfu_dropout_fwd(x.data_ptr(), y.data_ptr(), mask.data_ptr(), 0, 0.5, 1234,
                                    off.data_ptr(), 0, s) == L.DFU_OK
    assert L.load().dfu_dropout_bwd(x.data_ptr(), mask.data_ptr(), y.data_ptr(), 0, 0.5, 0,
                                    s) == L.DFU_OK
    assert off.item() == 5 and (y == 7.0).all() and (mask == 1).all()


# ------------------------------------------------------------------- module / training step
class Tap:
    """Forward hooks on every hnn.Dropout of a model: per call, the input and output tensors,
    the rng_offset read before the call, and (through tensor hooks) the gradients at both."""

    def __init__(self, model):
        from dfu_hip import nn as hnn
        self.mods = [m for m in model.modules() if isinstance(m, hnn.Dropout)]
        self.calls = {id(m): [] for m in self.mods}
        for m in self.mods:
            m.register_forward_pre_hook(self._pre)
            m.register_forward_hook(self._post)

    def _pre(self, mod, args):
        mod._tap_start = None if torch.cuda.is_current_stream_capturing() \
            else int(mod.rng_offset.item())

    def _post(self, mod, args, out):
        rec = dict(x=args[0], y=out, start=mod._tap_start)
        if out.requires_grad and out is not args[0]:
            out.register_hook(lambda g, r=rec: r.__setitem__("gy", g.detach().clone()))
            args[0].register_hook(lambda g, r=rec: r.__setitem__("gx", g.detach().clone()))
        self.calls[id(mod)].append(rec)

    def last(self, mod):
        return self.calls[id(mod)][-1]


def test_module_in_fusion_head():
    """hnn.Dropout inside MLPFusion(64, 32, hidden_dims=(48, 40), dropout=0.7), B = 5 (ragged;
    exact-fp32 GEMM path): each layer's output is the restatement of its own input under its
    own seed and running offset, bitwise, and the gradient at its input is the gradient at its
    output times that mask times scale, bitwise (DropoutFn.backward uses its own mask)."""
    from models.fusion import MLPFusion
    torch.manual_seed(3)
    m = MLPFusion(64, 32, num_classes=2, hidden_dims=(48, 40), dropout=0.7).to(DEV).train()
    tap = Tap(m)
    d1, d2 = tap.mods
    assert d1.seed != d2.seed and d1.rng_offset.is_cuda
    rgb = torch.randn(5, 64, device=DEV).abs()
    th = torch.randn(5, 32, device=DEV)
    masks = {}
    for it in range(2):  # the second forward continues each stream at its advanced offset
        out = m(rgb, th)
        (out * torch.randn(5, 2, device=DEV)).sum().backward()
        for d in (d1, d2):
            r = tap.last(d)
            n = r["x"].numel()
            assert r["start"] == it * n and d.rng_offset.item() == (it + 1) * n
            k = R.keep(d.seed, r["start"], n, 0.7)
            same_bits(r["y"], R.apply_torch(r["x"].detach().cpu(), k.reshape(r["x"].shape), 0.7),
                      f"module y, layer n={n}, forward {it}")
            same_bits(r["gx"], R.apply_torch(r["gy"].cpu(), k.reshape(r["x"].shape), 0.7),
                      f"module grad, layer n={n}, forward {it}")
            masks[(id(d), it)] = k
    n1, n2 = 5 * 48, 5 * 40
    assert masks[(id(d1), 0)].size == n1 and masks[(id(d2), 0)].size == n2
    assert not np.array_equal(masks[(id(d1), 0)][:n2], masks[(id(d2), 0)])
    assert not np.array_equal(masks[(id(d1), 0)], masks[(id(d1), 1)])
    # the same counters under the other layer's seed are another mask: had both layers shared a
    # seed, the bitwise comparisons above could not both have held
    assert not np.array_equal(R.keep(d1.seed, 0, n2, 0.7), R.keep(d2.seed, 0, n2, 0.7))


def test_module_identity_modes():
    """.eval() and p = 0 return the input object itself and draw nothing."""
    from dfu_hip import nn as hnn
    x = torch.randn(4, 8, device=DEV, requires_grad=True)
    d = hnn.Dropout(0.7).to(DEV)
    d.train()
    y = d(x)
    assert y is not x and d.rng_offset.item() == 32
    d.eval()
    assert d(x) is x and d.rng_offset.item() == 32
    z = hnn.Dropout(0.0).to(DEV).train()
    assert z(x) is x and z.rng_offset.item() == 0


def _ref_head_step(Ws, bs, rgb, th, labels, cw, keeps, scale):
    """Plain torch fp64 forward of Linear -> ReLU -> dropout (written out) ... -> Linear and the
    weighted CE loss; keeps[i] is the i-th hidden layer's mask (None: no dropout)."""
    h = torch.cat([rgb, th], 1)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ W.t() + b
        if i < len(Ws) - 1:
            h = torch.relu(h)
            if keeps[i] is not None:
                h = h * keeps[i] * scale
    return torch.nn.functional.cross_entropy(h, labels, weight=cw)


def test_head_train_steps_with_dropout():
    """Three training steps of the train-script head at the reference's widths,
    MLPFusion(2048, 768, hidden_dims=(512, 256), dropout=0.5), B = 8, weighted CE, FusedAdamW,
    against plain torch fp64 on the CPU from the same initial weights, whose dropout is
    h * keep * scale with masks from the restatement (each module's seed and running offset).

    Tolerances: those of tests/test_golden_gpu.py::test_head_train_steps for this head with
    dropout off -- loss 1e-5, gradients rtol 1e-5 / atol 1e-7, parameters rtol 1e-6 /
    atol 0.01 lr (fp32 reassociation; Adam turns a near-zero gradient's noise into a visible
    fraction of one step, bounded at 1 % of lr).  The loss must also differ from the
    dropout-free loss by more than its tolerance, so dropout cannot be silently off.

    How the parameter tolerance is applied.  Adam's update lr m^ / (sqrt(v^) + eps) does not
    depend on the gradient's scale, so a gradient of 1e-6 carrying the 1e-7 of fp32 noise the
    gradient check allows moves its element by 10 % of a step whatever computed it: torch's
    own fp32 CPU AdamW against this fp64 reference leaves 0 to 4 of the first layer's 1.44 M
    weights beyond 1 % of lr (up to 2.6 %; six seeds tried).  So, as test_golden_gpu.py does at
    this width, all elements are compared through golden_util.check_array (64 samples, row and
    column sums for arrays above 65536 elements, elementwise below).  On top of that every
    well-conditioned element is compared elementwise at the full tolerance: one whose reference
    gradient in each of the three steps is exactly 0 (a dropped or dead unit: 0 on the GPU as
    well) or at least 1e-4, where noise of 1e-7 + 1e-5 |g| is a relative 1.1e-3 per step and
    cannot add up to 1 % of lr over three steps.  Those are 88 % or more of every tensor
    (asserted above 80 %), and on the CPU experiment they deviated by at most 1e-4 lr."""
    import oracle.golden_inputs as GI
    from golden_util import check_array
    from dfu_hip import nn as hnn
    from dfu_hip.optim import FusedAdamW
    from models.fusion import MLPFusion
    LR, WD, STEPS, B, P = 1e-4, 1e-4, 3, 8, 0.5
    torch.manual_seed(17)
    m = MLPFusion(2048, 768, num_classes=2, hidden_dims=(512, 256), dropout=P)
    lins = [l for l in m.modules() if isinstance(l, hnn.Linear)]
    Ws = [l.weight.detach().double().clone().requires_grad_(True) for l in lins]
    bs = [l.bias.detach().double().clone().requires_grad_(True) for l in lins]
    g = torch.Generator().manual_seed(18)
    rgb = torch.randn(B, 2048, generator=g).abs()  # post-ReLU pooled features
    th = torch.randn(B, 768, generator=g)
    labels = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])
    cw = torch.tensor([1.6, 0.8])
    m = m.to(DEV).train()
    drops = [d for d in m.modules() if isinstance(d, hnn.Dropout)]
    assert len(drops) == 2 and all(d.p == P for d in drops)
    crit = hnn.CrossEntropyLoss(weight=cw.to(DEV))
    opt = FusedAdamW(m.parameters(), lr=LR, weight_decay=WD)
    ropt = torch.optim.AdamW(Ws + bs, lr=LR, weight_decay=WD)
    widths = (512, 256)
    scale = float(R.scale(P))
    rgb_d, th_d, labels_d = rgb.to(DEV), th.to(DEV), labels.to(DEV)
    conditioned = [np.ones(tuple(t.shape), bool) for t in Ws + bs]
    for s in range(STEPS):
        keeps = [torch.from_numpy(R.keep(d.seed, s * B * w, B * w, P).reshape(B, w)).double()
                 for d, w in zip(drops, widths)]
        ropt.zero_grad()
        rloss = _ref_head_step(Ws, bs, rgb.double(), th.double(), labels, cw.double(), keeps,
                               scale)
        rloss.backward()
        with torch.no_grad():
            plain = _ref_head_step(Ws, bs, rgb.double(), th.double(), labels, cw.double(),
                                   [None, None], scale)
        opt.zero_grad()
        loss = crit(m(rgb_d, th_d), labels_d)
        loss.backward()
        print(f"step {s}: loss {loss.item():.7f} ref {rloss.item():.7f} "
              f"dropout-free {plain.item():.7f}")
        assert abs(loss.item() - rloss.item()) < 1e-5, (s, loss.item(), rloss.item())
        assert abs(loss.item() - plain.item()) > 1e-3, "dropout had no effect on the loss"
        if s == 0:
            for i, l in enumerate(lins):
                np.testing.assert_allclose(l.weight.grad.cpu().numpy(), Ws[i].grad.numpy(),
                                           rtol=1e-5, atol=1e-7, err_msg=f"grad{i}w")
                np.testing.assert_allclose(l.bias.grad.cpu().numpy(), bs[i].grad.numpy(),
                                           rtol=1e-5, atol=1e-7, err_msg=f"grad{i}b")
        for c, t in zip(conditioned, Ws + bs):
            a = t.grad.abs().numpy()
            c &= (a == 0) | (a >= 1e-4)
        opt.step()
        ropt.step()
    for d, w in zip(drops, widths):
        assert d.rng_offset.item() == STEPS * B * w
    got = [l.weight for l in lins] + [l.bias for l in lins]
    names = [f"param{i}w" for i in range(3)] + [f"param{i}b" for i in range(3)]
    for name, g, r, c in zip(names, got, Ws + bs, conditioned):
        g, r = g.detach().cpu().numpy().astype(np.float64), r.detach().numpy()
        dev = np.abs(g - r)
        print(f"{name}: {c.mean():.3f} well-conditioned, max deviation "
              f"{dev[c].max(initial=0.0) / LR:.2e} lr there, {dev.max() / LR:.2e} lr anywhere")
        assert c.size < 1000 or c.mean() > 0.8, name
        np.testing.assert_allclose(g[c], r[c], rtol=1e-6, atol=0.01 * LR, err_msg=name)
        fx = {name: r} if r.size <= 65536 else \
            {f"{name}_{k}": v for k, v in GI.summarize(r).items()}
        check_array(fx, name, g, 1e-6, 0.01 * LR)


def test_graph_replay_advances_the_mask():
    """A captured training step (Linear(64, 32) -> ReLU -> Dropout(0.7) -> Linear(32, 2), CE,
    FusedAdamW, static inputs) draws a fresh mask at every replay: after two eager warm-up
    steps, replay r's Dropout output is the restatement of its input at offset (2 + r) n,
    bitwise, the three masks differ, and rng_offset ends at 5 n (the capture executes
    nothing)."""
    import torch.nn as tnn
    from dfu_hip import graphs
    from dfu_hip import nn as hnn
    from dfu_hip.optim import FusedAdamW
    torch.manual_seed(23)
    B, P = 6, 0.7
    drop = hnn.Dropout(P)
    m = tnn.Sequential(hnn.Linear(64, 32), hnn.ReLU(), drop, hnn.Linear(32, 2)).to(DEV).train()
    x = torch.randn(B, 64, device=DEV)
    labels = torch.tensor([0, 1, 1, 0, 1, 0], device=DEV)
    crit = hnn.CrossEntropyLoss(weight=torch.tensor([1.0, 2.0], device=DEV))
    opt = FusedAdamW(m.parameters(), lr=1e-2, weight_decay=1e-2)
    tap = Tap(m)
    n = B * 32

    def step():
        opt.zero_grad()
        crit(m(x), labels).backward()
        opt.step()

    for it in range(2):
        step()
        r = tap.last(drop)
        same_bits(r["y"], R.apply_torch(r["x"].detach().cpu(),
                                        R.keep(drop.seed, it * n, n, P).reshape(B, 32), P),
                  f"eager step {it}")
    torch.cuda.synchronize()
    assert drop.rng_offset.item() == 2 * n
    opt.check_grads = False  # inside a captured graph the gradient pointers are static
    graph = graphs.try_capture(step)
    assert graph is not None, "the training step with dropout must capture"
    torch.cuda.synchronize()
    assert drop.rng_offset.item() == 2 * n, "the capture itself must execute nothing"
    rec = tap.last(drop)
    assert rec["start"] is None  # recorded inside the capture
    masks, xs = [], []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert drop.rng_offset.item() == (3 + r) * n
        xin = rec["x"].detach().cpu().clone()
        k = R.keep(drop.seed, (2 + r) * n, n, P)
        same_bits(rec["y"], R.apply_torch(xin, k.reshape(B, 32), P), f"replay {r}")
        masks.append(k)
        xs.append(xin)
    assert drop.rng_offset.item() == 5 * n
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.array_equal(masks[a], masks[b])
    # the step trains: the Dropout's input moved between replays, so each comparison above was
    # made on that replay's own activations
    assert not torch.equal(xs[0], xs[2])
    # one stale mask would show: the outputs' zero patterns differ where the inputs were alive
    alive = (xs[0] > 0) & (xs[1] > 0)
    assert not np.array_equal((masks[0].reshape(B, 32) & alive.numpy()),
                              (masks[1].reshape(B, 32) & alive.numpy()))
