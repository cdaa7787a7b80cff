"""The parity-mode ("bf16x3") stem and forward kernels (csrc/stem.hip, csrc/precise.hip) at the
shapes the workload never runs: the persistent tile loops and register prefetch of the stem conv
and its weight gradient, every admitted stem geometry and each refusal, LayerNorm / BN apply /
pooling / GELU at partial blocks, single vectors, clipped windows, ties and the tails of erfc.
Every reference is plain torch in fp64 (F.conv2d, F.unfold, F.layer_norm, F.max_pool2d,
torch.special.erfc); another entry point of the library is compared only where "bitwise equal
to the explicit path" is the statement.  Tolerances are those of the named tests of
test_precision_gpu.py unless derived in the docstring."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import close, rnd
from test_precision_gpu import _ops, _pair, _trip

L, ops = _ops()
pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SENT = 7.0  # sentinel of the refusal tests' output buffers


def P_(t):
    return None if t is None else t.data_ptr()


def last_error():
    return (L.load().dfu_last_error_string() or b"").decode()


def _refused(call, *needles):
    """`call` raises DfuError(DFU_E_INVALID) whose text names every needle."""
    with pytest.raises(L.DfuError) as e:
        call()
    assert e.value.code == L.DFU_E_INVALID, e.value
    for n in needles:
        assert n in str(e.value), (n, str(e.value))


def _hi_is_nearest(hi, lo):
    """hi is a bf16 nearest to hi + lo.  (bf16(hi + lo) == hi itself fails for a correct split:
    lo = bf16(v - hi) may round up to exactly half an ulp of hi, hi + lo is then the midpoint of
    two bf16 neighbours and round-to-even leaves an odd hi -- 259 of 262144 normal deviates split
    with torch on the CPU.  Those exact ties are the only exception admitted here.)"""
    s = hi.double() + lo.double()  # exact: both summands lie within the 24 bits of the fp32 v
    r = s.to(BF16)
    tie = (s - hi.double()).abs() == (s - r.double()).abs()
    bad = (r != hi) & ~tie
    assert not bad.any(), f"hi is not the rounding of hi + lo at {int(bad.sum())} elements"


# ------------------------------------------------------------------------------ stem inputs
def _pq(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1  # 7x7 / s2 / p3 (and 3x3 / s2 / p1)


@functools.lru_cache(maxsize=None)
def _stem_x(B, H, W, form="nchw"):
    """x = randn (B, 3, H, W) as NCHW, channels-last (sw = 3) or a view at storage offset 1, and
    the hi im2col rows bf16(unfold(x)) [B*P*Q][147] (the rounding of exact copies)."""
    g = torch.Generator().manual_seed(1000 + 7 * H + W)
    if form == "offset":
        buf = torch.randn(B * 3 * H * W + 1, generator=g).to(DEV)
        x = buf[1:].view(B, 3, H, W)
        assert x.storage_offset() == 1
    else:
        x = torch.randn(B, 3, H, W, generator=g).to(DEV)
        if form == "nhwc":
            x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert x.stride(3) == 3 and x.stride(1) == 1
    col = F.unfold(x.contiguous(), 7, padding=3, stride=2).transpose(1, 2).reshape(-1, 147)
    return x, col.to(BF16)


@functools.lru_cache(maxsize=None)
def _stem_w():
    g = torch.Generator().manual_seed(77)
    return (torch.randn(64, 3, 7, 7, generator=g) * 0.05).to(DEV)


@functools.lru_cache(maxsize=None)
def _stem_case(B, H, W, form="nchw"):
    """-> x, w, the fp64 convolution as rows [B*P*Q][64], the hi im2col rows."""
    x, col = _stem_x(B, H, W, form)
    w = _stem_w()
    ref = F.conv2d(x.double().contiguous(), w.double(), stride=2, padding=3)
    return x, w, ref.permute(0, 2, 3, 1).reshape(-1, 64).contiguous(), col


def _check_conv_pair(y, ylo, ref, what):
    """The conv output pair against the fp64 convolution: test_stem_conv_x3_fused_equals_pair_
    im2col_gemm's bar.  -> delta, the per-element bar."""
    delta = 2e-5 * ref.abs().max().item()
    err = ((y.double() + ylo.double()) - ref).abs().max().item()
    print(f"\n[{what}] max |y + y_lo - fp64 conv| {err:.3e} (bar {delta:.3e})")
    assert err < delta, what
    _hi_is_nearest(y, ylo)
    return delta


def _check_stem_conv(out, ref, colref, what):
    """One dfu_stem_conv_x3 result against the fp64 convolution.

    stats[t] = (sum, M2 about the block mean) of the 128 rows of block t.  With v_i = r_i + e_i,
    |e_i| <= delta (the per-element bar): |sum v - sum r| <= 128 delta, and
    M2(v) - M2(r) = 2 sum (r_i - rbar)(e_i - ebar) + sum (e_i - ebar)^2, where
    sum (e_i - ebar)^2 <= sum e_i^2 <= 128 delta^2 and, by Cauchy-Schwarz, the cross term is at
    most 2 sqrt(M2(r)) sqrt(128) delta: |M2 err| <= 2 delta sqrt(128 M2(r)) + 128 delta^2."""
    y, ylo, st, col, _, _ = out
    M = ref.shape[0]
    delta = _check_conv_pair(y, ylo, ref, what)
    if col is not None:
        assert torch.equal(col[:, :147], colref), what + ": col != bf16(unfold(x))"
        assert (col[:, 147:] == 0).all(), what + ": padded taps of col not zero"
    blk = ref.view(M // 128, 128, 64)
    s_ref = blk.sum(1)
    m2_ref = ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1)
    assert st.shape == (M // 128, 2, 64)
    es = (st[:, 0].double() - s_ref).abs()
    em = (st[:, 1].double() - m2_ref).abs()
    m2_bar = 2 * delta * (128 * m2_ref).sqrt() + 128 * delta ** 2
    print(f"[{what}] stats: sum err {es.max().item():.3e} (bar {128 * delta:.3e}), "
          f"M2 err / bar {(em / m2_bar).max().item():.3e}")
    assert (es <= 128 * delta).all(), what
    assert (em <= m2_bar).all(), what


def _stem_conv_both(x, w, ref, colref, what):
    """want_col True and False: y, y_lo and stats bitwise the same, each checked against fp64."""
    full = ops.stem_conv_x3(x, w, want_col=True)
    bare = ops.stem_conv_x3(x, w, want_col=False)
    assert bare[3] is None and full[4:] == bare[4:] == _pq(x.shape[2], x.shape[3])
    for a, b, n in zip(full[:3], bare[:3], ("y", "y_lo", "stats")):
        assert torch.equal(a, b), f"{what}: {n} differs without col"
    _check_stem_conv(full, ref, colref, what + " col")
    _check_stem_conv(bare, ref, colref, what + " no col")
    return full


# ------------------------------------------------------------------------------ 1. stem conv
# Q = 64: tiles of exactly two rows | W = 250: all 256 staging threads, tiles over three rows |
# H != W, several images | odd H and W (other bottom / right padding) | sw = 3 | offset view
STEM_GEOMS = [(1, 128, 128, "nchw"), (1, 256, 250, "nchw"), (3, 64, 192, "nchw"),
              (2, 63, 159, "nchw"), (1, 128, 128, "nhwc"), (1, 128, 128, "offset")]


@pytest.mark.parametrize("B,H,W,form", STEM_GEOMS)
def test_stem_conv_x3_geometries(B, H, W, form):
    x, w, ref, colref = _stem_case(B, H, W, form)
    _stem_conv_both(x, w, ref, colref, f"stem conv {B}x{H}x{W} {form}")


def test_stem_conv_x3_equals_explicit_path_at_96_columns():
    """test_stem_conv_x3_fused_equals_pair_im2col_gemm's comparison (pair im2col + interleaved-
    pair GEMM: pair and hi rows bitwise, statistics to fp32 summation order) at H != W, B = 3."""
    B, H, W = 3, 64, 192
    x, w, _, _ = _stem_case(B, H, W)
    y, ylo, st, col, Pn, Qn = ops.stem_conv_x3(x, w)
    M = B * Pn * Qn
    (chi, clo), P2, Q2 = ops.im2col_f32_x3(x, 7, 7, 2, 3, 160)
    w3 = ops.split_x3(w.reshape(64, -1), ops.X3_PAIRS, seg=160)
    y2 = torch.empty(M, 64, dtype=BF16, device=DEV)
    y2lo = torch.empty_like(y2)
    st2 = torch.empty(M // 128, 2, 64, device=DEV)
    ops.gemm(M, 64, 320, chi, 160, w3, 320, y2, 64, epilogue=L.EPI_F32_STATS, stats=st2,
             x3=True, a_lo=clo, x3_pairs=True, aux_out=y2lo, ldaux_out=64)
    assert (Pn, Qn) == (P2, Q2) == (32, 96)
    assert torch.equal(col, chi)
    assert torch.equal(y, y2) and torch.equal(ylo, y2lo)
    torch.testing.assert_close(st[:, 0], st2[:, 0], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(st[:, 1], st2[:, 1], rtol=1e-4, atol=1e-3)


def test_stem_conv_x3_persistent_loop_and_prefetch():
    """More tiles than the 2 * CUs workgroups, and no multiple of them: some workgroups take two
    tiles (the t += gridDim.x loop, the prefetched rows handed over at the loop top) and some
    one.  The fp64 checks as above; and image b of the batch is bitwise image b run alone (B = 1,
    where no workgroup takes a second tile): a stale or mixed-up prefetch register would show."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H = W = 128
    B = 2 * cus // 32 + 1
    tiles = B * 64 * 64 // 128
    assert tiles > 2 * cus and tiles % (2 * cus) != 0, (tiles, cus)
    x, w, ref, colref = _stem_case(B, H, W)
    y, ylo, st, col, _, _ = _stem_conv_both(x, w, ref, colref, f"stem conv persistent B={B}")
    for b in (0, B // 2, B - 1):
        y1, ylo1, st1, col1, _, _ = ops.stem_conv_x3(x[b:b + 1], w)
        r = slice(b * 4096, (b + 1) * 4096)
        assert torch.equal(y[r], y1) and torch.equal(ylo[r], ylo1), b
        assert torch.equal(col[r], col1), b
        assert torch.equal(st[b * 32:(b + 1) * 32], st1), b


@pytest.mark.parametrize("H,W,needles", [(128, 120, ("Q >= 64", "Q=60")),
                                         (130, 128, ("128 == 0", "P=65 Q=64")),
                                         (128, 252, ("W <= 250", "P=64 Q=126"))])
def test_stem_conv_x3_refusals(H, W, needles):
    """Q = 60; P*Q = 4160; W = 252 alone (P*Q = 8064 = 63 * 128): DFU_E_INVALID from the host
    check, the condition named, nothing written."""
    lib = L.load()
    B = 1
    Pn, Qn = _pq(H, W)
    M = B * Pn * Qn
    x = torch.zeros(B, 3, H, W, device=DEV)
    w = _stem_w()
    y = torch.full((M, 64), SENT, dtype=BF16, device=DEV)
    ylo = torch.full((M, 64), SENT, dtype=BF16, device=DEV)
    st = torch.full((M // 128 + 1, 2, 64), SENT, device=DEV)
    col = torch.full((M, 160), SENT, dtype=BF16, device=DEV)
    for c in (col, None):
        rc = lib.dfu_stem_conv_x3(P_(x), *x.stride(), B, 3, H, W, P_(w), 64, 7, 7, 2, 3, P_(y),
                                  P_(ylo), P_(st), P_(c), ops.stream_ptr())
        assert rc == L.DFU_E_INVALID, rc
        for n in needles:
            assert n in last_error(), (n, last_error())
    _refused(lambda: ops.stem_conv_x3(x, w), *needles)
    torch.cuda.synchronize()
    for t in (y, ylo, st, col):
        assert (t == SENT).all()


# ------------------------------------------------------------------------------ 2. stem wgrad
# (B, H, W, form, G = the grid and slab count): G = 2 | 17: the reduce's 16-stride tail only |
# 48: g + 48 < G false for every slice | 49: one unrolled pass for slice 0 | 64 | 65: unrolled
# pass + tail | Q = 112 (the widest tile) even and odd W | odd H and W, Q = 80 | sw = 3 | offset
WGRAD_GEOMS = [(1, 7, 32, "nchw", 2), (1, 68, 32, "nchw", 17), (1, 192, 32, "nchw", 48),
               (7, 28, 32, "nchw", 49), (1, 256, 32, "nchw", 64), (1, 260, 32, "nchw", 65),
               (1, 8, 224, "nchw", 2), (1, 8, 223, "nchw", 2), (2, 63, 159, "nchw", 32),
               (1, 128, 128, "nhwc", 32), (1, 128, 128, "offset", 32)]


def _wgrad_inputs(M, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    dy = (torch.randn(M, 64, generator=g) * 0.1).to(BF16).to(DEV)
    d0 = torch.randn(64, 147, generator=g).to(DEV)
    return dy, d0


def _check_wgrad(dw, d0, dy, colref, M, what):
    """test_stem_wgrad_x3_from_x_equals_im2col_gemm's bar (1e-5 of max |dw - d0|, set at
    M = 25088) against d0 + dy^T bf16(unfold(x)) in fp64; scaled by M / 25088 above that M (the
    worst-case fp32 accumulation error grows linearly with the number of summands)."""
    exact = d0.double() + dy.double().t() @ colref.double()
    err = ((dw.double() - exact).abs().max() / (exact - d0.double()).abs().max()).item()
    bar = 1e-5 * max(1.0, M / 25088)
    print(f"\n[{what}] M={M} rel err vs fp64 sum {err:.3e} (bar {bar:.3e})")
    assert err < bar, what


@pytest.mark.parametrize("B,H,W,form,G", WGRAD_GEOMS)
def test_stem_wgrad_x3_geometries(B, H, W, form, G):
    x, colref = _stem_x(B, H, W, form)
    Pn, Qn = _pq(H, W)
    M = B * Pn * Qn
    assert min(B * Pn // 2, 512) == G
    assert L.load().dfu_stem_wgrad_ws_bytes(B, H, W) == G * 64 * 147 * 4
    dy, d0 = _wgrad_inputs(M)
    dw = d0.clone()
    ops.stem_wgrad_x3(x, dy, dw)
    _check_wgrad(dw, d0, dy, colref, M, f"stem wgrad {B}x{H}x{W} {form}")
    dw2 = d0.clone()
    ops.stem_wgrad_x3(x, dy, dw2)
    assert torch.equal(dw, dw2)  # deterministic


def test_stem_wgrad_x3_persistent_loop():
    """544 two-row tiles on the 512 workgroups: 32 of them take a second tile (the loop and the
    prefetched x / dy registers handed over)."""
    B, H, W = 17, 128, 128
    Pn, Qn = _pq(H, W)
    assert B * Pn // 2 > 512
    M = B * Pn * Qn
    x, colref = _stem_x(B, H, W)
    assert L.load().dfu_stem_wgrad_ws_bytes(B, H, W) == 512 * 64 * 147 * 4
    dy, d0 = _wgrad_inputs(M, seed=1)
    dw = d0.clone()
    ops.stem_wgrad_x3(x, dy, dw)
    _check_wgrad(dw, d0, dy, colref, M, "stem wgrad persistent")
    dw2 = d0.clone()
    ops.stem_wgrad_x3(x, dy, dw2)
    assert torch.equal(dw, dw2)


def test_stem_wgrad_x3_refuses_short_slab():
    lib = L.load()
    B, H, W = 1, 68, 32
    x, _ = _stem_x(B, H, W)
    dy, d0 = _wgrad_inputs(B * 34 * 16)
    dw = d0.clone()
    nbytes = lib.dfu_stem_wgrad_ws_bytes(B, H, W)
    slab = torch.full((nbytes // 4,), SENT, device=DEV)
    rc = lib.dfu_stem_wgrad_x3(P_(x), *x.stride(), B, 3, H, W, P_(dy), 64, 7, 7, 2, 3, P_(dw),
                               P_(slab), nbytes - 1, ops.stream_ptr())
    assert rc == L.DFU_E_INVALID and "slab" in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    assert torch.equal(dw, d0) and (slab == SENT).all()


@pytest.mark.parametrize("H,W,shift,needle", [(10, 32, 0, "P=5"), (8, 48, 0, "Q=24"),
                                              (8, 240, 0, "Q=120"), (8, 32, 1, "aligned")])
def test_stem_wgrad_x3_refusals(H, W, shift, needle):
    """P odd; Q % 16 != 0; Q > 112; dy one element off its 16-byte alignment: dw untouched."""
    B = 1
    Pn, Qn = _pq(H, W)
    M = B * Pn * Qn
    x = torch.zeros(B, 3, H, W, device=DEV)
    dyb, d0 = _wgrad_inputs(M + 1)
    dy = dyb.view(-1)[shift:shift + M * 64].view(M, 64)
    dw = d0.clone()
    _refused(lambda: ops.stem_wgrad_x3(x, dy, dw), needle)
    torch.cuda.synchronize()
    assert torch.equal(dw, d0)


# ------------------------------------------------------------------------------ 3. predicate
SWEEP_HW = sorted({(h, w) for _, h, w, _ in STEM_GEOMS} | {(h, w) for _, h, w, _, _ in WGRAD_GEOMS}
                  | {(128, 120), (130, 128), (128, 252), (10, 32), (8, 48), (8, 240), (64, 120)})


@pytest.mark.parametrize("H,W", SWEEP_HW)
def test_stem_conv_x3_ok_is_both_entry_points(H, W):
    """ops.stem_conv_x3_ok (what StemFn asks before it takes the fused conv, whose backward then
    needs the fused weight gradient) is True exactly when dfu_stem_conv_x3 and dfu_stem_wgrad_x3
    both accept the geometry."""
    B = 1
    Pn, Qn = _pq(H, W)
    x = torch.zeros(B, 3, H, W, device=DEV)
    w = _stem_w()
    dy = torch.zeros(B * Pn * Qn, 64, dtype=BF16, device=DEV)
    dw = torch.zeros(64, 147, device=DEV)

    def accepts(call):
        try:
            call()
            return True
        except L.DfuError as e:
            assert e.code == L.DFU_E_INVALID
            return False

    conv_ok = accepts(lambda: ops.stem_conv_x3(x, w, want_col=False))
    wgrad_ok = accepts(lambda: ops.stem_wgrad_x3(x, dy, dw))
    assert ops.stem_conv_x3_ok(x, w, 2, 3) == (conv_ok and wgrad_ok), (conv_ok, wgrad_ok)


def test_stem_function_explicit_fallback(monkeypatch):
    """(2, 64, 120): Q = 60, the predicate says no and StemFn (parity mode) runs the explicit
    path -- pair im2col + interleaved-pair GEMM forward, MN-major GEMM over the hi im2col rows
    backward.  The conv output pair it hands to the pool and the conv1 weight gradient it leaves
    are checked with the bars of the fused kernels: the pair against the fp64 convolution,
    weight.grad against dy^T bf16(unfold(x)) in fp64 of the very dy the backward produced (both
    operands observed at the library's internal call, not recomputed)."""
    from dfu_hip import functional as Fn
    from models.resnet import ResNet
    B, H, W = 2, 64, 120
    x, w, ref, colref = _stem_case(B, H, W)
    torch.manual_seed(5)
    net = ResNet(layers=(1, 1, 1, 1)).to(DEV).train()
    with torch.no_grad():
        net.conv1.weight.copy_(w)
        net.bn1.weight.uniform_(0.5, 1.5)
        net.bn1.bias.uniform_(-0.5, 0.5)
    assert Fn.get_precision() == "parity" and not ops.stem_conv_x3_ok(x, w, 2, 3)
    seen = {}
    pool, wgrad = ops.maxpool_bn_fwd_x3, Fn.im2col_conv_wgrad

    def pool_spy(y, y_lo, *a, **kw):
        seen["pair"] = (y, y_lo)
        return pool(y, y_lo, *a, **kw)

    def wgrad_spy(dy, col, *a, **kw):
        seen["wgrad"] = (dy.clone(), col)
        return wgrad(dy, col, *a, **kw)

    monkeypatch.setattr(ops, "maxpool_bn_fwd_x3", pool_spy)
    monkeypatch.setattr(Fn, "im2col_conv_wgrad", wgrad_spy)
    out = Fn.StemFn.apply(x, net.conv1.weight, net.bn1.weight, net.bn1.bias, net)
    assert out.shape == (B, 64, 16, 30) and torch.isfinite(out.float()).all()
    g = rnd(B, 16, 30, 64, seed=6).permute(0, 3, 1, 2)  # bf16 channels_last
    out.backward(g)
    torch.cuda.synchronize()
    y, ylo = seen["pair"]
    _check_conv_pair(y, ylo, ref, "StemFn explicit path")
    dy, col = seen["wgrad"]  # reaching the explicit weight gradient is the fallback itself
    assert torch.equal(col[:, :147], colref)
    M = B * 32 * 60
    assert dy.shape == (M, 64) and dy.dtype == BF16
    _check_wgrad(net.conv1.weight.grad.view(64, 147), torch.zeros(64, 147, device=DEV), dy,
                 colref, M, "StemFn explicit wgrad")


# ------------------------------------------------------------------------------ 4. LayerNorm
# one row, one vector | two full chunks per lane, a partial last block | D/8 = 33 lanes, ldx > D
# | D/8 = 65: one lane takes a second chunk | the workload's width, strided, a partial block
LN_CASES = [(1, 8, 8), (5, 1024, 1024), (33, 264, 268), (7, 520, 520), (6, 768, 772)]
LN_EPS = 1e-6


@functools.lru_cache(maxsize=None)
def _ln_case(rows, D, ld):
    g = torch.Generator().manual_seed(400 + D)
    x = (torch.randn(rows, ld, generator=g) * 3 + 1).to(DEV)[:, :D]
    gamma = torch.randn(D, generator=g).to(DEV)
    beta = torch.randn(D, generator=g).to(DEV)
    xd = x.double()
    ref = F.layer_norm(xd, (D,), gamma.double(), beta.double(), LN_EPS)
    mean = xd.mean(1)
    rstd = (xd.var(1, unbiased=False) + LN_EPS).rsqrt()
    return x, gamma, beta, ref, mean, rstd


def _check_ln_moments(x, mean, rstd, mean_ref, rstd_ref, D):
    """mean: 16 sequential adds per lane and a 6-level wave tree round at most 22 times, each
    within U of a partial sum of magnitude <= sum |x|; the division once more: 24 U sum|x| / D.
    rstd: the variance is a sum of positive terms, so the same 22 roundings plus those of d = x -
    mean and d * d stay relative, about 25 U; the square root halves that, and sqrtf, the
    division by D, the eps add and the reciprocal add one each: well inside 32 U relative."""
    tol = 24 * U * x.double().abs().sum(1) / D
    em = (mean.double() - mean_ref).abs()
    er = ((rstd.double() - rstd_ref).abs() / rstd_ref)
    print(f"\n[ln moments D={D}] mean err / bar {(em / tol).max().item():.3f}, "
          f"rstd rel err {er.max().item() / U:.2f} U")
    assert (em <= tol).all()
    assert (er <= 32 * U).all()


@pytest.mark.parametrize("rows,D,ld", LN_CASES)
def test_layernorm_fwd_x3_shapes(rows, D, ld):
    """test_layernorm_and_gelu_x3's bar for hi + lo; the bf16 copy is the hi segment, the third
    segment the first; mean and rstd (the backward's inputs) against fp64."""
    x, gamma, beta, ref, mean_ref, rstd_ref = _ln_case(rows, D, ld)
    o3 = torch.full((rows, 3 * D), SENT, dtype=BF16, device=DEV)
    ob = torch.full((rows, D), SENT, dtype=BF16, device=DEV)
    mean = torch.full((rows,), SENT, device=DEV)
    rstd = torch.full((rows,), SENT, device=DEV)
    ops.layernorm_fwd_x3(x, ld, rows, D, gamma, beta, LN_EPS, o3, ob, mean, rstd)
    v, _, _ = _trip(o3, D)
    err = (v.double() - ref).abs().max().item()
    rmax = ref.abs().max().item()
    print(f"\n[ln x3 {rows}x{D} ld {ld}] max err {err:.3e} (max |ref| {rmax:.2f})")
    assert err < 2e-5 * rmax
    assert torch.equal(ob, o3[:, :D]) and torch.equal(o3[:, 2 * D:], o3[:, :D])
    _check_ln_moments(x, mean, rstd, mean_ref, rstd_ref, D)


@pytest.mark.parametrize("rows,D,ld", LN_CASES)
def test_layernorm_fwd_h16_shapes(rows, D, ld):
    """One fp16 (2**-11) or bf16 (2**-8) rounding of the fp32 value, which is within the x3
    bar of fp64."""
    x, gamma, beta, ref, mean_ref, rstd_ref = _ln_case(rows, D, ld)
    o16 = torch.full((rows, D), SENT, dtype=F16, device=DEV)
    ob = torch.full((rows, D), SENT, dtype=BF16, device=DEV)
    mean = torch.full((rows,), SENT, device=DEV)
    rstd = torch.full((rows,), SENT, device=DEV)
    ops.layernorm_fwd_h16(x, ld, rows, D, gamma, beta, LN_EPS, o16, ob, mean, rstd)
    slack = 2e-5 * ref.abs().max().item()
    assert ((o16.double() - ref).abs() <= 2.0 ** -11 * ref.abs() + slack).all()
    assert ((ob.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + slack).all()
    _check_ln_moments(x, mean, rstd, mean_ref, rstd_ref, D)


@pytest.mark.parametrize("D,ld", [(1032, 1032), (12, 12), (8, 10)])
def test_layernorm_x3_refusals(D, ld):
    """D > 1024, D % 8 != 0, a row stride that breaks the 16-byte loads: both entry points return
    DFU_E_INVALID and write nothing."""
    rows = 3
    x = torch.zeros(rows, ld, device=DEV)[:, :D]
    gamma = torch.ones(D, device=DEV)
    o3 = torch.full((rows, 3 * D), SENT, dtype=BF16, device=DEV)
    o16 = torch.full((rows, D), SENT, dtype=F16, device=DEV)
    ob = torch.full((rows, D), SENT, dtype=BF16, device=DEV)
    mean = torch.full((rows,), SENT, device=DEV)
    rstd = torch.full((rows,), SENT, device=DEV)
    _refused(lambda: ops.layernorm_fwd_x3(x, ld, rows, D, gamma, gamma, LN_EPS, o3, ob, mean,
                                          rstd), "dfu_layernorm_fwd_x3")
    _refused(lambda: ops.layernorm_fwd_h16(x, ld, rows, D, gamma, gamma, LN_EPS, o16, ob, mean,
                                           rstd), "dfu_layernorm_fwd_h16")
    torch.cuda.synchronize()
    for t in (o3, o16, ob, mean, rstd):
        assert (t == SENT).all()


# ------------------------------------------------------------------------------ 5. BN apply
def _mask_bits(mask, M, C):
    return ((mask.view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).view(M, C) > 0


def _bn_inputs(M, C):
    g = torch.Generator().manual_seed(500 + M + C)
    y = torch.randn(M, C, generator=g).to(DEV)
    sc = (torch.rand(C, generator=g) + 0.5).to(DEV)
    sh = torch.randn(C, generator=g).to(DEV)
    res = torch.randn(M, C, generator=g).to(DEV)
    return y, sc, sh, res


# one vector in all | one vector per row, a partial block | 256 vectors per row | 1032 vectors:
# four blocks and a tail of 8
BN_CASES = [(1, 8), (37, 8), (300, 2048), (129, 64)]


@pytest.mark.parametrize("M,C", BN_CASES)
def test_bn_apply_x3_shapes_relu_and_residual_modes(M, C):
    """test_bn_apply_x3_residual_modes' tolerances and identities (against fp64 here), relu 0 and
    1, the three residual modes, y as fp32 and as a split pair; with relu = 0 the bitmask still
    reports out > 0.  Buffers that are not requested are passed as None."""
    y, sc, sh, res = _bn_inputs(M, C)
    rhi, rlo = _pair(res)
    yh, yl = _pair(y)

    def new(dtype=BF16):
        return torch.full((M, C), SENT, dtype=dtype, device=DEV)

    for relu in (0, 1):
        for mode, r, rl in ((0, None, None), (1, res, None), (2, rhi, rlo)):
            what = f"M={M} C={C} relu={relu} mode={mode}"
            ref = y.double() * sc.double() + sh.double() + (res.double() if mode else 0)
            if relu:
                ref = ref.clamp_min(0)
            lo, ob, of, yb = new(), new(), new(F32), new()
            mask = torch.full((M * C // 8,), 0xAA, dtype=torch.uint8, device=DEV)
            ops.bn_apply_x3(y, sc, sh, r, mode, relu, M, C, out_lo=lo, out_bf16=ob, out_f32=of,
                            y_bf16=yb, residual_lo=rl, relu_mask=mask)
            tol = 2e-6 if mode != 2 else 2e-5  # the pair residual carries 16 mantissa bits
            close(of.double(), ref, atol=tol, rtol=tol, what=what)
            assert ((ob.float() + lo.float() - of).abs() <= of.abs() * 2.0 ** -16).all(), what
            assert torch.equal(ob, of.to(BF16)), what
            assert torch.equal(yb, y.to(BF16)), what
            assert torch.equal(_mask_bits(mask, M, C), of > 0), what
            if not relu:
                assert (of < 0).any() or M * C < 16
            # y as a split pair (the conv epilogue's form)
            lo2, ob2 = new(), new()
            mask2 = torch.full((M * C // 8,), 0xAA, dtype=torch.uint8, device=DEV)
            ops.bn_apply_x3(yh, sc, sh, r, mode, relu, M, C, out_lo=lo2, out_bf16=ob2,
                            residual_lo=rl, y_lo=yl, relu_mask=mask2)
            v2 = ob2.float() + lo2.float()
            close(v2.double(), ref, atol=3e-5, rtol=3e-5, what=what + " pair y")
            assert torch.equal(_mask_bits(mask2, M, C), v2 > 0), what


@pytest.mark.parametrize("M,C", BN_CASES)
def test_bn_apply_x3_output_subsets(M, C):
    """out_f32 alone; out_bf16 without out_lo (one bf16 rounding, 2**-8, of the fp32 result);
    everything but y_bf16."""
    y, sc, sh, res = _bn_inputs(M, C)
    ref = (y.double() * sc.double() + sh.double() + res.double()).clamp_min(0)
    tol = 2e-6
    of = torch.full((M, C), SENT, device=DEV)
    ops.bn_apply_x3(y, sc, sh, res, 1, 1, M, C, out_f32=of)
    close(of.double(), ref, atol=tol, rtol=tol, what="out_f32 only")
    ob = torch.full((M, C), SENT, dtype=BF16, device=DEV)
    ops.bn_apply_x3(y, sc, sh, res, 1, 1, M, C, out_bf16=ob)
    assert torch.equal(ob, of.to(BF16))
    assert ((ob.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + tol * (1 + ref.abs())).all()
    lo = torch.full((M, C), SENT, dtype=BF16, device=DEV)
    ob2 = torch.full((M, C), SENT, dtype=BF16, device=DEV)
    of2 = torch.full((M, C), SENT, device=DEV)
    ops.bn_apply_x3(y, sc, sh, res, 1, 1, M, C, out_lo=lo, out_bf16=ob2, out_f32=of2)
    close(of2.double(), ref, atol=tol, rtol=tol, what="no y_bf16")
    assert torch.equal(ob2, of2.to(BF16))
    assert ((ob2.float() + lo.float() - of2).abs() <= of2.abs() * 2.0 ** -16).all()


def test_bn_apply_x3_refusals():
    """C / 8 = 3 (no power of two); out_lo without out_bf16; scale one float off its 16-byte
    alignment: DFU_E_INVALID, nothing written."""
    M = 16
    outs = []

    def new(C, dtype=BF16):
        outs.append(torch.full((M, C), SENT, dtype=dtype, device=DEV))
        return outs[-1]

    y24, s24 = torch.zeros(M, 24, device=DEV), torch.ones(24, device=DEV)
    _refused(lambda: ops.bn_apply_x3(y24, s24, s24, None, 0, 1, M, 24, out_f32=new(24, F32)),
             "power of two", "C=24")
    y, s = torch.zeros(M, 64, device=DEV), torch.ones(64, device=DEV)
    _refused(lambda: ops.bn_apply_x3(y, s, s, None, 0, 1, M, 64, out_lo=new(64),
                                     out_f32=new(64, F32)), "dfu_bn_apply_x3")
    soff = torch.ones(65, device=DEV)[1:]
    _refused(lambda: ops.bn_apply_x3(y, soff, s, None, 0, 1, M, 64, out_f32=new(64, F32)),
             "aligned")
    torch.cuda.synchronize()
    for t in outs:
        assert (t == SENT).all()


# ------------------------------------------------------------------------------ 6. max pool
# a single clipped 1x1 window | windows of 2x2 and 2x2 | odd x even | the odd sizes of
# test_maxpool_bn_fused_x3_equals_apply_then_pool
POOL_CASES = [(1, 1, 1, 8), (2, 2, 3, 8), (2, 7, 8, 64), (3, 15, 9, 64)]


def _pool_ref(x):
    """fp64 F.max_pool2d(3, 2, 1) of CPU NHWC x -> pooled NHWC (with autograd to the returned
    NCHW leaf), torch's argmax as the library's window index (ih - (2p - 1)) * 3 + (iw -
    (2q - 1)) [B][P][Q][C], and the leaf."""
    B, H, W, C = x.shape
    Pn, Qn = _pq(H, W)
    leaf = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out, idx = F.max_pool2d(leaf, 3, 2, 1, return_indices=True)
    assert out.shape == (B, C, Pn, Qn)
    ih, iw = idx // W, idx % W
    p = torch.arange(Pn).view(1, 1, Pn, 1)
    q = torch.arange(Qn).view(1, 1, 1, Qn)
    am = (ih - (2 * p - 1)) * 3 + (iw - (2 * q - 1))
    assert am.min() >= 0 and am.max() <= 8
    return out.permute(0, 2, 3, 1), am.permute(0, 2, 3, 1).to(torch.uint8), leaf


def _pool_top2_gap(x):
    """Per output of the 3x3/s2/p1 pool of CPU NHWC fp64 x: (the largest window value, its
    distance to the second largest; inf for a window of one element)."""
    B, H, W, C = x.shape
    Pn, Qn = _pq(H, W)
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=-math.inf)
    win = F.unfold(xp, 3, stride=2).view(B, C, 9, Pn, Qn)
    top = win.topk(2, dim=2).values
    return top[:, :, 0].permute(0, 2, 3, 1), (top[:, :, 0] - top[:, :, 1]).permute(0, 2, 3, 1)


@pytest.mark.parametrize("B,H,W,C", POOL_CASES)
def test_maxpool_fwd_x3_clipped_windows_and_ties(B, H, W, C):
    """Multiples of 0.25 in [-1, 1] (ties in most windows, every value a bf16): the pooled pair is
    exact, the argmax is torch's (the first maximum in row-major window order), and
    dfu_maxpool_bwd fed with it is torch's backward within one bf16 rounding (2**-8) of the fp64
    sum of the up to four windows an input pixel wins."""
    g = torch.Generator().manual_seed(600 + H * W)
    x = torch.randint(-4, 5, (B, H, W, C), generator=g).float() / 4
    ref, am_ref, leaf = _pool_ref(x)
    ylo, yb, am, Pn, Qn = ops.maxpool_fwd_x3(x.to(DEV).reshape(-1, C), B, H, W, C)
    assert (Pn, Qn) == _pq(H, W)
    assert torch.equal(yb.cpu(), ref.detach().to(BF16))
    v = yb.double().reshape(-1, C) + ylo.double()
    assert torch.equal(v.cpu().view(B, Pn, Qn, C), ref.detach())
    assert torch.equal(am.cpu(), am_ref)
    dy = rnd(B, Pn, Qn, C, seed=601)
    ref.backward(dy.double().cpu())
    dx = ops.maxpool_bwd(dy.reshape(-1, C), am, B, H, W, C, Pn, Qn)
    dref = leaf.grad.permute(0, 2, 3, 1)
    assert ((dx.double().cpu() - dref).abs() <= 2.0 ** -8 * dref.abs()).all()


def test_maxpool_fwd_x3_continuous_input_odd_sizes():
    """test_maxpool_and_avgpool_x3's comparison with torch at (3, 15, 9, 64)."""
    B, H, W, C = 3, 15, 9, 64
    g = torch.Generator().manual_seed(610)
    x = torch.randn(B, H, W, C, generator=g)
    ref, am_ref, _ = _pool_ref(x)
    ref = ref.detach()
    ylo, yb, am, Pn, Qn = ops.maxpool_fwd_x3(x.to(DEV).reshape(-1, C), B, H, W, C)
    v = (yb.double().reshape(-1, C) + ylo.double()).cpu().view(B, Pn, Qn, C)
    assert torch.allclose(v, ref, rtol=2e-5, atol=0)
    assert torch.equal(yb.cpu(), ref.to(BF16))
    assert torch.equal(am.cpu(), am_ref)


POOL_BAR = 3e-5  # test_bn_apply_x3_residual_modes' bar for a pair y, as rtol and atol
POOL_SEED = 620


def _fused_pool_inputs(B, H, W, C):
    """CPU: y [B*H*W][C] fp32, scale, shift, and the fp64 relu(y * scale + shift) as NHWC.  The
    shift has mean 0.5: a third of the pre-activations are negative, but few windows are zero
    throughout (with mean 0 such windows alone are 5.5% of the outputs of the largest case).  The
    fp64 reference by itself leaves out 0, 0, 0.9% and 1.1% of the four cases' outputs."""
    g = torch.Generator().manual_seed(POOL_SEED + H * W)
    y = torch.randn(B * H * W, C, generator=g)
    sc = torch.rand(C, generator=g) + 0.5
    sh = torch.randn(C, generator=g) * 0.5 + 0.5
    a = (y.double() * sc.double() + sh.double()).clamp_min(0).view(B, H, W, C)
    return y, sc, sh, a


def _near_tie(a):
    """Outputs whose two largest window values of the fp64 reference `a` lie within POOL_BAR."""
    top, gap = _pool_top2_gap(a)
    return gap <= POOL_BAR * (1 + top.abs())


@pytest.mark.parametrize("B,H,W,C", POOL_CASES)
def test_maxpool_bn_fwd_x3_clipped_windows(B, H, W, C):
    """The fused bn1 + ReLU + pool over a pair against torch's pool of the fp64 relu(y * scale +
    shift).  The argmax is compared where the two largest window values differ by more than the
    value bar (windows that ReLU left all zero tie exactly); at most 5% of the outputs may be
    left out that way.  Pair, argmax and ReLU bitmask are also bitwise the two-kernel path's
    (test_maxpool_bn_fused_x3_equals_apply_then_pool's statement) at these shapes."""
    y, sc, sh, a = _fused_pool_inputs(B, H, W, C)
    ref, am_ref, _ = _pool_ref(a)
    ref = ref.detach()
    near = _near_tie(a)
    assert near.float().mean().item() <= 0.05, near.float().mean().item()
    hi, lo = _pair(y.to(DEV))
    scd, shd = sc.to(DEV), sh.to(DEV)
    M = B * H * W
    mask = torch.full((M * C // 8,), 0xAA, dtype=torch.uint8, device=DEV)
    lo_f, out_f, am_f, Pn, Qn = ops.maxpool_bn_fwd_x3(hi, lo, scd, shd, B, H, W, C, relu_mask=mask)
    v = (out_f.double().reshape(-1, C) + lo_f.double()).cpu().view(B, Pn, Qn, C)
    close(v, ref, atol=POOL_BAR, rtol=POOL_BAR, what="fused pool value")
    _hi_is_nearest(out_f.reshape(-1, C), lo_f)
    assert torch.equal(am_f.cpu()[~near], am_ref[~near])
    # the two-kernel path: dfu_bn_apply_x3 (fp32 out, bitmask) then dfu_maxpool_fwd_x3
    af = torch.empty(M, C, device=DEV)
    mask_ref = torch.empty_like(mask)
    ops.bn_apply_x3(hi, scd, shd, None, 0, True, M, C, out_f32=af, y_lo=lo, relu_mask=mask_ref)
    lo_r, out_r, am_r, _, _ = ops.maxpool_fwd_x3(af, B, H, W, C)
    assert torch.equal(out_f, out_r) and torch.equal(lo_f, lo_r) and torch.equal(am_f, am_r)
    assert torch.equal(mask, mask_ref)


def test_maxpool_entry_points_refuse_wrong_output_size():
    """dfu_maxpool_fwd_x3 and dfu_maxpool_bwd check P and Q against H and W (as dfu_maxpool_bn_fwd
    always did): a P or Q one too large would read and write past the buffers."""
    lib = L.load()
    B, H, W, C = 1, 7, 8, 8
    Pn, Qn = _pq(H, W)
    s = ops.stream_ptr()
    x = torch.zeros(B * H * W, C, device=DEV)
    n = B * (Pn + 1) * (Qn + 1)
    lo = torch.full((n, C), SENT, dtype=BF16, device=DEV)
    yb = torch.full((n, C), SENT, dtype=BF16, device=DEV)
    am = torch.full((n, C), 9, dtype=torch.uint8, device=DEV)
    dx = torch.full((B * H * W, C), SENT, dtype=BF16, device=DEV)
    for p, q in ((Pn + 1, Qn), (Pn, Qn + 1), (Pn - 1, Qn)):
        rc = lib.dfu_maxpool_fwd_x3(P_(x), B, H, W, C, P_(lo), P_(yb), P_(am), p, q, s)
        assert rc == L.DFU_E_INVALID and "dfu_maxpool_fwd_x3: bad P/Q" in last_error()
        rc = lib.dfu_maxpool_bwd(P_(yb), P_(am), B, H, W, C, p, q, P_(dx), s)
        assert rc == L.DFU_E_INVALID and "dfu_maxpool_bwd: bad P/Q" in last_error()
    torch.cuda.synchronize()
    assert (lo == SENT).all() and (yb == SENT).all() and (am == 9).all() and (dx == SENT).all()


# ------------------------------------------------------------------------------ 7. avgpool, GELU
@pytest.mark.parametrize("B,HW,C", [(1, 1, 8), (2, 50, 24), (3, 49, 2048)])
def test_avgpool_fwd_x3_shapes(B, HW, C):
    """test_maxpool_and_avgpool_x3's bar against the fp64 mean of hi + lo."""
    g = torch.Generator().manual_seed(700 + C)
    hi, lo = _pair(torch.randn(B * HW, C, generator=g).to(DEV))
    a = ops.avgpool_fwd_x3(hi, lo, B, HW, C)
    ref = (hi.double() + lo.double()).view(B, HW, C).mean(1)
    assert a.shape == (B, C)
    assert torch.allclose(a.double(), ref, rtol=1e-5, atol=1e-6)


# 0, -0.0, where erfcf / expf underflow (|x| >= 10), the central points; a row of 8 takes the
# first 8 (the zeros and the far tails)
GELU_GRID = [0.0, -0.0, -1e4, 1e4, -40.0, 40.0, -13.5, -10.0, 13.5, 10.0, -6.0, 6.0, -3.0, 3.0,
             -1.0, 1.0, -0.5, 0.5, -2.0 ** -20, 2.0 ** -20]


@pytest.mark.parametrize("rows,N", [(1, 8), (37, 24), (5, 3072)])
def test_gelu_x3_grid_and_tails(rows, N):
    """Every row: the fixed grid, filled up with randn * 3.  Reference: fp64 x / 2 erfc(-x /
    sqrt 2) and its derivative.  The triple keeps 2**-17 of the fp32 value, the rest of the
    2**-16 |ref| + 1e-30 bar is the fp32 evaluation; gelu' keeps test_layernorm_and_gelu_x3's
    bf16 bound; h_bf16 is the hi segment; nothing is NaN or Inf.  Measured on an MI355X: at most
    0.61 x 2**-16 for |x| <= 6 and 0.58 x 2**-16 beyond (x = -6.8), so the device erfcf needs no
    bound of its own in the tails."""
    g = torch.Generator().manual_seed(710 + N)
    x = torch.randn(rows, N, generator=g) * 3
    k = min(N, len(GELU_GRID))
    x[:, :k] = torch.tensor(GELU_GRID[:k])
    h3, hb, hp = ops.gelu_x3(x.to(DEV))
    xd = x.double()
    cdf = 0.5 * torch.special.erfc(-xd / math.sqrt(2))
    ref = xd * cdf
    dref = cdf + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    for t in (h3, hb, hp):
        assert torch.isfinite(t.float()).all()
    v, hi0, hi2 = _trip(h3, N)
    assert torch.equal(hb, h3[:, :N]) and torch.equal(hi0, hi2)
    err = (v.double().cpu() - ref).abs()
    rel = err / ref.abs().clamp_min(1e-300)
    big = ref.abs() > 1e-25
    tail = xd.abs() > 6
    for name, sel in (("|x| <= 6", ~tail & big), ("|x| > 6", tail & big)):
        if sel.any():
            i = rel[sel].argmax()
            print(f"\n[gelu x3 {rows}x{N}] {name}: max rel err {rel[sel][i].item():.3e} "
                  f"= {rel[sel][i].item() * 2 ** 16:.3f} x 2**-16 at x = {xd[sel][i].item():.6g}")
    assert (err <= 2.0 ** -16 * ref.abs() + 1e-30).all()
    assert ((hp.double().cpu() - dref).abs() <= 2.0 ** -8 * dref.abs() + 1e-6).all()
