"""One direct test per libdfu_hip export that the rest of the suite reaches only through
whole-model parity runs: each kernel against an fp64 reference of the same operation on the same
inputs (exact operations bitwise), at the small shapes where it can go wrong -- tails, strides
larger than the row, more than one block, NULL optional outputs.

Every tolerance below is derived in a comment from the roundings the kernel performs
(u = 2**-24, the relative error of one correctly rounded fp32 operation) or copied from a named
test of test_kernels_gpu.py; none is fitted to an observed error."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dfu_hip import _lib as L
from dfu_hip import ops
from test_kernels_gpu import close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def bits(t):
    """The raw bit pattern of a 16- or 32-bit floating tensor (so -0.0 != +0.0, inf == inf)."""
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def within(got, ref64, tol64, what):
    """|got - ref| <= tol elementwise, everything in fp64."""
    err = (got.double() - ref64).abs()
    bad = err > tol64
    assert not bad.any(), (f"{what}: max err {err.max().item():.3e}, worst err/tol "
                           f"{(err / tol64.clamp_min(1e-300)).max().item():.3f} "
                           f"(n_bad={int(bad.sum())})")


def P(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------ gemm_f32
def _f32_splits(M, N, K):
    """csrc/gemm_f32.hip splits_for, then the TK = 16 rounding of dfu_gemm_f32."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    s = max(1, min(512 // tiles, (K + 63) // 64))
    kps = (((K + s - 1) // s) + 15) // 16 * 16
    return s, (K + kps - 1) // kps


GEMM_F32_SHAPES = [
    # M, N, K, A and B stored [K][M] / [K][N]
    (65, 3, 2816, False),    # 2 tiles, 44 splits
    (5, 70, 17, False),      # K tail, no split
    (64, 64, 16, False),     # exactly one tile, one K step
    (130, 66, 1000, True),   # 6 tiles, 16 splits, both operands MN-major
]


@pytest.mark.parametrize("M,N,K,trans", GEMM_F32_SHAPES)
def test_gemm_f32(M, N, K, trans):
    """C = accumulate*C0 + A B^T (+ bias) (relu), through ops.gemm_f32 (split-K through the
    workspace) and through lib.dfu_gemm_f32 with workspace = NULL (unsplit), all eight
    bias / relu / accumulate combinations, ldc > N.

    Tolerance per element: (K + splits + 3) u (|A| |B|^T + |bias| + |C0|).  Derivation: within a
    split the products are accumulated by fmaf, one rounding per k, K roundings over all splits,
    each at most u times the magnitude of a partial sum, itself at most (|A| |B|^T)[m][n]; the
    reduce kernel adds `splits` slabs (one rounding each), then bias and C0 (one rounding each),
    all bounded by u (|A| |B|^T + |bias| + |C0|); relu is exact and 1-Lipschitz.  That is
    K + splits + 2 roundings to first order; one more u covers the second-order terms
    ((1 + u)^(K + 46) - 1 < (K + 47) u for K < 2**12)."""
    lib = L.load()
    planned, splits = _f32_splits(M, N, K)
    need = lib.dfu_gemm_f32_workspace_bytes(M, N, K)
    # the header's contract: split slabs of M x N floats each where it splits, 0 for short K
    assert need == (planned * M * N * 4 if planned > 1 else 0)
    assert lib.dfu_gemm_f32_workspace_bytes(M, N, 64) == 0
    assert lib.dfu_gemm_f32_workspace_bytes(M, N, 1) == 0
    A = rnd(M, K, dtype=F32, seed=100)
    B = rnd(N, K, dtype=F32, seed=101)
    bias = rnd(N, dtype=F32, seed=102)
    ldc = N + 5
    C0 = rnd(M, ldc, dtype=F32, seed=103)
    if trans:
        Am, sam, sak = A.t().contiguous(), 1, M
        Bm, sbn, sbk = B.t().contiguous(), 1, N
    else:
        Am, sam, sak = A, K, 1
        Bm, sbn, sbk = B, K, 1
    prod = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    for use_ws in (True, False):
        ns = splits if use_ws else 1
        for has_bias in (False, True):
            for relu in (False, True):
                for acc in (False, True):
                    what = f"gemm_f32 ws={use_ws} bias={has_bias} relu={relu} acc={acc}"
                    C = C0.clone()
                    b = bias if has_bias else None
                    if use_ws:
                        ops.gemm_f32(M, N, K, Am, sam, sak, Bm, sbn, sbk, C, ldc, bias=b,
                                     relu=relu, accumulate=acc)
                    else:
                        rc = lib.dfu_gemm_f32(M, N, K, P(Am), sam, sak, P(Bm), sbn, sbk, P(C), ldc,
                                              P(b), int(relu), int(acc), None, 0, ops.stream_ptr())
                        assert rc == 0, what
                    ref = prod.clone()
                    m = mag.clone()
                    if has_bias:
                        ref += bias.double()
                        m += bias.double().abs()
                    if acc:
                        ref += C0[:, :N].double()
                        m += C0[:, :N].double().abs()
                    if relu:
                        ref = ref.clamp_min(0)
                    within(C[:, :N], ref, (K + ns + 3) * U * m, what)
                    assert same_bits(C[:, N:], C0[:, N:]), what + ": columns past N touched"
    # split-K through slabs is bitwise reproducible
    outs = []
    for _ in range(2):
        C = C0.clone()
        ops.gemm_f32(M, N, K, Am, sam, sak, Bm, sbn, sbk, C, ldc, bias=bias, accumulate=True)
        outs.append(C)
    assert same_bits(outs[0], outs[1])


# ------------------------------------------------------------------------------ casts
def _special_f32():
    """7 x 13 fp32 values: ties that round to even (down and up), a value just above a tie, a
    fp32 subnormal (-> the smallest bf16 subnormal), bf16 subnormals, +-0, +-inf, the largest
    finite fp32 (-> bf16 inf), then random numbers."""
    g = torch.Generator().manual_seed(110)
    v = torch.randn(7 * 13, generator=g) * 3
    sp = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8),
          1e-40, -1e-40, 2.0 ** -133, 3 * 2.0 ** -134, 0.0, -0.0, float("inf"), -float("inf"),
          3.4028234663852886e38, -3.4028234663852886e38, 2.0 ** -126]
    v[:len(sp)] = torch.tensor(sp, dtype=F32)
    return v[torch.randperm(v.numel(), generator=g)].view(7, 13)


def test_cast_rows_bf16():
    rows, cols, ld_in, ld_out = 7, 13, 16, 24
    src = torch.full((rows, ld_in), 123.0, dtype=F32)
    src[:, :cols] = _special_f32()
    x = src.to(DEV)
    out = torch.full((rows, ld_out), 7.0, dtype=BF16, device=DEV)
    ops.cast_rows_bf16(x[:, :cols], ld_out=ld_out, out=out)
    ref = src[:, :cols].to(BF16)  # round to nearest even, in software on the host
    assert same_bits(out[:, :cols].cpu(), ref)
    assert torch.equal(bits(out[:, cols:]), torch.zeros_like(bits(out[:, cols:]))), "pad != +0"


def test_cast_rows_f32():
    rows, cols, ld_in, ld_out = 7, 13, 16, 24
    src = torch.full((rows, ld_in), 123.0, dtype=BF16)
    src[:, :cols] = _special_f32().to(BF16)
    x = src.to(DEV)
    out = torch.full((rows, ld_out), 7.0, dtype=F32, device=DEV)
    out0 = out.clone()
    ops.cast_rows_f32(x[:, :cols], out=out[:, :cols])
    assert same_bits(out[:, :cols].cpu(), src[:, :cols].float())
    assert same_bits(out[:, cols:], out0[:, cols:]), "pad columns touched"


# ------------------------------------------------------------------------------ relu
def _relu_input(dtype):
    g = torch.Generator().manual_seed(120)
    x = torch.randn(1000, generator=g)
    x[:6] = torch.tensor([-0.0, 0.0, float("inf"), -float("inf"), 2.0 ** -130, -2.0 ** -130])
    return x.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_relu_fwd(dtype):
    """Bitwise against torch.relu on the same tensor; the bf16 kernel tests the sign bit, so
    -0.0 (and every negative, -inf and negative subnormals included) must give +0."""
    x = _relu_input(dtype)
    y = ops.relu_fwd(x)
    assert bits(y)[0].item() == 0 and bits(y)[1].item() == 0, "relu(+-0) is not +0"
    assert same_bits(y, torch.relu(x))
    assert same_bits(y, torch.where(x > 0, x, torch.zeros_like(x)))


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_relu_bwd(dtype):
    y = _relu_input(dtype)  # negatives too: dx = dy where y > 0, else +0
    dy = rnd(1000, dtype=dtype, seed=121)
    dy[7] = -0.0
    dx = ops.relu_bwd(dy, y)
    assert same_bits(dx, torch.ops.aten.threshold_backward(dy, y, 0))
    assert same_bits(dx, torch.where(y > 0, dy, torch.zeros_like(dy)))


# ------------------------------------------------------------------------------ concat / split
@pytest.mark.parametrize("Na,Nb", [(2048, 768), (3, 5)])
def test_concat2_split2(Na, Nb):
    rows = 5
    lib = L.load()
    af, bf = rnd(rows, Na, dtype=F32, seed=130), rnd(rows, Nb, dtype=F32, seed=131)
    for a in (af, af.to(BF16)):
        for b in (bf, bf.to(BF16)):
            out = ops.concat2_bf16(a, b)
            assert same_bits(out, torch.cat([a.float(), b.float()], 1).to(BF16)), (a.dtype, b.dtype)
    assert same_bits(ops.concat2_f32(af, bf), torch.cat([af, bf], 1))
    for g in (rnd(rows, Na + Nb, dtype=F32, seed=132), rnd(rows, Na + Nb, dtype=BF16, seed=133)):
        ga, gb = ops.split2_f32(g, Na, Nb)
        assert same_bits(ga, g[:, :Na].float()) and same_bits(gb, g[:, Na:].float())
        # ga or gb NULL: only the other is written
        ga2 = torch.full((rows, Na), 9.0, device=DEV)
        gb2 = torch.full((rows, Nb), 9.0, device=DEV)
        s = ops.stream_ptr()
        assert lib.dfu_split2_f32(P(g), int(g.dtype == BF16), rows, Na, Nb, P(ga2), None, s) == 0
        assert same_bits(ga2, ga)
        assert lib.dfu_split2_f32(P(g), int(g.dtype == BF16), rows, Na, Nb, None, P(gb2), s) == 0
        assert same_bits(gb2, gb)


# ------------------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("stride,offset", [(197, 0), (2, 1)])
def test_gather_scatter_rows_f32(stride, offset):
    """The class-token pick out[i] = in[i * stride + offset] and its adjoint (add)."""
    lib = L.load()
    rows, D, ld_in, ld_out = 3, 20, 24, 28
    n_in = (rows - 1) * stride + offset + 1
    s = ops.stream_ptr()
    src = rnd(n_in, ld_in, dtype=F32, seed=140)
    out = torch.full((rows, ld_out), 5.0, device=DEV)
    assert lib.dfu_gather_rows_f32(P(src), ld_in, stride, offset, rows, D, P(out), ld_out, s) == 0
    ref = torch.full((rows, ld_out), 5.0, device=DEV)
    ref[:, :D] = src[offset::stride][:rows, :D]
    assert same_bits(out, ref)
    # scatter-add into a non-zero destination: picked rows get one fp32 add, the rest stay
    g = rnd(rows, ld_in, dtype=F32, seed=141)
    dst = rnd(n_in, ld_out, dtype=F32, seed=142)
    ref = dst.clone()
    ref[offset::stride][:rows, :D] += g[:, :D]
    assert lib.dfu_scatter_rows_f32(P(g), ld_in, stride, offset, rows, D, P(dst), ld_out, s) == 0
    assert same_bits(dst, ref)


# ------------------------------------------------------------------------------ ViT embedding
VIT_SHAPES = [(3, 5, 16), (9, 197, 768), (1, 2, 8)]  # B = 9 crosses the 8-image unroll


@pytest.mark.parametrize("B,T,D", VIT_SHAPES)
def test_vit_cls_rows(B, T, D):
    cls = rnd(D, dtype=F32, seed=150)
    pos = rnd(T, D, dtype=F32, seed=151)
    x = torch.full((B, T, D), -3.5, device=DEV)
    ops.vit_cls_rows(cls, pos, x, B, T, D)
    ref = torch.full((B, T, D), -3.5, device=DEV)
    ref[:, 0] = cls + pos[0]
    assert same_bits(x, ref)


@pytest.mark.parametrize("B,T,D", VIT_SHAPES)
def test_vit_embed_bwd(B, T, D):
    """dcls += sum_b gx[b,0]; dpos[t] += sum_b gx[b,t]; dbias += sum_{b,t>0} gx[b,t] (the class
    token row is not a patch: it must not be counted); gpatch = bf16(gx[:,1:]).  The kernel
    accumulates into non-zero buffers.  Each fp32 sum of n terms (the initial value included)
    is within n u sum|terms| of the exact sum, whatever the order."""
    gx = rnd(B, T, D, dtype=F32, seed=160)
    dcls0 = rnd(D, dtype=F32, seed=161)
    dpos0 = rnd(T, D, dtype=F32, seed=162)
    dbias0 = rnd(D, dtype=F32, seed=163)
    dcls, dpos, dbias = dcls0.clone(), dpos0.clone(), dbias0.clone()
    gpatch = ops.vit_embed_bwd(gx, B, T, D, dcls, dpos, dbias)
    g64, a64 = gx.double(), gx.double().abs()
    assert same_bits(gpatch, gx[:, 1:].reshape(B * (T - 1), D).to(BF16))
    within(dcls, dcls0.double() + g64[:, 0].sum(0),
           (B + 1) * U * (dcls0.double().abs() + a64[:, 0].sum(0)), "dcls")
    within(dpos, dpos0.double() + g64.sum(0),
           (B + 1) * U * (dpos0.double().abs() + a64.sum(0)), "dpos")
    n = B * (T - 1) + 1
    within(dbias, dbias0.double() + g64[:, 1:].sum((0, 1)),
           n * U * (dbias0.double().abs() + a64[:, 1:].sum((0, 1))), "dbias")
    # every optional output NULL: the patch gradient alone
    assert same_bits(ops.vit_embed_bwd(gx, B, T, D, None, None, None), gpatch)


# ------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("C", [2, 5])
def test_ce_weighted_fwd_bwd(B, C):
    """Loss and dlogits vs fp64 F.cross_entropy; row 0 holds |z| = 80 (exp(80) overflows fp32, so
    the kernel has to shift by the row maximum) and its label is the lowest logit (loss term
    160).  Tolerances: test_colsum_ce_adamw_dropout's 1e-5 (loss) and 1e-6 (gradient), which
    are for |z| of order 1, times max |z| (log-sum-exp rounds at the magnitude of z)."""
    g = torch.Generator().manual_seed(170 + B + C)
    z = torch.randn(B, C, generator=g) * 2
    z[0] = torch.linspace(-80.0, 80.0, C)
    y = torch.randint(0, C, (B,), generator=g)
    y[0] = 0
    w = torch.tensor([0.5, 2.0, 1.0, 3.0, 0.25])[:C]
    z, y, w = z.to(DEV), y.to(DEV), w.to(DEV)
    loss = torch.empty(1, device=DEV)
    dl = torch.full((B, C), 9.0, device=DEV)
    ops.ce_weighted_fwd(z, y, w, loss, dl)
    zr = z.double().requires_grad_(True)
    ref = F.cross_entropy(zr, y, weight=w.double())
    ref.backward()
    zs = max(1.0, z.abs().max().item())
    close(loss.double(), ref.detach().view(1), atol=1e-5 * zs, what="ce loss")
    within(dl, zr.grad, torch.full_like(zr.grad, 1e-6 * zs), "ce dlogits")
    half = torch.tensor([0.5], device=DEV)
    assert same_bits(ops.ce_weighted_bwd(dl, half), dl * 0.5)


# ------------------------------------------------------------------------------ optimizer, fill
def test_adamw_tensor_table():
    """dfu_adamw (the tensor-table form; the step uses dfu_adamw_flat): three steps over tensors
    of 1, 10007 and 65536 + 5 elements (the last spans two 65536-element chunks) against
    torch.optim.AdamW in fp64, with test_colsum_ce_adamw_dropout's AdamW tolerance."""
    lib = L.load()
    numels = [1, 10007, 65536 + 5]
    ps = [rnd(n, dtype=F32, seed=270 + i) for i, n in enumerate(numels)]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    gs = [torch.empty_like(p) for p in ps]
    refs = [p.double().clone().requires_grad_(True) for p in ps]
    opt = torch.optim.AdamW(refs, lr=1e-3, weight_decay=1e-2)

    def table(ts):
        return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)
    pt, gt, mt, vt = table(ps), table(gs), table(ms), table(vs)
    nt = torch.tensor(numels, dtype=torch.int64, device=DEV)
    chunks = [(t << 32) | c for t, n in enumerate(numels) for c in range((n + 65535) // 65536)]
    assert len(chunks) == 4
    ct = torch.tensor(chunks, dtype=torch.int64, device=DEV)
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    for it in range(3):
        for i, (g, r) in enumerate(zip(gs, refs)):
            g.copy_(rnd(g.numel(), dtype=F32, seed=280 + 10 * it + i))
            r.grad = g.double()
        opt.step()
        ops.step_increment(step)
        rc = lib.dfu_adamw(P(pt), P(gt), P(mt), P(vt), P(nt), len(numels), P(ct), len(chunks),
                           1e-3, 0.9, 0.999, 1e-8, 1e-2, P(step), ops.stream_ptr())
        assert rc == 0
    assert step.item() == 3
    for p, r in zip(ps, refs):
        close(p.double(), r.detach(), atol=1e-6, rtol=1e-5, what=f"adamw table n={p.numel()}")


def test_zero_fills_exactly_the_bytes_given():
    buf = torch.full((4099,), 0x5A, dtype=torch.uint8, device=DEV)
    ops.zero_(buf[3:4098])  # 4095 bytes from an odd address
    assert (buf[3:4098] == 0).all() and (buf[:3] == 0x5A).all() and buf[4098].item() == 0x5A
    x = torch.full((1000,), 3.0, device=DEV)
    assert ops.zero_(x[1:999]) is not None and x.sum().item() == 6.0


# ------------------------------------------------------------------------------ eval metrics
def _first_argmax(x):
    return np.argmax(x.cpu().numpy(), axis=1)  # numpy: the first maximum


@pytest.mark.parametrize("rows", [1, 300])  # 300: more rows than one 256-thread block
@pytest.mark.parametrize("C", [2, 7])
def test_argmax_rows(rows, C):
    g = torch.Generator().manual_seed(180)
    x = torch.randint(0, 3, (rows, C), generator=g).float()  # three values: ties in most rows
    x[0] = 1.0                                                # all equal: index 0
    x = x.to(DEV)
    got = ops.argmax_rows(x)
    assert got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), _first_argmax(x))
    assert torch.equal(got.cpu(), torch.max(x.cpu(), 1).indices)
    xr = rnd(rows, C, dtype=F32, seed=181)
    assert np.array_equal(ops.argmax_rows(xr).cpu().numpy(), _first_argmax(xr))


@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("C", [2, 7])
def test_softmax_rows(rows, C):
    """vs fp64 torch.softmax, relative tolerance (range + C + 4) 2**-23 with range = the
    largest max - min of a row (<= 16 here).  Derivation, in u = 2**-24: the shifted argument
    d = x - max is one rounding, |d| u <= range u absolute, which exp turns into range u
    relative; expf is good to 1 ulp = 2 u; so every exponential carries (range + 2) u.  The
    denominator adds C of them with C - 1 roundings: (range + 2 + C - 1) u.  The reciprocal
    and the final product are one rounding each.  Sum: (2 range + C + 5) u =
    (range + (C + 5) / 2) 2**-23 <= (range + C + 4) 2**-23."""
    g = torch.Generator().manual_seed(190)
    x = torch.rand(rows, C, generator=g) * 16
    x[0] = 3.25  # equal values: exp(0) = 1 and the sum C are exact, so every entry is fp32(1 / C)
    x = x.to(DEV)
    out = ops.softmax_rows(x)
    ref = torch.softmax(x.double(), 1)
    rng = (x.max(1).values - x.min(1).values).max().item()
    within(out, ref, (rng + C + 4) * 2.0 ** -23 * ref, "softmax_rows")
    assert np.array_equal(out[0].cpu().numpy(), np.full(C, np.float32(1) / np.float32(C)))


@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("C", [2, 7])
def test_metrics_accumulate(rows, C):
    """Three calls into the same buffers (the second without a loss): confusion[label][argmax]
    counts with labels outside [0, C) skipped, batches == 3, loss_sum the exact fp64 sum."""
    conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    loss_sum = torch.zeros(1, dtype=F64, device=DEV)
    batches = torch.zeros(1, dtype=torch.int64, device=DEV)
    want = np.zeros((C, C), dtype=np.int64)
    losses = [torch.tensor(0.7, device=DEV), None, torch.tensor(1.3, device=DEV)]
    for call, loss in enumerate(losses):
        g = torch.Generator().manual_seed(200 + call)
        z = torch.randint(0, 3, (rows, C), generator=g).float().to(DEV)  # ties: first max wins
        y = torch.randint(-1, C + 1, (rows,), generator=g).to(DEV)       # -1 and C: skipped
        ops.metrics_accumulate(z, y, loss, conf, loss_sum, batches)
        for lab, am in zip(y.cpu().tolist(), _first_argmax(z).tolist()):
            if 0 <= lab < C:
                want[lab, am] += 1
    assert np.array_equal(conf.cpu().numpy(), want)
    assert batches.item() == 3
    assert loss_sum.item() == float(np.float32(0.7)) + float(np.float32(1.3))


# ------------------------------------------------------------------------------ BatchNorm pieces
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("C", [8, 1536])
def test_bn_eval_coeffs(C, affine):
    """scale = gamma / sqrt(rv + eps), shift = beta - rm * scale (gamma / beta NULL: 1 / 0).
    Running variances of 1e-5 .. 1e-3 against eps = 1e-5: the epsilon is 1 % to 50 % of the sum.
    scale: rv + eps (one rounding, halved by the square root), sqrtf, the division and the
    product with gamma, each correctly rounded: 3.5 u <= the 4 u relative bound.
    shift: rm * gamma * inv carries two more roundings on top of inv's 2.5 u (4.5 u of
    |rm scale|), the subtraction one u of |shift| <= |beta| + |rm scale|.  The difference can
    cancel, so the bound is relative to the operands: u (5.5 |rm scale| + |beta|)."""
    eps = 1e-5
    eps32 = float(np.float32(eps))  # the kernel receives eps as a float
    g = torch.Generator().manual_seed(210)
    rv = (10 ** (-5 + 2 * torch.rand(C, generator=g))).to(DEV)
    rm = (torch.randn(C, generator=g) * 0.01).to(DEV)
    gamma = (torch.randn(C, generator=g) * 0.5 + 1).to(DEV) if affine else None
    beta = torch.randn(C, generator=g).to(DEV) if affine else None
    scale = torch.empty(C, device=DEV)
    shift = torch.empty(C, device=DEV)
    ops.bn_eval_coeffs(gamma, beta, rm, rv, eps, scale, shift)
    g64 = gamma.double() if affine else torch.ones(C, dtype=F64, device=DEV)
    b64 = beta.double() if affine else torch.zeros(C, dtype=F64, device=DEV)
    s_ref = g64 / torch.sqrt(rv.double() + eps32)
    within(scale, s_ref, 4 * U * s_ref.abs(), "bn_eval_coeffs scale")
    within(shift, b64 - rm.double() * s_ref,
           U * (5.5 * (rm.double() * s_ref).abs() + b64.abs()), "bn_eval_coeffs shift")


@pytest.mark.parametrize("M,C", [(300, 64), (128, 8), (1, 1536), (257, 72)])
def test_bn_tile_stats(M, C):
    """(sum, M2 about the tile mean) per 128-row tile from stored bf16 rows, against fp64 on the
    same bf16 values with test_gemm_stats' tolerances; (257, 72): a one-row last tile, a ragged
    last 64-channel group.  The records then go through bn_finalize: mean and biased variance
    of the whole batch (test_batchnorm_train_fwd_bwd's running-statistics tolerances)."""
    x = rnd(M, C, seed=220, scale=2.0) + 0.5
    stats = ops.bn_tile_stats(x, M, C)
    tiles = (M + 127) // 128
    assert stats.shape == (tiles, 2, C)
    x64 = x.double()
    for t in range(tiles):
        blk = x64[t * 128:(t + 1) * 128]
        close(stats[t, 0].double(), blk.sum(0), atol=1e-2, rtol=1e-4, what=f"tile {t} sum")
        close(stats[t, 1].double(), ((blk - blk.mean(0)) ** 2).sum(0), atol=1e-2, rtol=1e-3,
              what=f"tile {t} M2")
    mean, invstd, scale, shift = (torch.empty(C, device=DEV) for _ in range(4))
    ops.bn_finalize(stats, M, C, None, None, 1e-5, 0.1, None, None, None, mean, invstd, scale,
                    shift)
    close(mean, x.float().mean(0), atol=1e-4, what="mean")
    var = 1.0 / invstd.double() ** 2 - float(np.float32(1e-5))
    close(var, x.float().var(0, unbiased=False), atol=1e-3, rtol=1e-3, what="var")


# ------------------------------------------------------------------------------ column sums
COLSUM_CASES = [
    # dtype, rows, N, ld
    (F32, 1, 2, 2),          # the fusion head's N = 2: scalar tail only, one row
    (F32, 65, 515, 520),     # two column blocks, N % 8 != 0, ld > N, one-row last block
    (F32, 130, 768, 768),    # three row blocks
    (BF16, 65, 520, 528),    # vector path past column 512, ld > N
    (BF16, 64, 8, 8),        # exactly one block, one vector
]


@pytest.mark.parametrize("dtype,rows,N,ld", COLSUM_CASES)
def test_colsum(dtype, rows, N, ld):
    """colsum_add into a non-zero out, and the partials-only form: [ceil(rows / 64)][N], each
    row the sum of its 64-row block.  rows terms and the previous value of out are rows roundings,
    each at most u times a partial sum: rows u (sum|x| + |out|) per column; a block's partial
    has 64 terms at most."""
    x = rnd(rows, ld, dtype=dtype, seed=230)[:, :N]
    assert x.stride(0) == ld
    out0 = rnd(N, dtype=F32, seed=231)
    out = out0.clone()
    ops.colsum_add(x, out)
    x64 = x.double()
    within(out, out0.double() + x64.sum(0),
           rows * U * (out0.double().abs() + x64.abs().sum(0)), "colsum_add")
    part = ops.colsum_partial(x)
    blocks = (rows + 63) // 64
    assert part.shape == (blocks, N)
    for b in range(blocks):
        blk = x64[b * 64:(b + 1) * 64]
        within(part[b], blk.sum(0), 64 * U * blk.abs().sum(0), f"colsum_partial block {b}")


def test_reduce_partials_batch():
    """Nine reductions through ops.PartialReductions (the ninth add comes after the automatic
    flush at eight): differing widths, padded strides, an offset into a [blocks][2][D] slab,
    1 / 32 / 33 / 394 blocks (32 = the kernel's row lanes).  Bitwise equal to
    reduce_partials_add on the same numbers (the header: "same sums as dfu_reduce_partials")
    and within blocks u (sum|p| + |out|) of the exact sum (blocks roundings, the add into the
    pre-filled out included)."""
    slab = rnd(394, 2, 768, dtype=F32, seed=240)
    small = rnd(394, 2, 4, dtype=F32, seed=241)
    cases = [  # (buffer [blocks][stride], D, stride, offset)
        (rnd(1, 4, dtype=F32, seed=242), 4, 4, 0),
        (rnd(32, 8, dtype=F32, seed=243), 8, 8, 0),
        (rnd(33, 9, dtype=F32, seed=244), 9, 9, 0),
        (slab, 768, 1536, 0),
        (slab, 768, 1536, 768),
        (rnd(33, 2304, dtype=F32, seed=245), 2304, 2304, 0),
        (rnd(32, 12, dtype=F32, seed=246), 9, 12, 0),
        (small, 4, 8, 4),
        (rnd(1, 768, dtype=F32, seed=247), 768, 768, 0),
    ]
    assert len(cases) == L.REDUCE_BATCH + 1
    red = ops.PartialReductions()
    outs, refs = [], []
    for i, (buf, D, stride, offset) in enumerate(cases):
        blocks = buf.shape[0]
        flat = buf.reshape(blocks, -1)
        assert flat.shape[1] == stride
        p = flat[:, offset:offset + D]
        o0 = rnd(D, dtype=F32, seed=250 + i)
        o, r = o0.clone(), o0.clone()
        red.add(buf, o, D, stride=stride, offset=offset, blocks=blocks)
        ops.reduce_partials_add(p.contiguous(), r)
        outs.append(o)
        refs.append((r, o0.double() + p.double().sum(0),
                     blocks * U * (o0.double().abs() + p.double().abs().sum(0))))
        if i == L.REDUCE_BATCH - 1:
            assert not red.entries, "no automatic flush at DFU_REDUCE_BATCH entries"
    assert len(red.entries) == 1
    red.flush()
    for i, (o, (r, exact, tol)) in enumerate(zip(outs, refs)):
        assert same_bits(o, r), f"entry {i}: differs from dfu_reduce_partials"
        within(o, exact, tol, f"entry {i}")


# ------------------------------------------------------------------------------ bf16x3 patchify
def test_patchify_f32_x3():
    """The pattern-0 triple [hi | lo | hi] of the ViT patch rows: hi is patchify_f32 bitwise,
    hi + lo the fp32 unfold (test_pooling_and_layout's "im2col x3 hi + lo" bound), on the
    vector path (contiguous), the strided path (channels-last) and the scalar path of an
    unaligned view (csrc/elem.hip patchify_vec)."""
    ps, K = 16, 3 * 16 * 16
    xc = rnd(2, 3, 32, 48, dtype=F32, seed=260)
    base = torch.empty(xc.numel() + 1, device=DEV)
    base[1:] = xc.reshape(-1)
    unaligned = base[1:].view(2, 3, 32, 48)
    assert unaligned.data_ptr() % 16 == 4
    for x in (xc, xc.contiguous(memory_format=torch.channels_last), unaligned):
        t3 = ops.patchify_f32_x3(x, ps)
        assert t3.shape == (2 * 2 * 3, 3 * K)
        hi, lo, hi2 = t3[:, :K], t3[:, K:2 * K], t3[:, 2 * K:]
        assert same_bits(hi, ops.patchify_f32(x, ps)) and same_bits(hi2, hi)
        ref = F.unfold(x, ps, stride=ps).transpose(1, 2).reshape(-1, K)
        assert same_bits(hi, ref.to(BF16))
        close(hi.float() + lo.float(), ref, atol=1e-6, rtol=1e-5, what="patchify x3 hi + lo")
