"""The code paths of already-tested kernels that no other test reaches: every padded-length
instantiation of the attention kernels (and lengths just past a 32-key boundary, where 31 of 32
keys are padding), LayerNorm at other widths / strides / gradient types, and the general
(non-FIXED) BatchNorm apply kernels.  References and tolerances are those of the named tests of
test_kernels_gpu.py, test_fp16_gpu.py and test_precision_gpu.py unless derived here."""
import pytest
import torch
import torch.nn.functional as F

from dfu_hip import _lib as L
from dfu_hip import ops
from test_kernels_gpu import close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def P(t):
    return None if t is None else t.data_ptr()


def last_error():
    return (L.load().dfu_last_error_string() or b"").decode()


# ------------------------------------------------------------------------------ attention
ATT_B, ATT_H, ATT_DH = 1, 2, 64
ATT_D = ATT_H * ATT_DH
ATT_SCALE = ATT_DH ** -0.5
# npad = 32 .. 256 in steps of 32 (KT = 2 .. 16): 1 | 32, 33 | 65, 96 | 97 | 129 | 161 | 193,
# 224 | 225, 255; 33, 65, 97, ... sit one key past a 32-boundary
ATT_N = [1, 32, 33, 65, 96, 97, 129, 161, 193, 224, 225, 255]


def _heads(t, N):
    """[B*N][3*H*dh] -> q, k, v as [B][H][N][dh]"""
    return t.view(ATT_B, N, 3, ATT_H, ATT_DH).permute(2, 0, 3, 1, 4).unbind(0)


def _boost_key(qkv, N, boost=True):
    """N = 33: the one real key past the 32-boundary, scaled by 8, dominates the softmax of
    the queries it agrees with; a padded key of its 32-block that leaked in would show."""
    if N == 33 and boost:
        qkv.view(ATT_B, N, 3, ATT_H, ATT_DH)[:, 32, 1] *= 8
    return qkv


def _sdpa64(qkv, N):
    """fp64 softmax attention of the given (already rounded) qkv: o [B*N][D], lse [B*H][N], and
    the autograd leaves."""
    q, k, v = (t.double().requires_grad_(True) for t in _heads(qkv, N))
    s = (q @ k.transpose(-1, -2)) * ATT_SCALE
    o = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(ATT_B * N, ATT_D)
    return o, torch.logsumexp(s, -1).reshape(ATT_B * ATT_H, N), (q, k, v)


@pytest.mark.parametrize("N,boost", [(n, False) for n in ATT_N] + [(33, True)])
def test_attention_bf16_every_length(N, boost):
    """attention_fwd and attention_bwd, test_attention's tolerances (absolute: written for
    outputs of order 1).  N = 33 runs twice: as every other length, and with key 32 scaled by 8.
    dq and dv grow with that key: with test_attention's unit-scale dout the exact fp64 dq
    reaches 10.2 and merely storing it in bf16 is off by 3.1e-2, above the 3e-2 bound (dv: 9.7,
    1.6e-2), so no kernel with a bf16 dqkv can pass; dout is therefore scaled by 1/8 in that
    case, which brings every gradient back to the magnitude the bounds are for (max |dq| 1.27,
    bf16 storage error 3.9e-3)."""
    qkv = _boost_key(rnd(ATT_B * N, 3 * ATT_D, seed=30), N, boost)
    o, lse = ops.attention_fwd(qkv, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
    assert lse.shape[1] == ops.attention_npad(N) == (N + 31) // 32 * 32
    ref_o, ref_lse, (q, k, v) = _sdpa64(qkv, N)
    close(o, ref_o, atol=2e-2, what="attn fwd")
    close(lse[:, :N], ref_lse, atol=1e-3, what="lse")
    do = rnd(ATT_B * N, ATT_D, seed=31, scale=0.125 if boost else 1.0)
    ref_o.backward(do.double())
    dqkv = ops.attention_bwd(qkv, o, do, lse, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
    dq, dk, dv = _heads(dqkv, N)
    close(dq, q.grad, atol=3e-2, what="dq")
    close(dk, k.grad, atol=3e-2, what="dk")
    close(dv, v.grad, atol=3e-2, what="dv")


@pytest.mark.parametrize("N", ATT_N)
def test_attention_f16_every_length(N):
    """attention_fwd_f16 (test_attention_fwd_f16_matches_sdpa's inputs and bounds) and the
    backward reading the fp16 qkv (test_attention_bwd_reads_fp16_qkv: bitwise the bf16 backward
    on bf16(qkv16))."""
    torch.manual_seed(4)
    qkv = _boost_key((torch.randn(ATT_B * N, 3 * ATT_D, device=DEV) * 2).to(F16), N)
    o16, ob, lse = ops.attention_fwd_f16(qkv, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
    ref, lref, _ = _sdpa64(qkv, N)
    ref = ref.detach()
    err = (o16.double() - ref).abs().max().item()
    print(f"\n[attn f16 N={N}] max abs err {err:.2e} (max |o| {ref.abs().max().item():.2f})")
    assert err < 2.0 ** -9 * ref.abs().max().item()
    assert ((ob.double() - o16.double()).abs() <= o16.double().abs() * 2.0 ** -7 + 1e-3).all()
    assert torch.allclose(lse[:, :N].double(), lref.detach(), rtol=2.0 ** -14, atol=1e-5)
    qb = qkv.to(BF16)
    ob2, lse2 = ops.attention_fwd(qb, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
    do = (torch.randn(ATT_B * N, ATT_D, device=DEV) * 0.1).to(BF16)
    d16 = ops.attention_bwd(qkv, ob2, do, lse2, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
    db = ops.attention_bwd(qb, ob2, do, lse2, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
    assert d16.dtype == BF16 and torch.equal(d16, db)


@pytest.mark.parametrize("N", [n for n in ATT_N if n <= 224])
def test_attention_f32_every_length(N):
    """attention_fwd_f32, test_attention_fwd_f32_matches_sdpa's inputs and bounds."""
    torch.manual_seed(7)
    qkv = _boost_key(torch.randn(ATT_B * N, 3 * ATT_D, device=DEV) * 2, N)
    qb = torch.empty(ATT_B * N, 3 * ATT_D, dtype=BF16, device=DEV)
    o3, ob, lse = ops.attention_fwd_f32(qkv, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE, qkv_bf16=qb)
    ref, lref, _ = _sdpa64(qkv, N)
    ref = ref.detach()
    D = ATT_D
    o = o3[:, :D].float() + o3[:, D:2 * D].float()
    err = (o.double() - ref).abs().max().item()
    print(f"\n[attn x3 N={N}] max abs err {err:.2e} (max |o| {ref.abs().max().item():.2f})")
    assert err < 2.0 ** -14 * ref.abs().max().item()
    assert torch.equal(ob, o3[:, :D]) and torch.equal(o3[:, 2 * D:], o3[:, :D])
    assert torch.equal(qb, qkv.to(BF16))
    assert torch.allclose(lse[:, :N].double(), lref.detach(), rtol=2.0 ** -14, atol=1e-5)


def test_attention_single_token_identities():
    """N = 1: the softmax is 1, so o = v, lse = scale q.k, dv = do and dq = dk = 0.  p = 1 is
    exact, so o and dv are copies up to one bf16 rounding (2**-8 relative).  ds = p (dp - delta)
    with dp = do.v on the MFMA and delta = do.o in fp32: two orders of the same 64 exact
    products, each within 64 u sum|do v| of the exact sum; dq = ds scale k, dk = ds scale q."""
    N = 1
    qkv = rnd(ATT_B * N, 3 * ATT_D, seed=32)
    do = rnd(ATT_B * N, ATT_D, seed=33)
    o, lse = ops.attention_fwd(qkv, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
    q, k, v = (t.double() for t in _heads(qkv, N))
    vrow = v.permute(0, 2, 1, 3).reshape(ATT_B * N, ATT_D)
    assert ((o.double() - vrow).abs() <= 2.0 ** -8 * vrow.abs()).all()
    close(lse[:, :1].double(), ((q * k).sum(-1) * ATT_SCALE).reshape(ATT_B * ATT_H, 1), atol=1e-3,
          what="lse")
    for src in (qkv, qkv.to(F16)):  # the fp16-qkv backward rounds to bf16: the same numbers
        dqkv = ops.attention_bwd(src, o, do, lse, ATT_B, N, ATT_H, ATT_DH, ATT_SCALE)
        dq, dk, dv = (t.double() for t in _heads(dqkv, N))
        dov = do.double().view(ATT_B, N, ATT_H, ATT_DH).permute(0, 2, 1, 3)
        assert ((dv - dov).abs() <= 2.0 ** -8 * dov.abs()).all()
        ds_tol = 128 * U * (dov.abs() * v.abs()).sum(-1, keepdim=True) * ATT_SCALE
        assert (dq.abs() <= ds_tol * k.abs().max()).all(), dq.abs().max().item()
        assert (dk.abs() <= ds_tol * q.abs().max()).all(), dk.abs().max().item()


def test_attention_length_limits_are_refused():
    """N = 257 (any forward, the backward) and N = 225 (the fp32 forward) return DFU_E_INVALID
    from the host-side check; no kernel is launched."""
    lib = L.load()
    N, npad = 257, 288
    s = ops.stream_ptr()
    qkv = torch.zeros(ATT_B * N, 3 * ATT_D, dtype=BF16, device=DEV)
    qf = torch.zeros(ATT_B * N, 3 * ATT_D, dtype=F32, device=DEV)
    o = torch.full((ATT_B * N, ATT_D), 3.0, dtype=BF16, device=DEV)
    o3 = torch.zeros(ATT_B * N, 3 * ATT_D, dtype=BF16, device=DEV)
    lse = torch.zeros(ATT_B * ATT_H, npad, device=DEV)
    B, H, dh = ATT_B, ATT_H, ATT_DH
    assert lib.dfu_attention_fwd(P(qkv), B, N, H, dh, ATT_SCALE, P(o), P(lse), s) == L.DFU_E_INVALID
    assert "N=257" in last_error()
    assert lib.dfu_attention_fwd_f16(P(qkv), B, N, H, dh, ATT_SCALE, P(o3), P(o), P(lse),
                                     s) == L.DFU_E_INVALID
    assert lib.dfu_attention_bwd(P(qkv), P(o), P(o), P(lse), B, N, H, dh, ATT_SCALE, P(lse),
                                 P(o3), s) == L.DFU_E_INVALID
    for n in (225, 257):
        assert lib.dfu_attention_fwd_f32(P(qf), B, n, H, dh, ATT_SCALE, npad, None, P(o3), P(o),
                                         P(lse), s) == L.DFU_E_INVALID
    assert "<= 224" in last_error()
    with pytest.raises(L.DfuError):
        ops.attention_fwd(qkv, B, N, H, dh, ATT_SCALE)
    torch.cuda.synchronize()
    assert (o == 3.0).all()


# ------------------------------------------------------------------------------ LayerNorm
LN_CASES = [(1, 4, 4), (33, 260, 264), (5, 1024, 1024), (40, 768, 772)]  # rows, D, ld


def _ln_inputs(rows, D, ld):
    g = torch.Generator().manual_seed(300 + D)
    xb = (torch.randn(rows, ld, generator=g) * 3 + 1).to(DEV)
    gamma = torch.randn(D, generator=g).to(DEV)
    beta = torch.randn(D, generator=g).to(DEV)
    return xb, gamma, beta


@pytest.mark.parametrize("out_bf16", [True, False])
@pytest.mark.parametrize("rows,D,ld", LN_CASES)
def test_layernorm_fwd_shapes(rows, D, ld, out_bf16):
    """D % 4 == 0 up to 1024, row strides larger than D, bf16 and fp32 output; the pad columns
    of a strided output stay untouched.  test_layernorm_fwd_bwd's tolerance."""
    xb, gamma, beta = _ln_inputs(rows, D, ld)
    x = xb[:, :D]
    out = torch.full((rows, ld), 7.0, dtype=BF16 if out_bf16 else F32, device=DEV)
    mean = torch.empty(rows, device=DEV)
    rstd = torch.empty(rows, device=DEV)
    ops.layernorm_fwd(x, ld, rows, D, gamma, beta, 1e-6, out, ld, out_bf16, mean, rstd)
    ref = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-6)
    close(out[:, :D], ref, atol=3e-2, rtol=1e-2, what="ln fwd")
    assert (out[:, D:] == 7.0).all(), "pad columns written"


@pytest.mark.parametrize("dy_bf16,gsum", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("rows,D,ld", LN_CASES)
def test_layernorm_bwd_shapes(rows, D, ld, dy_bf16, gsum):
    """The backward at the same shapes: bf16 dy, fp32 dy with lddy > D, gsum_partial == NULL;
    gx and its bf16 copy strided (pad columns untouched).  test_layernorm_fwd_bwd's
    tolerances."""
    xb, gamma, beta = _ln_inputs(rows, D, ld)
    x = xb[:, :D]
    mean = torch.empty(rows, device=DEV)
    rstd = torch.empty(rows, device=DEV)
    out = torch.empty(rows, D, device=DEV)
    ops.layernorm_fwd(x, ld, rows, D, gamma, beta, 1e-6, out, D, False, mean, rstd)
    lddy = ld + 4
    dyb = rnd(rows, lddy, dtype=BF16 if dy_bf16 else F32, seed=310)
    dy = dyb[:, :D]
    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = beta.double().requires_grad_(True)
    F.layer_norm(xr, (D,), gr, br, 1e-6).backward(dy.double())
    gxb = rnd(rows, ld, dtype=F32, seed=311)
    gx0 = gxb.clone()
    gx16 = torch.full((rows, ld), 7.0, dtype=BF16, device=DEV)
    dgam = torch.zeros(D, device=DEV)
    dbet = torch.zeros(D, device=DEV)
    gsp = ops.layernorm_bwd(dy, lddy, dy_bf16, x, ld, mean, rstd, gamma, rows, D, gxb, ld, gx16,
                            dgam, dbet, gsum=gsum)
    gx = gxb[:, :D]
    close(gx, gx0[:, :D].double() + xr.grad, atol=1e-3, rtol=1e-3, what="ln dx")
    assert torch.equal(gxb[:, D:], gx0[:, D:]), "gx pad columns written"
    close(gx16[:, :D], gx, atol=2e-2, rtol=1e-2, what="ln dx bf16")
    assert (gx16[:, D:] == 7.0).all(), "bf16 gx pad columns written"
    close(dgam, gr.grad, atol=1e-2, rtol=1e-3, what="ln dgamma")
    close(dbet, br.grad, atol=1e-2, rtol=1e-3, what="ln dbeta")
    if gsum:
        assert gsp.shape == ((rows + 31) // 32, D)
        tot = torch.zeros(D, device=DEV)
        ops.reduce_partials_add(gsp, tot)
        close(tot, gx.double().sum(0), atol=1e-3, rtol=1e-4, what="ln gx column sums")
    else:
        assert gsp is None


@pytest.mark.parametrize("D", [1028, 6])
def test_layernorm_refuses_unsupported_width(D):
    rows = 2
    ld = (D + 3) // 4 * 4
    x = torch.zeros(rows, ld, device=DEV)
    gamma = torch.ones(ld, device=DEV)
    out = torch.full((rows, ld), 7.0, device=DEV)
    mean = torch.zeros(rows, device=DEV)
    with pytest.raises(L.DfuError) as e:
        ops.layernorm_fwd(x, ld, rows, D, gamma, gamma, 1e-6, out, ld, False, mean, mean)
    assert e.value.code == L.DFU_E_INVALID
    with pytest.raises(L.DfuError) as e:
        ops.layernorm_bwd(x, ld, False, x, ld, mean, mean, gamma, rows, D, out, ld, None, None,
                          None)
    assert e.value.code == L.DFU_E_INVALID
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------ BatchNorm
def _bn_setup(M, C, seed=400):
    """bf16 rows, their statistics through bn_tile_stats + bn_finalize, and the fp64 leaves."""
    y = rnd(M, C, seed=seed, scale=2.0) + 0.5
    gamma = rnd(C, dtype=F32, seed=seed + 1) * 0.5 + 1
    beta = rnd(C, dtype=F32, seed=seed + 2)
    stats = ops.bn_tile_stats(y, M, C)
    mean, invstd, scale, shift = (torch.empty(C, device=DEV) for _ in range(4))
    ops.bn_finalize(stats, M, C, gamma, beta, 1e-5, 0.1, None, None, None, mean, invstd, scale,
                    shift)
    return y, gamma, beta, mean, invstd, scale, shift


def _bn_ref(y, gamma, beta, res, relu, dout, training=True, rm=None, rv=None):
    yf = y.double().requires_grad_(True)
    gf = gamma.double().requires_grad_(True)
    bf = beta.double().requires_grad_(True)
    rm = None if rm is None else rm.double()
    rv = None if rv is None else rv.double()
    ref = F.batch_norm(yf, rm, rv, gf, bf, training=training, momentum=0.1, eps=1e-5)
    if res is not None:
        ref = ref + res.double()
    if relu:
        ref = torch.relu(ref)
    if dout is not None:
        ref.backward(dout.double())
    return ref.detach(), yf.grad, gf.grad, bf.grad


def _mask_bits(mask, M, C):
    return ((mask.view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).view(M, C)


def test_batchnorm_general_form_fwd_bwd():
    """C = 1536: C / 8 = 192 is no power of two, so apply and backward-apply take the general
    (per-vector channel decode) kernels, as dfu_hip.nn.BatchNorm2d does for such widths.
    Forward with and without residual / ReLU and with the bitmask; backward with relu 0 / 1 /
    2 / 3 against F.batch_norm autograd in fp64 (test_batchnorm_train_fwd_bwd's tolerances);
    relu 2 and 3 bitwise equal to relu 1."""
    M, C = 300, 1536
    y, gamma, beta, mean, invstd, scale, shift = _bn_setup(M, C)
    res = rnd(M, C, seed=410)
    dout = rnd(M, C, seed=411)

    def bwd(o, mode, want_res):
        dy = torch.empty_like(y)
        dres = torch.empty_like(y) if want_res else None
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.bn_bwd(dout, y, o, mode, mean, invstd, gamma, M, C, dy, dres, dg, db, scale=scale,
                   shift=shift)
        return dy, dg, db, dres

    def check(got, ref, what):
        close(got[0], ref[1], atol=2e-2, rtol=2e-2, what=what + " bn dx")
        close(got[1], ref[2], atol=0.5, rtol=1e-2, what=what + " dgamma")
        close(got[2], ref[3], atol=0.5, rtol=1e-2, what=what + " dbeta")

    # plain BN
    out = torch.empty_like(y)
    ops.bn_apply(y, scale, shift, None, False, out, M, C)
    ref = _bn_ref(y, gamma, beta, None, False, dout)
    close(out, ref[0], atol=3e-2, rtol=1e-2, what="bn fwd")
    check(bwd(None, 0, False), ref, "relu=0")
    # BN + residual + ReLU
    ops.bn_apply(y, scale, shift, res, True, out, M, C)
    ref = _bn_ref(y, gamma, beta, res, True, dout)
    close(out, ref[0], atol=3e-2, rtol=1e-2, what="bn + res + relu fwd")
    got = bwd(out, 1, True)
    check(got, ref, "relu=1 residual")
    assert torch.equal(got[3], torch.where(out.float() > 0, dout, torch.zeros_like(dout)))
    # BN + ReLU with the bitmask
    mask = torch.empty(M * C // 8, dtype=torch.uint8, device=DEV)
    ops.bn_apply(y, scale, shift, None, True, out, M, C, mask=mask)
    ref = _bn_ref(y, gamma, beta, None, True, dout)
    close(out, ref[0], atol=3e-2, rtol=1e-2, what="bn + relu fwd")
    assert torch.equal(_mask_bits(mask, M, C).bool(), out.float() > 0), "bitmask != (out > 0)"
    plain = torch.empty_like(y)
    ops.bn_apply(y, scale, shift, None, True, plain, M, C)
    assert torch.equal(plain, out), "bn_apply_mask != bn_apply"
    r1 = bwd(out, 1, False)
    check(r1, ref, "relu=1")
    for mode, o in ((2, None), (3, mask)):
        for a, b in zip(r1[:3], bwd(o, mode, False)[:3]):
            assert torch.equal(a, b), f"relu={mode} differs from relu=1"


@pytest.mark.parametrize("C", [64, 1536])
def test_batchnorm_bwd_eval_mode(C):
    """dfu_bn_bwd with batch_stats = 0 (running statistics are constants): dy = gamma invstd g
    (one bf16 rounding: 2**-8 relative), dgamma / dbeta against an eval-mode F.batch_norm
    autograd with test_batchnorm_train_fwd_bwd's tolerances."""
    M = 300
    y = rnd(M, C, seed=420, scale=2.0) + 0.5
    gamma = rnd(C, dtype=F32, seed=421) * 0.5 + 1
    beta = rnd(C, dtype=F32, seed=422)
    rm = rnd(C, dtype=F32, seed=423) * 0.5 + 0.5
    rv = rnd(C, dtype=F32, seed=425).abs() * 2 + 1
    invstd = (rv.double() + 1e-5).rsqrt().float()
    dout = rnd(M, C, seed=424)
    dy = torch.empty_like(y)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ops.bn_bwd(dout, y, None, 0, rm, invstd, gamma, M, C, dy, None, dg, db, batch_stats=False)
    _, dy_ref, dg_ref, db_ref = _bn_ref(y, gamma, beta, None, False, dout, training=False, rm=rm,
                                       rv=rv)
    want = gamma.double() * invstd.double() * dout.double()
    assert ((dy.double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-30).all()
    close(dy, dy_ref, atol=2e-2, rtol=2e-2, what="eval bn dx")
    close(dg, dg_ref, atol=0.5, rtol=1e-2, what="eval dgamma")
    close(db, db_ref, atol=0.5, rtol=1e-2, what="eval dbeta")


@pytest.mark.parametrize("C", [24, 96])
def test_batchnorm_bwd_reduce_refuses_width(C):
    """C / 8 = 3 or 12 column threads do not divide the 256-thread block: the host check
    returns the "unsupported" error and launches nothing."""
    lib = L.load()
    M = 16
    y = torch.zeros(M, C, dtype=BF16, device=DEV)
    v = torch.ones(C, device=DEV)
    partial = torch.full((lib.dfu_bn_bwd_blocks(M, C), 2, C), 7.0, device=DEV)
    rc = lib.dfu_bn_bwd_reduce(P(y), P(y), None, 0, None, None, P(v), P(v), M, C, P(partial),
                               ops.stream_ptr())
    assert rc == L.DFU_E_INVALID and "unsupported" in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    assert (partial == 7.0).all()
