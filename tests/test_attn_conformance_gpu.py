"""The attention kernels of csrc/attn.hip against the fp64 references and derived limits of
attn_ref.py (test_attn_ref_cpu.py shows those limits accept a faithful fp32 evaluation
everywhere and reject a lost key, a lost query, a leaked padding key and a short Delta).  Every
element of every output is compared; the references are plain torch operations on the device.

    test_every_kernel   B = 2, H = 3; N = 1, 2 (one tile, 31 / 30 padding keys), 17, 33, 97, 193,
                        225 (16 m + 1: a query alone in its tile; 33, 97, 193, 225 one key past a
                        32-boundary), 197 (the workload), 208 (a multiple of 16, not of 32: a
                        whole padding tile), 255, 256 (no padding); regimes gauss, two_peak,
                        shifted; dfu_attention_fwd, _fwd_f16, _fwd_f32 (N <= 224), _bwd and
                        _bwd_qkv16.  Operands sit in NaN-guarded buffers, outputs start as NaN
                        with guards behind them.  The backward runs from givens: the forward
                        kernel's own o and lse, and an lse shifted by known amounts.
    test_slice_walk     k_attn_fwd's persistent walk: B H = 4 CUs + CUs / 2 + 1 slices at
                        N = 197, so a workgroup sees it = 0 .. 4 (both LDS buffers, the query-tile
                        rotation's wrap at it = 4) and the last round is short; every slice inside
                        the limits, sampled slices bit for bit what the same slice gives alone.
    test_slice_walk_one_extra   B H = CUs + 1: exactly one workgroup has two slices.
    test_far_regime     scores near -110, lse < -100: exp2(-Ls) overflows, which the backward's
                        dQ pass survives only because it masks the padding keys of a partly
                        filled tile.

Each test prints its worst error / limit per kernel and output; test_report prints the maxima.
"""
import pytest
import torch

import attn_ref as R
import gemm_ref as G
from dfu_hip import _lib as L
from dfu_hip import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DH = R.DH
SCALE = DH ** -0.5
NS = [1, 2, 17, 33, 97, 193, 197, 208, 225, 255, 256]
WORST = R.Worst()


def bits(t):
    return t.contiguous().view(G.INT_OF[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def operand(x):
    """A tensor as a device operand with NaN before and after it."""
    return G.Guarded(x.shape[0], x.shape[1], x.shape[1], x.dtype, DEV).set(x.to(DEV))


def output(rows, cols, dtype):
    """An output no kernel has written: NaN everywhere, guards before and after."""
    return G.Guarded(rows, cols, cols, dtype, DEV)


def lse_tail_untouched(lse, N):
    return bool((bits(lse.view[:, N:]) == lse._sentinel()).all())


def forward(kind, qkv, B, H, N, npad=None):
    """One forward launch into fresh guarded outputs; returns {name: Guarded}."""
    lib, D, s = L.load(), H * DH, ops.stream_ptr()
    npad = R.npad(N) if npad is None else npad
    out = {"lse": output(B * H, npad, F32)}
    if kind == "bf16":
        out["o"] = output(B * N, D, BF16)
        rc = lib.dfu_attention_fwd(qkv.ptr(), B, N, H, DH, SCALE, out["o"].ptr(),
                                   out["lse"].ptr(), s)
    elif kind == "f16":
        out["o16"], out["o_bf"] = output(B * N, D, F16), output(B * N, D, BF16)
        rc = lib.dfu_attention_fwd_f16(qkv.ptr(), B, N, H, DH, SCALE, out["o16"].ptr(),
                                       out["o_bf"].ptr(), out["lse"].ptr(), s)
    else:
        out["qkv_bf"], out["o3"] = output(B * N, 3 * D, BF16), output(B * N, 3 * D, BF16)
        out["o_bf"] = output(B * N, D, BF16)
        rc = lib.dfu_attention_fwd_f32(qkv.ptr(), B, N, H, DH, SCALE, npad, out["qkv_bf"].ptr(),
                                       out["o3"].ptr(), out["o_bf"].ptr(), out["lse"].ptr(), s)
    L.check(rc, f"attention forward {kind}")
    torch.cuda.synchronize()
    for name, g in out.items():
        assert g.untouched(), f"{kind} forward N={N}: wrote outside {name}"
    assert lse_tail_untouched(out["lse"], N), f"{kind} forward N={N}: wrote lse columns >= N"
    return out


def check_forward(kind, qkv, out, B, H, N, tag):
    """Every element of o (o16, o_bf, hi + lo) and lse inside its limit, and the bitwise
    relations between the outputs of one launch."""
    q, k, v = R.heads(qkv.view, B, H, N)
    ref = R.fwd_ref(q, k, v, SCALE, kind)
    D = H * DH
    got = {"lse": out["lse"].view[:, :N].reshape(B, H, N)}
    if kind == "bf16":
        got["o"] = R.rows(out["o"].view, B, H, N)
    elif kind == "f16":
        got["o16"] = R.rows(out["o16"].view, B, H, N)
        got["o_bf"] = R.rows(out["o_bf"].view, B, H, N)
    else:
        o3 = out["o3"].view
        hi, lo = o3[:, :D], o3[:, D:2 * D]
        got["o"] = R.rows((hi.double() + lo.double()).contiguous(), B, H, N)
        got["o_bf"] = R.rows(out["o_bf"].view, B, H, N)
        assert same_bits(out["o_bf"].view, hi), f"{tag}: o_bf != hi"
        assert same_bits(o3[:, 2 * D:], hi), f"{tag}: third segment != hi"
        assert same_bits(out["qkv_bf"].view, qkv.view.to(BF16)), f"{tag}: qkv_bf16 != bf16(qkv)"
    res = {n: WORST.add(f"fwd {kind} {n}", R.check(t, ref[n], f"{tag} {kind} {n}"))
           for n, t in got.items()}
    if kind == "f16":
        d = (out["o_bf"].view.double() - out["o16"].view.double()).abs()
        assert (d <= R.pair_limit(out["o16"].view)).all(), f"{tag}: o_bf and o16 too far apart"
    res["lse limit"] = ref["lse"][1].max().item()
    return res


def backward(qkv, o, dout, lse, B, H, N):
    """One backward launch (fp16 qkv: dfu_attention_bwd_qkv16) into a fresh guarded dqkv."""
    lib = L.load()
    dqkv = output(B * N, 3 * H * DH, BF16)
    delta = torch.empty(B * H, R.npad(N), dtype=F32, device=DEV)
    fn = lib.dfu_attention_bwd_qkv16 if qkv.view.dtype == F16 else lib.dfu_attention_bwd
    L.check(fn(qkv.ptr(), o.data_ptr(), dout.ptr(), lse.data_ptr(), B, N, H, DH, SCALE,
               delta.data_ptr(), dqkv.ptr(), ops.stream_ptr()), "attention backward")
    torch.cuda.synchronize()
    assert dqkv.untouched(), f"backward N={N}: wrote outside dqkv"
    return dqkv.view


def check_backward(qkv, o, lse, dout, B, H, N, tag, key):
    """The backward from the givens (o, lse): every element inside its limit; bit-identical
    whatever the lse columns >= N hold; the same again with lse shifted by -1/8, 0, +1/8 per
    query.  qkv fp16: bitwise the bf16 backward on bf16(qkv)."""
    assert o.isfinite().all() and lse[:, :N].isfinite().all(), f"{tag}: non-finite givens"
    qb = qkv.view.to(BF16)
    res = {}
    shift = ((torch.arange(N, device=DEV) % 3).float() - 1) * 0.125
    for what, given in (("", lse), (" lse shifted", torch.cat([lse[:, :N] + shift, lse[:, N:]], 1))):
        first = None
        for fill in (0.0, float("nan"), float("-inf")):
            l = given.clone()
            l[:, N:] = fill
            dqkv = backward(qkv, o, dout, l, B, H, N)
            if first is None:
                first = dqkv
            assert same_bits(dqkv, first), f"{tag}{what}: dqkv depends on lse columns >= N ({fill})"
        ref = R.bwd_ref(qb, o, given, dout.view, SCALE, B, H, N)
        for n, t in zip(("dq", "dk", "dv"), R.heads(first, B, H, N)):
            res[n + what] = WORST.add(f"{key} {n}", R.check(t, ref[n], f"{tag}{what} {n}"))
        if qkv.view.dtype == F16:
            assert same_bits(first, backward(operand(qb), o, dout, given, B, H, N)), \
                f"{tag}{what}: the fp16-qkv backward differs from the bf16 one on bf16(qkv16)"
    return res


def run_all(B, H, N, regime, x3=True):
    """Every kernel on one shape and regime; prints the worst ratios."""
    tag = f"attn B={B} H={H} N={N} {regime}"
    for kind in ("bf16", "f16") + (("x3",) if x3 and N <= 224 else ()):
        qkv_cpu, dout_cpu = R.inputs(B, H, N, regime, dtype=R.DTYPE[kind])
        qkv, dout = operand(qkv_cpu), operand(dout_cpu)
        out = forward(kind, qkv, B, H, N)
        res = check_forward(kind, qkv, out, B, H, N, tag)
        if kind == "x3":
            wide = forward(kind, qkv, B, H, N, npad=R.npad(N) + 32)  # lse stride follows npad
            for name in ("o3", "o_bf", "qkv_bf"):
                assert same_bits(wide[name].view, out[name].view), f"{tag}: npad changes {name}"
            assert same_bits(wide["lse"].view[:, :N], out["lse"].view[:, :N]), \
                f"{tag}: lse rows do not follow the npad argument"
        else:
            o = out["o" if kind == "bf16" else "o_bf"].view
            res.update(check_backward(qkv, o, out["lse"].view, dout, B, H, N, tag,
                                      "bwd" if kind == "bf16" else "bwd_qkv16"))
        print(f"{tag} {kind}: worst err/limit " + ", ".join(f"{n} {r:.3g}" for n, r in res.items()))


@pytest.mark.parametrize("regime", ["gauss", "two_peak", "shifted"])
@pytest.mark.parametrize("N", NS)
def test_every_kernel(N, regime):
    run_all(2, 3, N, regime)


# ------------------------------------------------------------------------------ slice walk
def walk(B, H, N, regime, kind, samples):
    """One forward of B H slices through ops, every slice against the chunked fp64 reference,
    and the sampled slices bit for bit against a launch of that slice alone."""
    tag = f"attn walk B={B} H={H} N={N} {regime} {kind}"
    qkv = R.inputs(B, H, N, regime, dtype=R.DTYPE[kind])[0].to(DEV)
    if kind == "bf16":
        o, lse = ops.attention_fwd(qkv, B, N, H, DH, SCALE)
        outs = {"o": o}
    else:
        o16, o, lse = ops.attention_fwd_f16(qkv, B, N, H, DH, SCALE)
        outs = {"o16": o16, "o_bf": o}
    torch.cuda.synchronize()
    res, CH = {}, 32
    for b0 in range(0, B, CH):
        nb = min(CH, B - b0)
        q, k, v = R.heads(qkv[b0 * N:(b0 + nb) * N], nb, H, N)
        ref = R.fwd_ref(q, k, v, SCALE, kind)
        got = {n: R.rows(t[b0 * N:(b0 + nb) * N], nb, H, N) for n, t in outs.items()}
        got["lse"] = lse[b0 * H:(b0 + nb) * H, :N].reshape(nb, H, N)
        for n, t in got.items():
            r = R.check(t, ref[n], f"{tag} batches {b0}..{b0 + nb - 1} {n}")
            res[n] = max(res.get(n, 0.0), WORST.add(f"walk {kind} {n}", r))
    for s in samples:
        b, h = divmod(s, H)
        one = qkv.view(B, N, 3, H, DH)[b, :, :, h].reshape(N, 3 * DH).contiguous()
        alone = (ops.attention_fwd if kind == "bf16" else ops.attention_fwd_f16)(
            one, 1, N, 1, DH, SCALE)
        for (n, t), a in zip(outs.items(), alone):
            assert same_bits(t.view(B, N, H, DH)[b, :, h].contiguous(), a), \
                f"{tag}: slice {s} {n} differs from the same slice run alone"
        assert same_bits(lse[s, :N].contiguous(), alone[-1][0, :N].contiguous()), \
            f"{tag}: slice {s} lse differs from the same slice run alone"
    print(f"{tag}: {B * H} slices, sampled {samples}, worst err/limit " +
          ", ".join(f"{n} {r:.3g}" for n, r in res.items()))


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("regime", ["gauss", "two_peak"])
def test_slice_walk(regime, kind):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H, N = 3, 197
    B = -(-(4 * cus + cus // 2 + 1) // H)
    BH = B * H
    rounds = -(-BH // cus)
    assert rounds == 5 and BH % cus != 0  # it = 0 .. 4 and a short last round
    samples = sorted({0, BH - 1} | {r * cus + min(37 + r, BH - r * cus - 1) for r in range(rounds)})
    walk(B, H, N, regime, kind, samples)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_slice_walk_one_extra(kind):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    walk(cus + 1, 1, 197, "two_peak", kind, [0, 1, cus - 1, cus])


# ------------------------------------------------------------------------------ far regime
@pytest.mark.parametrize("N", [33, 197, 208, 224])
def test_far_regime(N):
    """Everything finite and inside the limits (check() counts a NaN or inf as outside) where
    every lse is below -100.  Before the dQ pass masked the padding keys of a partly filled
    tile this failed at N = 33 and N = 197 with NaN in every dq element (dk, dv inside their
    limits) and passed at N = 208 and N = 224."""
    run_all(1, 2, N, "far")


def test_report():
    """Runs last in file order; prints what the cases above collected."""
    print(WORST.report("MI355X"))
