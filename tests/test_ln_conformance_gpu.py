"""The LayerNorm kernels (csrc/ln.hip k_ln_fwd and k_ln_bwd, csrc/precise.hip k_ln_fwd_x3 as
dfu_layernorm_fwd_x3 / _h16) and the reductions behind them (csrc/elem.hip k_reduce_partials,
k_reduce_partials_batch) against the fp64 references, derived bounds and bit-exact orders of
ln_ref.py (test_ln_ref_cpu.py shows those bounds accept a faithful fp32 evaluation everywhere
and reject a wrong divisor, a wrong eps, a bf16 mean, a one-pass variance, a skipped tail
chunk, a missing row, a stale row pair, a dy read through bf16, a column sum of dx and a
truncated bf16 copy).  Every element of every output is compared; the references are plain
torch operations on the device.

    forward D    4 one float4 | 256 one per lane | 260 lane 0 takes a second | 768 |
                 1020 lane 63 lacks its fourth | 1024        (x3 / h16: 8, 512, 520, 768, 1016,
                 1024, the same edges of 8-float chunks)
    forward rows 1 | 4 one block | 5 a second block with one wave
    backward rows 1 half a pair | 2 | 3 | 8 a wave | 9 | 31 | 32 a block | 33 | 65 | 1100 =
                 35 blocks: reduce lanes 0..2 add a second partial
    backward D   4 | 256 | 260 | 764 | 768 NV = 3's limit | 772 the smallest NV = 4 | 1024
    regimes      gauss everywhere; flat, offset, outlier, const at D = 768 and at one ragged D
    strides      ld = D + 4 on some cases, the class-token stride 197 * 768 on one (x; in the
                 backward gx and gx_bf16 too); pad columns and one row past the end hold
                 sentinels, pad columns of the inputs NaN

The backward is checked FROM GIVENS (the forward kernel's own mean / rstd, and the same moved by
a few hundred ulps), with bf16 and fp32 dy, with and without gx_bf16 and gsum_partial, and with
non-zero initial gx, dgamma and dbeta.  Outputs that are fully written start as NaN.  Each test
prints its worst error / bound per quantity.
"""
import pytest
import torch

import ln_ref as R
from dfu_hip import _lib as L
from dfu_hip import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
EPS = R.LN_EPS
SENT = 7.0
NAN = float("nan")

_IN = {}


def P(t):
    return None if t is None else t.data_ptr()


def inp(rows, D, regime):
    """One case's inputs on the device, made once and never written."""
    if (rows, D, regime) not in _IN:
        _IN[(rows, D, regime)] = {k: v.to(DEV) for k, v in R.inputs(rows, D, regime).items()}
    return _IN[(rows, D, regime)]


def strided(v, ld, fill, dtype=None):
    """[rows + 1][ld] filled with `fill`, v in its [:rows, :D] corner."""
    rows, D = v.shape
    buf = torch.full((rows + 1, ld), fill, dtype=dtype or v.dtype, device=DEV)
    buf[:rows, :D] = v
    return buf


def intact(buf, rows, D, what):
    """The pad columns and the row past the end still hold the sentinel."""
    assert (buf[:rows, D:] == SENT).all(), f"{what}: pad columns written"
    assert (buf[rows:] == SENT).all(), f"{what}: a row past the end written"


def ulps(got, ref):
    """Worst |got - ref| in units of the last place of ref's fp32 binade."""
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs())) - 23)
    return ((got.double() - ref).abs() / ulp).max().item()


def report(tag, worst, extra=""):
    print(f"{tag}: worst err/bound " + ", ".join(f"{q} {r:.3f}" for q, r in worst.items())
          + extra)


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("rows,D,ld,regime", R.FWD_CASES)
def test_ln_fwd(rows, D, ld, regime, kind):
    d = inp(rows, D, regime)
    ldo = D if ld in (D, R.CLS_LD) else ld
    xb = strided(d["x"], ld, NAN)
    ob = strided(torch.full((rows, D), NAN, device=DEV), ldo, SENT, BF16 if kind == "bf16" else F32)
    mean = torch.full((rows + 1,), SENT, device=DEV)
    rstd = torch.full((rows + 1,), SENT, device=DEV)
    mean[:rows] = rstd[:rows] = NAN
    ops.layernorm_fwd(xb, ld, rows, D, d["gamma"], d["beta"], EPS, ob, ldo, kind == "bf16", mean,
                      rstd)
    ref = R.fwd_ref(d["x"], d["gamma"], d["beta"], EPS, kind)
    what = f"ln_fwd {kind} ({rows}, {D}) ld {ld} {regime}"
    worst = {"mean": R.check(mean[:rows], ref["mean"], f"{what} mean"),
             "rstd": R.check(rstd[:rows], ref["rstd"], f"{what} rstd"),
             "out": R.check(ob[:rows, :D], ref["out"], f"{what} out")}
    report(what, worst, f"; rstd {ulps(rstd[:rows], ref['rstd'][0]):.2f} ulp")
    intact(ob, rows, D, what)
    assert mean[rows] == SENT and rstd[rows] == SENT, f"{what}: statistics past the end written"
    if regime == "const":
        want = d["beta"].expand(rows, D).to(ob.dtype).contiguous()
        assert R.same_bits(ob[:rows, :D].contiguous(), want), f"{what}: a constant row != beta"
        assert torch.equal(mean[:rows], d["x"][:, 0]), f"{what}: a constant row's mean"
    # without the statistics outputs (the eval-mode call) the output is the same
    ob2 = strided(torch.full((rows, D), NAN, device=DEV), ldo, SENT, ob.dtype)
    ops.layernorm_fwd(xb, ld, rows, D, d["gamma"], d["beta"], EPS, ob2, ldo, kind == "bf16", None,
                      None)
    assert R.same_bits(ob[:rows, :D].contiguous(), ob2[:rows, :D].contiguous())
    intact(ob2, rows, D, what)


@pytest.mark.parametrize("kind", ["x3", "h16"])
@pytest.mark.parametrize("rows,D,ld,regime", R.X3_CASES)
def test_ln_fwd_x3_h16(rows, D, ld, regime, kind):
    d = inp(rows, D, regime)
    xb = strided(d["x"], ld, NAN)
    wide = 3 * D if kind == "x3" else D
    o1 = strided(torch.full((rows, wide), NAN, device=DEV), wide, SENT,
                 BF16 if kind == "x3" else F16)
    ob = strided(torch.full((rows, D), NAN, device=DEV), D, SENT, BF16)
    mean = torch.full((rows + 1,), SENT, device=DEV)
    rstd = torch.full((rows + 1,), SENT, device=DEV)
    mean[:rows] = rstd[:rows] = NAN
    fn = ops.layernorm_fwd_x3 if kind == "x3" else ops.layernorm_fwd_h16
    fn(xb, ld, rows, D, d["gamma"], d["beta"], EPS, o1, ob, mean, rstd)
    ref = R.fwd_ref(d["x"], d["gamma"], d["beta"], EPS, kind)
    what = f"ln_fwd {kind} ({rows}, {D}) ld {ld} {regime}"
    if kind == "x3":
        hi, lo, third = o1[:rows, :D], o1[:rows, D:2 * D], o1[:rows, 2 * D:]
        first = hi.double() + lo.double()
        assert R.same_bits(ob[:rows].contiguous(), hi.contiguous()), f"{what}: out_bf16 != hi"
        assert R.same_bits(third.contiguous(), hi.contiguous()), f"{what}: third segment != hi"
    else:
        first = o1[:rows]
    worst = {"mean": R.check(mean[:rows], ref["mean"], f"{what} mean"),
             "rstd": R.check(rstd[:rows], ref["rstd"], f"{what} rstd"),
             "out": R.check(first, ref["out"], f"{what} out"),
             "out_bf": R.check(ob[:rows], ref["out_bf"], f"{what} out_bf")}
    report(what, worst, f"; rstd {ulps(rstd[:rows], ref['rstd'][0]):.2f} ulp")
    intact(o1, rows, wide, what)
    intact(ob, rows, D, what)
    assert mean[rows] == SENT and rstd[rows] == SENT, f"{what}: statistics past the end written"
    if regime == "const":
        beta = d["beta"].expand(rows, D)
        assert R.same_bits(ob[:rows].contiguous(), beta.to(BF16).contiguous()), \
            f"{what}: a constant row != beta"
        if kind == "h16":
            assert R.same_bits(o1[:rows].contiguous(), beta.to(F16).contiguous())
        else:
            want_lo = (beta - beta.to(BF16).float()).to(BF16)
            assert R.same_bits(lo.contiguous(), want_lo.contiguous())
        assert torch.equal(mean[:rows], d["x"][:, 0]), f"{what}: a constant row's mean"


# ------------------------------------------------------------------------------ backward
def run_bwd(d, rows, D, ld, dyk, mean, rstd, with_bf, with_gsum):
    """dfu_layernorm_bwd through the C ABI into fresh buffers.  Returns gx, gx_bf16 (or None),
    partial [blocks][2][D], gsum_partial (or None) with every sentinel checked."""
    lddy = D if ld in (D, R.CLS_LD) else ld
    nb = R.bwd_blocks(rows)
    assert nb == L.load().dfu_ln_bwd_blocks(rows)
    dyb = strided(d[dyk], lddy, NAN)
    xb = strided(d["x"], ld, NAN)
    gxb = strided(d["gx0"], ld, SENT)
    g16 = torch.full((rows + 1, ld), SENT, dtype=BF16, device=DEV) if with_bf else None
    part = torch.full((nb + 1, 2, D), SENT, device=DEV)
    gsp = torch.full((nb + 1, D), SENT, device=DEV) if with_gsum else None
    part[:nb] = NAN
    if with_gsum:
        gsp[:nb] = NAN
    L.check(L.load().dfu_layernorm_bwd(P(dyb), lddy, int(dyk == "dy16"), P(xb), ld, P(mean),
                                       P(rstd), P(d["gamma"]), rows, D, P(gxb), ld, P(g16),
                                       P(part), P(gsp), ops.stream_ptr()), "dfu_layernorm_bwd")
    what = f"ln_bwd ({rows}, {D}) ld {ld}"
    intact(gxb, rows, D, f"{what} gx")
    assert (part[nb] == SENT).all(), f"{what}: a partial block past the end written"
    if with_bf:
        intact(g16, rows, D, f"{what} gx_bf16")
    if with_gsum:
        assert (gsp[nb] == SENT).all(), f"{what}: a gsum block past the end written"
    return (gxb[:rows, :D].contiguous(), g16[:rows, :D].contiguous() if with_bf else None,
            part[:nb].contiguous(), gsp[:nb].contiguous() if with_gsum else None)


@pytest.mark.parametrize("dyk", ["dy16", "dy32"])
@pytest.mark.parametrize("rows,D,ld,regime", R.BWD_CASES)
def test_ln_bwd(rows, D, ld, regime, dyk):
    d = inp(rows, D, regime)
    nb = R.bwd_blocks(rows)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    scratch = torch.empty(rows, D, device=DEV)
    ops.layernorm_fwd(d["x"], D, rows, D, d["gamma"], d["beta"], EPS, scratch, D, False, mean, rstd)
    for shifted, (mu, rs) in enumerate(((mean, rstd), R.perturbed(mean, rstd))):
        ref = R.bwd_ref(d["x"], d[dyk], d["gamma"], mu, rs, d["gx0"])
        what = f"ln_bwd {dyk} ({rows}, {D}) ld {ld} {regime} shifted={shifted}"
        gx, g16, part, gsp = run_bwd(d, rows, D, ld, dyk, mu, rs, True, True)
        worst = {"gx": R.check(gx, ref["gx"], f"{what} gx"),
                 "dgamma_p": R.check(part[:, 0], ref["dgamma_p"], f"{what} dgamma partial"),
                 "dbeta_p": R.check(part[:, 1], ref["dbeta_p"], f"{what} dbeta partial"),
                 "gsum_p": R.check(gsp, ref["gsum_p"], f"{what} gsum partial")}
        report(what, worst)
        # what the kernel only adds or only rounds: bit for bit
        assert R.same_bits(part[:, 1].contiguous(), R.block_row_sums(d[dyk], rows)), \
            f"{what}: dbeta partial is not the row-order sum of dy"
        assert R.same_bits(gsp, R.block_row_sums(gx, rows)), \
            f"{what}: gsum_partial is not the row-order sum of the stored gx"
        assert torch.equal(g16.view(torch.int16), R.bf16_rne_bits(gx)), \
            f"{what}: gx_bf16 is not the round-to-nearest-even of the stored gx"
        # the options change nothing else
        for with_bf, with_gsum in ((False, True), (True, False), (False, False)):
            o = run_bwd(d, rows, D, ld, dyk, mu, rs, with_bf, with_gsum)
            assert R.same_bits(o[0], gx) and R.same_bits(o[2], part), \
                f"{what}: gx_bf16={with_bf} gsum={with_gsum} changes gx or the partials"
            assert o[1] is None or R.same_bits(o[1], g16)
            assert o[3] is None or R.same_bits(o[3], gsp)
        # the reductions, from the kernel's own partials, into non-zero dgamma / dbeta / gsum
        want_g = R.reduce_partials(part[:, 0], d["dgamma0"])
        want_b = R.reduce_partials(part[:, 1], d["dbeta0"])
        want_s = R.reduce_partials(gsp, d["dbeta0"])
        dg, db = d["dgamma0"].clone(), d["dbeta0"].clone()
        L.check(L.load().dfu_reduce_partials(P(part), nb, 2, D, P(dg), P(db), ops.stream_ptr()),
                "dfu_reduce_partials")
        assert R.same_bits(dg, want_g) and R.same_bits(db, want_b), f"{what}: reduce_partials"
        dg1, db1 = d["dgamma0"].clone(), d["dbeta0"].clone()
        for a, b_ in ((dg1, None), (None, db1)):  # one output at a time leaves the other
            L.check(L.load().dfu_reduce_partials(P(part), nb, 2, D, P(a), P(b_),
                                                 ops.stream_ptr()), "dfu_reduce_partials")
        assert R.same_bits(dg1, want_g) and R.same_bits(db1, want_b)
        gs = d["dbeta0"].clone()
        ops.reduce_partials_add(gsp, gs)
        assert R.same_bits(gs, want_s), f"{what}: reduce_partials_add of gsum_partial"
        dg2, db2, gs2 = d["dgamma0"].clone(), d["dbeta0"].clone(), d["dbeta0"].clone()
        batch = ops.PartialReductions()
        batch.add(part, dg2, D, stride=2 * D, offset=0)
        batch.add(part, db2, D, stride=2 * D, offset=D)
        batch.add(gsp, gs2, D)
        batch.flush()
        assert R.same_bits(dg2, want_g) and R.same_bits(db2, want_b) and R.same_bits(gs2, want_s), \
            f"{what}: reduce_partials_batch"


def test_ln_bwd_through_ops_matches_the_c_abi():
    """ops.layernorm_bwd (what the model calls) gives the C ABI's bits at the class-token case."""
    rows, D, ld, regime = R.BWD_CASES[2]
    assert ld == R.CLS_LD and rows == 3
    d = inp(rows, D, regime)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    out = torch.empty(rows, D, device=DEV)
    xb = strided(d["x"], ld, NAN)
    ops.layernorm_fwd(xb, ld, rows, D, d["gamma"], d["beta"], EPS, out, D, False, mean, rstd)
    gx, g16, part, gsp = run_bwd(d, rows, D, ld, "dy32", mean, rstd, True, True)
    gxb = strided(d["gx0"], ld, SENT)
    gb = torch.full((rows + 1, ld), SENT, dtype=BF16, device=DEV)
    dg, db = d["dgamma0"].clone(), d["dbeta0"].clone()
    gsp2 = ops.layernorm_bwd(d["dy32"], D, False, xb, ld, mean, rstd, d["gamma"], rows, D, gxb, ld,
                             gb, dg, db, gsum=True)
    assert R.same_bits(gxb[:rows, :D].contiguous(), gx) and R.same_bits(gsp2, gsp)
    assert R.same_bits(gb[:rows, :D].contiguous(), g16)
    assert R.same_bits(dg, R.reduce_partials(part[:, 0], d["dgamma0"]))
    assert R.same_bits(db, R.reduce_partials(part[:, 1], d["dbeta0"]))
    intact(gxb, rows, D, "ops gx")
    intact(gb, rows, D, "ops gx_bf16")
