"""Shared helper of the BatchNorm conformance tests (test_bn_ref_cpu.py,
test_bn_conformance_gpu.py): fp64 references of what csrc/bn.hip computes, the error bounds of
its kernels derived from the roundings they perform, and an fp32 emulation of the three backward
kernels with named mutations (the CPU test shows the bounds accept the emulation everywhere and
reject every mutation).  Plain torch on whatever device the inputs live on; helper module, no
test.

Notation.  U = 2**-24 bounds the relative error of one correctly rounded fp32 operation (a cast
from fp64 included), UB = 2**-8 that of one round-to-nearest bf16 store (8 significand bits;
2**-9 would be half of it and is wrong).  G(n) = n U / (1 - n U) >= (1 + U)**n - 1 bounds n
compounded fp32 roundings (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1);
every bound below keeps its second-order terms this way, so each is a true upper bound and not
only a first-order one.  hipcc may contract a * b + c into one fma: that removes a rounding,
so every count below is the uncontracted (larger) one.  S64(n) = (n + 8) 2**-52 covers the
fp64 arithmetic of a kernel's n-term fp64 sum plus the handful of fp64 operations behind it,
and the same in the reference; it is ~1e-13 and never decides a comparison.
"""
import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
RED_U = 4        # csrc/bn.hip RED_U: rows in flight per thread and iteration of k_bn_bwd_reduce
FIN_TPS = 128    # csrc/bn.hip FIN_TPS: stats tiles / row-blocks per finalize slice

# what test_bn_tile_stats and test_gemm_stats allow a (sum, M2) record to be off by
REC_SUM_ATOL, REC_SUM_RTOL = 1e-2, 1e-4
REC_M2_ATOL, REC_M2_RTOL = 1e-2, 1e-3


def G(n):
    return n * U / (1.0 - n * U)


def S64(n):
    return (n + 8) * 2.0 ** -52


def f32(x):
    """A Python float as the kernel receives it through a `float` parameter."""
    return float(np.float32(x))


# ------------------------------------------------------------------ inputs
# (M, C) of the conformance cases; test_bn_conformance_gpu.py's docstring says what each reaches
SHAPES = [(1, 8), (2, 8), (300, 64), (257, 72), (2053, 128), (16384, 64), (16533, 64),
          (8200, 2048), (10930, 1536)]
BIG_MEAN = (2053, 128)  # the shape whose activations are 8 + 0.25 randn: mean 32 sigma from zero


def inputs(M, C, seed=500):
    """CPU tensors of one case: bf16 y (2 randn + 0.5; BIG_MEAN: 8 + 0.25 randn), res and dout
    (randn), fp32 gamma (1 + randn / 2) and beta (randn)."""
    gen = torch.Generator().manual_seed(seed + 7 * M + C)

    def rn(*shape):
        return torch.randn(*shape, generator=gen)

    y = 8 + 0.25 * rn(M, C) if (M, C) == BIG_MEAN else 2 * rn(M, C) + 0.5
    return {"y": y.to(BF16), "res": rn(M, C).to(BF16), "dout": rn(M, C).to(BF16),
            "gamma": 1 + 0.5 * rn(C), "beta": rn(C), "dgamma0": rn(C), "dbeta0": rn(C)}


# ------------------------------------------------------------------ host-logic mirrors
def bwd_rows_per_block(M, C):
    """csrc/bn.hip bwd_rows_per_block (C % 8 == 0)."""
    cv = C // 8
    ct_n = min(cv, 64)
    rl_n = 256 // ct_n
    rpb = rl_n * RED_U
    col_groups = cv // ct_n
    while (M + rpb - 1) // rpb * col_groups > 2048 and rpb < M:
        rpb *= 2
    return rpb


def bwd_row_lanes(C):
    return 256 // min(C // 8, 64)


def bwd_admits(C):
    """dfu_bn_bwd_reduce's width check."""
    cv = C // 8
    ct_n = min(cv, 64)
    return C % 8 == 0 and 256 % ct_n == 0 and cv % ct_n == 0


def slices(n):
    """Finalize slices over n stats tiles or row-blocks (gridDim.y with a workspace)."""
    return (n + FIN_TPS - 1) // FIN_TPS


def mask_bits(mask, M, C):
    """bool [M][C] from bn_apply's bitmask (bit e of byte i = element 8 i + e)."""
    sh = torch.arange(8, device=mask.device, dtype=torch.uint8)
    return ((mask.view(-1, 1) >> sh) & 1).view(M, C).bool()


# ------------------------------------------------------------------ forward finalize
def finalize_from_records(stats, M, gamma, beta, eps, momentum, rmean=None, rvar=None):
    """k_bn_finalize from its own input: the fp32 [tiles][2][C] (sum sb, M2 qb) slab, taken as
    given and recombined in fp64 as the kernel specifies,

        mu = sum_t sb_t / M,  var = max(sum_t (qb_t + sb_t^2 / n_t) / M - mu^2, 0),

    n_t = 128 except the last tile's M - 128 (tiles - 1); invstd = 1 / sqrt(var + eps) with eps
    and momentum the fp32 values the kernel receives.  gamma / beta None = 1 / 0.

    Returns {name: (reference fp64, bound fp64)} for mean, invstd, scale, shift and, when given,
    running_mean, running_var.  The kernel does the recombination in fp64 too (order differs:
    S64 slack e_mu, e_var below), so what remains are its last fp32 operations:

    mean = (float)mu                       b_mu = U |mu| + e_mu
    invstd = (float)(1 / sqrt(var + eps))  b_is = U invstd + e_is (1 + U), e_is = e_var
                                           through d invstd / d var = -(var + eps)^-1.5 / 2 at
                                           the smallest var the slack admits
    scale = fl(g * invstd32)               |g| b_is + U |g| (invstd + b_is)    (~ 2 U |scale|)
    shift = fl(b - fl(fl(mu32 * g) * invstd32)): the product carries the casts of mu and
        invstd and two multiplications, the subtraction one rounding of at most |b| + |product|:
        with A = |mu| + b_mu, B = invstd + b_is,
        |g| (A B - |mu| invstd) + G(2) |g| A B + U (|b| + (1 + G(2)) |g| A B)
        (~ U (|beta| + 5 |mu scale|): c = 5 counted from the source; the difference can cancel,
        so the bound is relative to the operands).
    running = fl(fl(fl(1 - m) * r) + fl(m * new32)), new = mu or the unbiased var M / (M - 1)
        (var itself at M = 1), new32 its fp32 cast (b_new = U |new| + slack):
        G(2) |(1 - m) r| + m b_new + U m N + U ((1 + G(2)) |(1 - m) r| + (1 + U) m N),
        N = |new| + b_new          (~ 3 U (|(1 - m) r| + |m new|): two roundings and the add's
        on each operand)."""
    tiles, _, C = stats.shape
    assert tiles == (M + 127) // 128
    s = stats.double()
    n_t = torch.full((tiles, 1), 128.0, dtype=F64, device=stats.device)
    n_t[-1] = M - (tiles - 1) * 128
    sb, qb = s[:, 0], s[:, 1]
    terms = qb + sb * sb / n_t
    mu = sb.sum(0) / M
    var = (terms.sum(0) / M - mu * mu).clamp_min(0.0)
    eps, m = f32(eps), f32(momentum)
    invstd = (var + eps).rsqrt()
    one = torch.ones(C, dtype=F64, device=stats.device)
    g = one if gamma is None else gamma.double()
    b = 0 * one if beta is None else beta.double()

    abs_mu = sb.abs().sum(0) / M
    e_mu = S64(tiles) * abs_mu
    e_var = 3 * S64(tiles) * (terms.abs().sum(0) / M + abs_mu * abs_mu)
    e_is = 0.5 * e_var * ((var - e_var).clamp_min(0.0) + eps) ** -1.5
    b_mu = U * mu.abs() + e_mu
    b_is = U * invstd + e_is * (1 + U)
    A, B = mu.abs() + b_mu, invstd + b_is
    gAB = g.abs() * A * B
    out = {
        "mean": (mu, b_mu),
        "invstd": (invstd, b_is),
        "scale": (g * invstd, g.abs() * b_is + U * g.abs() * B),
        "shift": (b - mu * g * invstd,
                  g.abs() * (A * B - mu.abs() * invstd) + G(2) * gAB
                  + U * (b.abs() + (1 + G(2)) * gAB)),
    }

    def running(r, new, b_new):
        keep = (1.0 - m) * r.double()
        N = new.abs() + b_new
        return (keep + m * new,
                G(2) * keep.abs() + m * b_new + U * m * N
                + U * ((1 + G(2)) * keep.abs() + (1 + U) * m * N))

    if rmean is not None:
        out["running_mean"] = running(rmean, mu, b_mu)
    if rvar is not None:
        bessel = M / (M - 1.0) if M > 1 else 1.0
        unb = var * bessel
        out["running_var"] = running(rvar, unb, U * unb + e_var * bessel * (1 + U))
    return out


def finalize_from_data(x, eps):
    """mean and invstd of the bf16 rows x[M][C] end to end: the fp64 statistics of the data, and
    a bound that admits any (sum, M2) records test_bn_tile_stats / test_gemm_stats accept,
    d_sb_t = 1e-2 + 1e-4 |sb_t|, d_qb_t = 1e-2 + 1e-3 |qb_t| around the exact records of tile t.

    mean: sum_t d_sb_t / M, then the cast.
    var: with exact records sum_t (qb_t + sb_t^2 / n_t) = sum x^2 (each tile's M2 plus n_t
    mean_t^2).  The derivative of (qb_t + sb_t^2 / n_t) / M - (sum sb / M)^2 by sb_t is
    2 sb_t / (n_t M) - 2 mu / M = 2 (mean_t - mu) / M: the first-order error of sb_t CANCELS
    between sb_t^2 / n_t and mu^2 down to the tile mean's distance from the batch mean.  (A
    bound with 2 |mu| d_sb_t / M instead is vacuous for activations whose mean is many standard
    deviations from zero.)  The second-order terms are d_sb_t^2 / (n_t M) and (sum d_sb / M)^2:

        d_var = sum_t (d_qb_t + 2 |mean_t - mu| d_sb_t + d_sb_t^2 / n_t) / M + (sum_t d_sb_t / M)^2

    and the clamp at zero only moves var towards the (non-negative) reference.
    invstd: |d invstd / d var| <= (v + eps)^-1.5 / 2 at the smallest admitted
    v = max(var - d_var, 0), then the cast: U (invstd + e) + e.  Where var + eps is not large
    against d_var (M = 1, 2) the bound is wide by construction; the bound from the records is the sharp one there.

    Returns {"mean": (ref, bound), "invstd": (ref, bound)}."""
    M, C = x.shape
    x64 = x.double()
    tiles = (M + 127) // 128
    mu = x64.mean(0)
    var = ((x64 - mu) ** 2).mean(0)
    eps = f32(eps)
    invstd = (var + eps).rsqrt()
    pad = tiles * 128 - M
    xp = torch.cat([x64, torch.zeros(pad, C, dtype=F64, device=x.device)]).view(tiles, 128, C)
    n_t = torch.full((tiles, 1), 128.0, dtype=F64, device=x.device)
    n_t[-1] = 128 - pad
    sb = xp.sum(1)
    mean_t = sb / n_t
    valid = (torch.arange(tiles * 128, device=x.device).view(tiles, 128, 1) < M)
    qb = (((xp - mean_t[:, None]) ** 2) * valid).sum(1)
    d_sb = REC_SUM_ATOL + REC_SUM_RTOL * sb.abs()
    d_qb = REC_M2_ATOL + REC_M2_RTOL * qb.abs()
    sum_dsb = d_sb.sum(0) / M
    acc = (d_qb + 2 * (mean_t - mu).abs() * d_sb + d_sb * d_sb / n_t).sum(0) / M
    d_var = acc + sum_dsb * sum_dsb + 3 * S64(tiles) * (var + mu * mu)
    e_is = 0.5 * d_var * ((var - d_var).clamp_min(0.0) + eps) ** -1.5
    e_mu = sum_dsb + S64(tiles) * mu.abs()
    return {"mean": (mu, U * (mu.abs() + e_mu) + e_mu),
            "invstd": (invstd, U * (invstd + e_is) + e_is)}


# ------------------------------------------------------------------ forward apply
def apply_ref(y, scale, shift, res, relu):
    """k_bn_apply with the kernel's own fp32 scale / shift as givens: v = y scale + shift (+ res)
    in fp64, out = bf16(act(fl(fmaf(y, scale, shift) + res))).

    The fma rounds once (U |y scale + shift|), the residual add once (U |v32|; with no residual
    it adds an exact zero): e = 2 U (|y scale| + |shift| + |res|) bounds |v32 - v| including the
    second-order term since U |v32| <= U (1 + U) (...).  ReLU is 1-Lipschitz, so
    |act(v32) - act(v)| <= e, and the bf16 store adds UB |act(v32)| <= UB (|act(v)| + e):

        |out - act(v)| <= UB |act(v)| + (1 + UB) e

    Returns (act(v) fp64, bound fp64)."""
    ys = y.double() * scale.double()
    v = ys + shift.double()
    mag = ys.abs() + shift.double().abs()
    if res is not None:
        v = v + res.double()
        mag = mag + res.double().abs()
    if relu:
        v = v.clamp_min(0.0)
    e = 2 * U * (1 + U) * mag
    return v, UB * v.abs() + (1 + UB) * e


# ------------------------------------------------------------------ backward
def bwd_ref(dout, y, keep, mean, invstd, gamma, batch_stats=True, dgamma0=None, dbeta0=None):
    """dfu_bn_bwd with the kernel's fp32 mean / invstd and gamma (None = 1) as givens, in fp64:

        g = keep dout (keep: bool ReLU mask or None), xh = (y - mean) invstd,
        SG = sum g, SGX = sum g xh, k = gamma invstd, m1 = SG / M, m2 = SGX / M
        dy = k (g - m1 - xh m2)   (m1 = m2 = 0 when batch_stats is false)
        dres = g exactly; dbeta = dbeta0 + SG; dgamma = dgamma0 + SGX.

    k_bn_bwd_reduce.  rpb = bwd_rows_per_block rows per block over rl_n row-lanes: a lane adds
    its rpb / rl_n rows in turn, lane 0 then adds the other rl_n - 1 lanes, all fp32.  No term
    passes through more than rpb / rl_n + rl_n - 2 <= rpb additions, so whatever the order
    E_g = G(rpb) sum |g|.  A g xh term is fl(fl(g fl(y - mean)) invstd): three roundings before
    it is added, E_gx = G(rpb + 3) sum |g xh|.  k_bn_bwd_finalize adds the blocks in fp64
    (S64(blocks) of the same sums).

    dbeta[c] += (float)sg: the cast U (|SG| + E_g), the add U (|prev| + |sg32|):
        E_g + U (|SG| + E_g) + U (|prev| + (1 + U) (|SG| + E_g)); dgamma alike with E_gx.

    k_bn_bwd_apply.  d = fma(ka, g, fma(kb, y, kc)), ka = k32 = fl(gamma invstd),
    kb = fl(fl(-k32 m2) invstd), kc = fl(k32 fl(fl(fl(m2 invstd) mean) - m1)), m1 / m2 the fp32
    casts of the fp64 sums over M.  The errors E_g / M and E_gx / M of m1 and m2 pass through
    exactly as in the formula (kb and kc use the same m2: its error multiplies xh, not y and
    mean apart): |k| (E_g / M + |xh| E_gx / M).  The roundings, counted per summand of
    ka g + kb y + kc with the inner and the outer fma's (one each, each at most U times the sum
    of the magnitudes under it):
        k g:              k32 1, outer fma 1                                         = 2
        k m2 invstd y:    k32 1, m2 cast 1, two products 2, inner 1, outer 1         = 6
        k m2 invstd mean: m2 cast 1, two products 2, subtraction 1, product by k32 1,
                          k32 1, inner 1, outer 1                                    = 8
        k m1:             m1 cast 1, subtraction 1, product 1, k32 1, inner 1, outer 1 = 6
    so R = |k| (E_g / M + |xh| E_gx / M) + G(8) |k| (|g| + m2' invstd (|y| + |mean|) + m1'),
    m1' = |m1| + E_g / M and m2' alike (the roundings act on the computed values).  The term in
    |y| + |mean| is what the cancellation in kb y + kc costs when the mean is far from zero.
    The bf16 store adds UB |d| <= UB (|dy| + R):

        |dy_kernel - dy| <= UB |dy| + (1 + UB) R

    With batch_stats false m1 = m2 = 0 and R = G(8) |k g|: test_batchnorm_bwd_eval_mode's bound
    plus the rounding of k.

    Returns {"dy": (ref, bound), "dgamma": ..., "dbeta": ..., "dres": g fp64}."""
    M, C = y.shape
    dev = y.device
    g = dout.double()
    if keep is not None:
        g = g * keep
    y64, mu, istd = y.double(), mean.double(), invstd.double()
    xh = (y64 - mu) * istd
    gx = g * xh
    SG, SGX = g.sum(0), gx.sum(0)
    rpb = bwd_rows_per_block(M, C)
    blocks = (M + rpb - 1) // rpb
    E_g = (G(rpb) + S64(blocks)) * g.abs().sum(0)
    E_gx = (G(rpb + 3) + S64(blocks)) * gx.abs().sum(0)

    def acc(prev, S, E):
        p = torch.zeros(C, dtype=F64, device=dev) if prev is None else prev.double()
        return p + S, E + U * (S.abs() + E) + U * (p.abs() + (1 + U) * (S.abs() + E))

    k = istd if gamma is None else gamma.double() * istd
    if batch_stats:
        m1, m2, Em1, Em2 = SG / M, SGX / M, E_g / M, E_gx / M
    else:
        m1 = m2 = Em1 = Em2 = torch.zeros(C, dtype=F64, device=dev)
    dy = k * (g - m1 - xh * m2)
    R = k.abs() * (Em1 + xh.abs() * Em2) + G(8) * k.abs() * (
        g.abs() + (m2.abs() + Em2) * istd * (y64.abs() + mu.abs()) + m1.abs() + Em1)
    return {"dy": (dy, UB * dy.abs() + (1 + UB) * R),
            "dgamma": acc(dgamma0, SGX, E_gx),
            "dbeta": acc(dbeta0, SG, E_g),
            "dres": g}


def worst(got, ref_bound):
    """(largest error / bound, number of elements outside the bound).  An element is inside
    only if err <= bound holds: a NaN or inf in the output (or in the reference or the bound,
    which a NaN given would cause) counts as outside with ratio inf.  A zero bound admits only
    a zero error (ratio 0 there)."""
    ref, bound = ref_bound
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(bad & ~(ratio > 1), torch.full_like(ratio, float("inf")), ratio)
    return ratio.max().item(), int(bad.sum())


def check(got, ref_bound, what):
    """Assert |got - ref| <= bound at every element; returns the worst error / bound."""
    assert got.shape == ref_bound[0].shape, (what, got.shape, ref_bound[0].shape)
    ratio, n_bad = worst(got, ref_bound)
    assert n_bad == 0, (f"{what}: {n_bad} of {got.numel()} outside the bound, "
                        f"worst err/bound {ratio:.3g}")
    return ratio


# ------------------------------------------------------------------ fp32 emulation
MUTATIONS = ("drop_m1", "drop_row", "div_m_minus_1", "reduce_ignores_mask")


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 values is exact in fp64, the sum rounds
    once there and once more to fp32 (differs from a true fma only at fp64 rounding ties)."""
    return (a.double() * b.double() + c.double()).float()


def emulate_bwd(dout, y, keep, mean, invstd, gamma, batch_stats=True, dgamma0=None, dbeta0=None,
                mutation=None):
    """k_bn_bwd_reduce, k_bn_bwd_finalize and k_bn_bwd_apply in fp32 torch operations with the
    kernels' summation order: per row-lane sums in row order, lane 0 adding the other lanes in
    fp32, the blocks in fp64, m1 / m2 cast to fp32, kb / kc formed as the source writes them and
    the two fmas.  An emulation for the CPU test of the bounds, not the GPU kernel.

    mutation: None, or one of MUTATIONS -- "drop_m1" (m1 = 0 in the apply), "drop_row" (the last
    row of the last block missing from the reduce), "div_m_minus_1" (m1, m2 over M - 1),
    "reduce_ignores_mask" (the reduce sums dout, the apply masks correctly).

    Returns (dy bf16, dres bf16, dgamma fp32, dbeta fp32)."""
    assert mutation is None or mutation in MUTATIONS
    M, C = y.shape
    d32, y32 = dout.float(), y.float()
    g = d32 if keep is None else torch.where(keep, d32, torch.zeros_like(d32))
    gr = d32 if mutation == "reduce_ignores_mask" else g
    term = (gr * (y32 - mean)) * invstd
    if mutation == "drop_row":
        gr, term = gr.clone(), term.clone()
        gr[M - 1] = 0
        term[M - 1] = 0
    rpb, rl_n = bwd_rows_per_block(M, C), bwd_row_lanes(C)
    blocks = (M + rpb - 1) // rpb
    pad = torch.zeros(blocks * rpb - M, C)

    def block_sums(v):
        # row r0 + k rl_n + rl belongs to lane rl, its k-th row; rows past M add an exact zero
        v = torch.cat([v, pad]).view(blocks, rpb // rl_n, rl_n, C)
        lanes = v[:, 0].clone()
        for k in range(1, rpb // rl_n):
            lanes = lanes + v[:, k]
        tot = lanes[:, 0].clone()
        for l in range(1, rl_n):
            tot = tot + lanes[:, l]
        return tot.double().sum(0)

    sg, sgx = block_sums(gr), block_sums(term)
    dbeta = (torch.zeros(C) if dbeta0 is None else dbeta0.clone()) + sg.float()
    dgamma = (torch.zeros(C) if dgamma0 is None else dgamma0.clone()) + sgx.float()
    k = invstd.clone() if gamma is None else gamma * invstd
    den = float(M - 1) if mutation == "div_m_minus_1" else float(M)
    zero = torch.zeros(C)
    m1 = (sg / den).float() if batch_stats else zero
    m2 = (sgx / den).float() if batch_stats else zero
    if mutation == "drop_m1":
        m1 = zero
    kb = (-k * m2) * invstd
    kc = k * ((m2 * invstd) * mean - m1)
    d = _fma32(k, g, _fma32(kb, y32, kc))
    return d.to(BF16), g.to(BF16), dgamma, dbeta
