"""Shared helper of the LayerNorm conformance tests (test_ln_ref_cpu.py,
test_ln_conformance_gpu.py): fp64 references of what csrc/ln.hip (k_ln_fwd, k_ln_bwd),
csrc/precise.hip (k_ln_fwd_x3) and csrc/elem.hip (k_reduce_partials) compute, the error bounds of
those kernels counted from the roundings they perform, the bit-exact orders of the outputs that
are only added or only rounded, and an fp32 emulation of the forward and the backward with named
mutations (the CPU test shows the bounds accept the emulation everywhere and reject every
mutation).  Plain torch on whatever device the inputs live on; helper module, no test.

Notation as in bn_ref.py: U = 2**-24 one fp32 rounding, UB = 2**-8 one bf16 store, G(n) the
compounded bound of n fp32 roundings; a * b + c is counted uncontracted (two roundings).  Sums
are bounded by their depth: a term that passes through k additions, whatever the order, carries
at most G(k) of the sum of the magnitudes (Higham, section 4.2).  wave_sum (common.h) is a
6-level butterfly: 6 additions on every term.  n_c = ceil(D / (64 w)) is the number of w-float
chunks the busiest lane (lane 0) holds, w = 4 in ln.hip and 8 in precise.hip; chunks past the
row are zeros whose additions are exact, and the first addition into a zero accumulator is exact.
"""
import numpy as np
import torch

from bn_ref import G, U, UB, check, worst  # noqa: F401  (re-exported for the tests)

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
UH = 2.0 ** -11          # one round-to-nearest fp16 store (11 significand bits)
H_TINY = 2.0 ** -25      # half the spacing of fp16's subnormals: the store's error below 2**-14
U_SPLIT = 2.0 ** -17     # st_triple8 / split8: hi = bf16(f), lo = bf16(f - hi).  f - hi is exact
                         # and |f - hi| <= 2**-8 2**e for 2**e <= |f| < 2**(e + 1) (half of bf16's
                         # spacing 2**(e - 7)); below 2**(e - 8) bf16's spacing is at most
                         # 2**(e - 16), so bf16(lo) is off by at most 2**(e - 17) <= 2**-17 |f|
                         # (at |f - hi| = 2**(e - 8) itself lo is exact).
RSQRT_ULPS = 2           # rsqrtf (k_ln_fwd) and 1.0f / sqrtf (k_ln_fwd_x3) are not correctly
                         # rounded; the ROCm installation ships no copy of HIP's accuracy table,
                         # so 2 ulps is ASSUMED (one ulp = 2 U relative at most).  Measured:
                         # rstd within 1.06 ulp of fp64, its variance included (EXPERIMENTS.md).
LNB_ROWS = 32            # csrc/ln.hip LNB_ROWS: rows per backward block, 8 per wave
LN_EPS = 1e-6
CLS_LD = 197 * 768       # TokenNormFn's row stride: the class-token rows of [B][197][768]


def f32(x):
    """A Python float as the kernel receives it through a `float` parameter."""
    return float(np.float32(x))


def bwd_blocks(rows):
    """csrc/ln.hip dfu_ln_bwd_blocks."""
    return (rows + LNB_ROWS - 1) // LNB_ROWS


def bwd_nv(D):
    """dfu_layernorm_bwd's template choice: float4 chunks per lane."""
    return 3 if D <= 768 else 4


# ------------------------------------------------------------------ inputs
REGIMES = ("gauss", "flat", "offset", "outlier", "const")

FWD_D = (4, 256, 260, 768, 1020, 1024)   # one float4 | one per lane | lane 0 takes a second |
                                         # the workload | lane 63 lacks its fourth | MAXV full
X3_D = (8, 512, 520, 768, 1016, 1024)    # the same edges with 8-float chunks, MAXV = 2
FWD_ROWS = (1, 4, 5)                     # one wave | one full block | a second block of one wave
BWD_ROWS = (1, 2, 3, 8, 9, 31, 32, 33, 65, 1100)  # half a pair | a pair | .. | a wave | a second
                                         # wave | a block less one | a block | a second block |
                                         # three | 35 blocks: reduce lanes 0..2 take a second
BWD_D = (4, 256, 260, 764, 768, 772, 1024)        # .. | NV = 3's limit | the smallest NV = 4 | full


def _cases(pairs, ragged, full_rows, ragged_rows):
    """(rows, D, ld, regime): every D and every row count with gauss, every other regime at
    D = 768 and at one ragged D; ld > D (sentinel columns) on some, CLS_LD on one."""
    out = [(r, D, ld, "gauss") for r, D, ld in pairs]
    for regime in REGIMES[1:]:
        out.append((full_rows, 768, 768, regime))
        out.append((ragged_rows, ragged, ragged + 4, regime))
    return out


FWD_CASES = _cases([(1, 4, 4), (4, 256, 260), (5, 260, 260), (5, 768, 768), (4, 768, CLS_LD),
                    (4, 1020, 1024), (1, 1024, 1024)], 260, 5, 5)
X3_CASES = _cases([(1, 8, 8), (4, 512, 516), (5, 520, 520), (5, 768, 768), (4, 768, CLS_LD),
                   (4, 1016, 1024), (1, 1024, 1024)], 520, 5, 5)
BWD_CASES = _cases([(1, 4, 4), (2, 256, 260), (3, 768, CLS_LD), (8, 260, 260), (9, 764, 768),
                    (31, 768, 768), (32, 772, 776), (33, 1024, 1024), (65, 768, 768),
                    (1100, 768, 768)], 260, 33, 9)


def inputs(rows, D, regime, seed=700):
    """CPU tensors of one case.  x by regime:
      gauss    3 randn + 1, gamma, beta ~ randn: what the older LayerNorm tests use
      flat     1 + 1e-3 randn: variance ~ eps, so eps changes rstd by a factor sqrt 2
      offset   8 + 0.25 randn: the mean 32 sigma from zero (bn_ref.BIG_MEAN); a one-pass
               variance E x^2 - mean^2 cancels six digits here
      outlier  randn with columns 1 and D - 2 at +150 and -150, gamma = 1 + 0.1 randn: a
               SYNTHETIC stand-in for the few large channels of a trained ViT's residual
               stream; nobody has measured that these are ViT-B's values
      const    even rows 2.5, odd rows 0 (what a never-written row looks like): sum, mean and
               x - mean are exact, the variance is 0
    dy32 ~ randn (fp32) and dy16 its own bf16 draw; gx0, dgamma0, dbeta0 ~ randn, non-zero
    initial values of everything the backward adds into."""
    assert regime in REGIMES
    gen = torch.Generator().manual_seed(seed + 13 * rows + D + 1000 * REGIMES.index(regime))

    def rn(*shape):
        return torch.randn(*shape, generator=gen)

    gamma, beta = rn(D), rn(D)
    if regime == "gauss":
        x = 3 * rn(rows, D) + 1
    elif regime == "flat":
        x = 1 + 1e-3 * rn(rows, D)
    elif regime == "offset":
        x = 8 + 0.25 * rn(rows, D)
    elif regime == "outlier":
        x = rn(rows, D)
        x[:, 1], x[:, D - 2] = 150.0, -150.0
        gamma = 1 + 0.1 * rn(D)
    else:
        x = torch.zeros(rows, D)
        x[0::2] = 2.5
    return {"x": x.float(), "gamma": gamma, "beta": beta, "dy32": rn(rows, D),
            "dy16": rn(rows, D).to(BF16), "gx0": rn(rows, D), "dgamma0": rn(D), "dbeta0": rn(D)}


def perturbed(mean, rstd):
    """The givens moved by a few hundred ulps (mean up 300, rstd down 200; a zero mean stays
    zero): a second, equally valid set of givens for the backward.  A backward that recomputes
    the statistics from x would agree with the unperturbed set only."""
    return (mean * (1 + 300 * 2.0 ** -23)).float(), (rstd * (1 - 200 * 2.0 ** -23)).float()


# ------------------------------------------------------------------ forward reference
FWD_KINDS = ("f32", "bf16", "x3", "h16")


def fwd_ref(x, gamma, beta, eps, kind):
    """mean, rstd and out of the fp32 rows x[rows][D] in fp64, eps the fp32 value the kernel
    receives: mu = sum x / D, var = sum (x - mu)^2 / D, rstd = (var + eps)^-1/2,
    v = (x - mu) rstd gamma + beta.  kind: "f32" / "bf16" (k_ln_fwd, w = 4), "x3" / "h16"
    (k_ln_fwd_x3, w = 8).

    mean = wave_sum(s) / (float)D.  k_ln_fwd: `s += v[i][0] + v[i][1] + v[i][2] + v[i][3]` is
    s + (((v0 + v1) + v2) + v3): 3 additions inside the chunk, n_c - 1 into s, 6 in wave_sum, the
    division: n_c + 9 roundings.  k_ln_fwd_x3: `s += v[i][e]` one by one: 8 n_c - 1, 6, the
    division: 8 n_c + 6.  b_mu = G(.) sum |x| / D.

    rstd = rsqrtf(wave_sum(q) / (float)D + eps) (x3: 1.0f / sqrtf(..)).  The sum of squares is
    taken about the kernel's own mean m = mu + d, |d| <= b_mu: sum (x - m)^2 / D = var + d^2
    exactly.  Each term of `const float d = v[i][e] - mean; q += d * d` has 2 roundings, then
    w n_c - 1 additions in the lane (one by one in both kernels), 6 in wave_sum and the
    division: k = w n_c + 8 roundings on positive terms, so q / D = (var + d^2) (1 + t),
    |t| <= G(k); the eps addition rounds once more:
        |arg - (var + eps)| <= e_arg = ((1 + G(k)) b_mu^2 + G(k) var) (1 + U) + U (var + eps).
    With rho = e_arg / (var + eps), arg^-1/2 is off by at most eta = (1 - rho)^-1/2 - 1
    relative, and rsqrtf / 1.0f / sqrtf by RSQRT_ULPS ulps of the computed value:
        b_r = rstd (eta + 2 U RSQRT_ULPS (1 + eta)).

    out.  `o[e] = (v[i][e] - mean) * rstd * g[e] + b[e]` is fl(fl(fl(fl(x - m) r) g) + b): the
    product p = (x - mu) rstd g is taken with the kernel's m and r and rounded 3 times (the
    subtraction, two products), the addition once (at most U (|p^| + |b|)).  With
    A = |x - mu| + b_mu, R = rstd + b_r:
        E = |g| (A R - |x - mu| rstd) + G(3) |g| A R + U ((1 + G(3)) |g| A R + |b|).
    "f32": E.  "bf16" and the bf16 copies: UB |v| + (1 + UB) E.  "h16": UH |v| + (1 + UH) E +
    H_TINY.  "x3" hi + lo: U_SPLIT (|v| + E) + E.

    Returns {"mean", "rstd", "out"[, "out_bf"]: (reference fp64, bound fp64)}; "out" is what the
    first output buffer holds (x3: hi + lo)."""
    assert kind in FWD_KINDS
    rows, D = x.shape
    w = 8 if kind in ("x3", "h16") else 4
    n_c = (D + 64 * w - 1) // (64 * w)
    x64 = x.double()
    mu = x64.sum(1) / D
    xc = x64 - mu[:, None]
    var = (xc * xc).sum(1) / D
    eps = f32(eps)
    rstd = (var + eps) ** -0.5
    b_mu = G(n_c + 9 if w == 4 else 8 * n_c + 6) * x64.abs().sum(1) / D
    k = w * n_c + 8
    e_arg = ((1 + G(k)) * b_mu * b_mu + G(k) * var) * (1 + U) + U * (var + eps)
    eta = (1 - e_arg / (var + eps)) ** -0.5 - 1
    b_r = rstd * (eta + 2 * U * RSQRT_ULPS * (1 + eta))
    g, b = gamma.double(), beta.double()
    v = xc * rstd[:, None] * g + b
    AR = (xc.abs() + b_mu[:, None]) * (rstd + b_r)[:, None]
    E = (g.abs() * (AR - xc.abs() * rstd[:, None]) + G(3) * g.abs() * AR
         + U * ((1 + G(3)) * g.abs() * AR + b.abs()))
    out = {"mean": (mu, b_mu), "rstd": (rstd, b_r)}
    bf = (v, UB * v.abs() + (1 + UB) * E)
    if kind == "f32":
        out["out"] = (v, E)
    elif kind == "bf16":
        out["out"] = bf
    elif kind == "h16":
        out["out"], out["out_bf"] = (v, UH * v.abs() + (1 + UH) * E + H_TINY), bf
    else:
        out["out"], out["out_bf"] = (v, U_SPLIT * (v.abs() + E) + E), bf
    return out


# ------------------------------------------------------------------ backward reference
def _block_sum(v, rows):
    """fp64 [rows][D] -> [blocks][D], the rows of each backward block summed."""
    nb = bwd_blocks(rows)
    pad = torch.zeros(nb * LNB_ROWS - rows, v.shape[1], dtype=v.dtype, device=v.device)
    return torch.cat([v, pad]).view(nb, LNB_ROWS, -1).sum(1)


def bwd_ref(x, dy, gamma, mean, rstd, gx0):
    """k_ln_bwd FROM GIVENS, in fp64: x, dy (bf16 or fp32), gamma, the fp32 mean / rstd actually
    passed in (never recomputed here) and the initial gx:

        xh = (x - mean) rstd,  s1 = sum dy g / D,  s2 = sum dy g xh / D,
        gx = gx0 + rstd (dy g - s1 - xh s2),
        partial[blk][0] = sum_rows dy xh,  partial[blk][1] = sum_rows dy,
        gsum_partial[blk] = sum_rows gx     (rows of the block; n_c = ceil(D / 256) below).

    The kernel's statements: `xh = (xv - mu) * rs`, `dxh = dy * gm`, `s1 += dxh`,
    `s2 += dxh * xh`, `dg += dy * xh`, `db += dy`, `s1 = wave_sum(s1) / (float)D` (s2 alike),
    `g[e] += rs * (dy * gm - s1 - xh * s2)`, `gs += g[e]`, and wave_reduce's
    `red[0][d] + red[1][d] + red[2][d] + red[3][d]`.

    s1: fl(dy g) 1 rounding, 4 n_c - 1 additions in the lane, 6 in wave_sum, the division:
        b_s1 = G(4 n_c + 7) sum |dy g| / D.
    s2: fl(fl(dy g) xh), xh = fl(fl(x - mean) rstd): 1 + 2 + 1 roundings, then as s1:
        b_s2 = G(4 n_c + 10) sum |dy g xh| / D.
    dx = fl(rstd fl(fl(fl(dy g) - s1) - fl(xh s2))), the roundings per summand:
        dy g:   product 1, two subtractions 2, product by rstd 1                    = 4
        s1:     two subtractions 2, product by rstd 1 (on |s1| + b_s1)              = 3
        xh s2:  xh 2, product 1, subtraction 1, product by rstd 1 (on |s2| + b_s2)  = 5
        R = rstd (b_s1 + |xh| b_s2 + G(4) |dy g| + G(3) (|s1| + b_s1) + G(5) |xh| (|s2| + b_s2))
    gx = fl(gx0 + dx^): one more rounding of at most |gx0| + |dx| + R:
        b_gx = R + U (|gx0| + |dx| + R).
    dgamma partial: fl(dy xh) 3 roundings, 7 additions over the wave's 8 rows, 3 over the 4
    waves: G(13) sum_rows |dy xh|.  dbeta partial: 7 + 3 additions, G(10) sum_rows |dy| (the GPU
    test checks it bit for bit as well; this bound serves the CPU test's mutations, and with
    bf16 dy, whose 8-bit significands mostly add exactly in fp32, the measured error is near
    zero by the data and not by a slack count).  gsum
    partial: the same 10 additions of the kernel's gx: sum_rows b_gx (1 + G(10)) +
    G(10) sum_rows |gx| (on the GPU: bit for bit from the kernel's own gx).

    Returns {"gx", "dgamma_p", "dbeta_p", "gsum_p": (reference fp64, bound fp64)}."""
    rows, D = x.shape
    n_c = (D + 255) // 256
    x64, d, g = x.double(), dy.double(), gamma.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x64 - mu) * rs
    dg_ = d * g
    s1 = dg_.sum(1, keepdim=True) / D
    s2 = (dg_ * xh).sum(1, keepdim=True) / D
    b_s1 = G(4 * n_c + 7) * dg_.abs().sum(1, keepdim=True) / D
    b_s2 = G(4 * n_c + 10) * (dg_ * xh).abs().sum(1, keepdim=True) / D
    dx = rs * (dg_ - s1 - xh * s2)
    R = rs.abs() * (b_s1 + xh.abs() * b_s2 + G(4) * dg_.abs() + G(3) * (s1.abs() + b_s1)
                    + G(5) * xh.abs() * (s2.abs() + b_s2))
    gx = gx0.double() + dx
    b_gx = R + U * (gx0.double().abs() + dx.abs() + R)
    return {"gx": (gx, b_gx),
            "dgamma_p": (_block_sum(d * xh, rows), G(13) * _block_sum((d * xh).abs(), rows)),
            "dbeta_p": (_block_sum(d, rows), G(10) * _block_sum(d.abs(), rows)),
            "gsum_p": (_block_sum(gx, rows),
                       (1 + G(10)) * _block_sum(b_gx, rows) + G(10) * _block_sum(gx.abs(), rows))}


# ------------------------------------------------------------------ bit-exact orders
def same_bits(a, b):
    """Equal shape, dtype and bit patterns (-0 != +0, NaN payloads compared)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    v = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def block_row_sums(v, rows):
    """k_ln_bwd's db / gs accumulation and wave_reduce on fp32 v[rows][D]: each wave adds its 8
    rows in row order into a zero accumulator, then red[0] + red[1] + red[2] + red[3].  Rows past
    `rows` add +0, which leaves a sum that started from +0 as it is.  -> fp32 [blocks][D]."""
    nb = bwd_blocks(rows)
    pad = torch.zeros(nb * LNB_ROWS - rows, v.shape[1], dtype=F32, device=v.device)
    w = torch.cat([v.float(), pad]).view(nb, 4, LNB_ROWS // 4, -1)
    acc = torch.zeros_like(w[:, :, 0])
    for r in range(LNB_ROWS // 4):
        acc = acc + w[:, :, r]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def bf16_rne_bits(v):
    """Round-to-nearest-even fp32 -> bf16 on the bit patterns (finite values), as int16: what
    common.h pack2 (v_cvt_pk_bf16_f32) stores."""
    b = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)


def reduce_partials(partial, out0):
    """k_reduce_partials / k_reduce_partials_batch on fp32 partial[blocks][D] (a strided view is
    fine): block-lane bl adds blocks bl, bl + 32, .. into a zero accumulator, lane 0 then adds
    lanes 1..31 in order, then out += s.  -> fp32 [D]."""
    nb, D = partial.shape
    trips = (nb + 31) // 32
    pad = torch.zeros(trips * 32 - nb, D, dtype=F32, device=partial.device)
    p = torch.cat([partial, pad]).view(trips, 32, D)
    lanes = torch.zeros_like(p[0])
    for t in range(trips):
        lanes = lanes + p[t]
    s = lanes[0].clone()
    for l in range(1, 32):
        s = s + lanes[l]
    return out0 + s


# ------------------------------------------------------------------ fp32 emulation
FWD_MUTATIONS = ("var_div_d_minus_1", "eps_x1000", "mean_bf16", "stats_skip_last_chunk",
                 "one_pass_variance")
BWD_MUTATIONS = ("means_div_d_minus_1", "s1_skip_last_chunk", "s2_skip_last_chunk",
                 "drop_last_row_of_block", "stale_pair", "dy_rounded_to_bf16",
                 "gsum_before_update", "bf16_truncate")


def _fma32(a, b, c):
    """fmaf on fp32 tensors (see bn_ref._fma32)."""
    return (a.double() * b.double() + c.double()).float()


def _lanes(v, w, n):
    """fp32 [rows][D] -> [rows][n][64][w]: chunk i of lane l holds columns w (l + 64 i) + e;
    columns past D are zero."""
    rows, D = v.shape
    pad = torch.zeros(rows, n * 64 * w - D, dtype=F32)
    return torch.cat([v.float(), pad], 1).view(rows, n, 64, w)


def _chunk_index(n):
    return torch.arange(64)[None, :] + 64 * torch.arange(n)[:, None]   # j of [chunk][lane]


def _wave_sum(s):
    """common.h wave_sum on [rows][64]: v += shfl_xor(v, o) for o = 32 .. 1."""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, 0]


def emulate_fwd(x, gamma, beta, eps, kind, contract=False, mutation=None):
    """k_ln_fwd ("f32", "bf16") or k_ln_fwd_x3 ("x3", "h16") in fp32 torch operations in the
    kernel's order; contract: every a * b + c as one fma (what hipcc may do) instead of two
    roundings.  An emulation for the CPU test of the bounds, not the GPU kernel.

    mutation: None or one of FWD_MUTATIONS -- "var_div_d_minus_1" (Bessel's divisor),
    "eps_x1000", "mean_bf16" (the mean rounded to bf16 before use), "stats_skip_last_chunk" (sum
    and sum of squares miss the row's last float4 / 8-float chunk), "one_pass_variance"
    (E x^2 - mean^2).

    Returns {"mean", "rstd", "out"[, "out_bf"]}: out fp32 / bf16 / the triple's hi + lo (fp32;
    "hi", "lo" too) / fp16."""
    assert kind in FWD_KINDS and (mutation is None or mutation in FWD_MUTATIONS)
    rows, D = x.shape
    w, n = (8, 2) if kind in ("x3", "h16") else (4, 4)
    nv = D // w
    v = _lanes(x, w, n)
    j = _chunk_index(n)
    valid = j < nv
    if mutation == "stats_skip_last_chunk":
        valid = valid & (j != nv - 1)
    vs = torch.where(valid[None, :, :, None], v, torch.zeros_like(v))
    s = torch.zeros(rows, 64)
    for i in range(n):
        if w == 4:
            s = s + (((vs[:, i, :, 0] + vs[:, i, :, 1]) + vs[:, i, :, 2]) + vs[:, i, :, 3])
        else:
            for e in range(w):
                s = s + vs[:, i, :, e]
    Df = torch.tensor(float(D), dtype=F32)
    mean = _wave_sum(s) / Df
    if mutation == "mean_bf16":
        mean = mean.to(BF16).float()
    q = torch.zeros(rows, 64)
    for i in range(n):
        for e in range(w):
            d = v[:, i, :, e] - mean[:, None]
            if mutation == "one_pass_variance":
                d = v[:, i, :, e]
            q = torch.where(valid[i][None], _fma32(d, d, q) if contract else q + d * d, q)
    den = torch.tensor(float(D - 1), dtype=F32) if mutation == "var_div_d_minus_1" else Df
    var = _wave_sum(q) / den
    if mutation == "one_pass_variance":
        var = var - mean * mean
    arg = var + torch.tensor(f32(eps * 1000 if mutation == "eps_x1000" else eps), dtype=F32)
    rstd = 1.0 / arg.sqrt() if w == 8 else arg.double().rsqrt().float()
    g, b = _lanes(gamma[None], w, n), _lanes(beta[None], w, n)
    t = (v - mean[:, None, None, None]) * rstd[:, None, None, None]
    o = _fma32(t, g, b) if contract else t * g + b
    o = o.reshape(rows, -1)[:, :D]
    out = {"mean": mean, "rstd": rstd}
    if kind == "f32":
        out["out"] = o
    elif kind == "bf16":
        out["out"] = o.to(BF16)
    elif kind == "h16":
        out["out"], out["out_bf"] = o.to(F16), o.to(BF16)
    else:
        hi = o.to(BF16)
        lo = (o - hi.float()).to(BF16)
        out.update(hi=hi, lo=lo, out=hi.float() + lo.float(), out_bf=hi)
    return out


def emulate_bwd(x, dy, gamma, mean, rstd, gx0, contract=False, mutation=None):
    """k_ln_bwd in fp32 torch operations in the kernel's order (per-lane sums over chunk and
    element, wave_sum, the row pair's update, the per-wave row sums and the 4-wave reduce).

    mutation: None or one of BWD_MUTATIONS -- "means_div_d_minus_1" (s1, s2 over D - 1),
    "s1_skip_last_chunk" / "s2_skip_last_chunk" (the row's last float4 missing from the sum),
    "drop_last_row_of_block" (row 31 of a block missing from dgamma / dbeta), "stale_pair" (the
    second row of a pair uses the first's mean and rstd), "dy_rounded_to_bf16" (an fp32 dy read
    through bf16), "gsum_before_update" (gsum_partial sums dx, not the updated gx),
    "bf16_truncate" (the bf16 copy truncated).

    Returns {"gx" fp32 [rows][D], "gx_bf" int16 bits, "partial" fp32 [blocks][2][D],
    "gsum_p" fp32 [blocks][D]}."""
    assert mutation is None or mutation in BWD_MUTATIONS
    rows, D = x.shape
    NV, nv = bwd_nv(D), D // 4
    d32 = dy.float()
    if mutation == "dy_rounded_to_bf16":
        d32 = d32.to(BF16).float()
    mu, rs = mean.clone(), rstd.clone()
    if mutation == "stale_pair":
        mu[1::2], rs[1::2] = mean[0:rows - rows % 2:2], rstd[0:rows - rows % 2:2]
    xv, dv, g0 = _lanes(x, 4, NV), _lanes(d32, 4, NV), _lanes(gx0, 4, NV)
    gm = _lanes(gamma[None], 4, NV)
    mu4, rs4 = mu[:, None, None, None], rs[:, None, None, None]
    xh = (xv - mu4) * rs4
    dxh = dv * gm
    last = (_chunk_index(NV) == nv - 1)[None, :, :, None]
    zero = torch.zeros_like(dxh)
    t1 = torch.where(last, zero, dxh) if mutation == "s1_skip_last_chunk" else dxh
    t2 = torch.where(last, zero, dxh) if mutation == "s2_skip_last_chunk" else dxh
    s1, s2 = torch.zeros(rows, 64), torch.zeros(rows, 64)
    for i in range(NV):
        for e in range(4):
            s1 = s1 + t1[:, i, :, e]
            s2 = _fma32(t2[:, i, :, e], xh[:, i, :, e], s2) if contract \
                else s2 + t2[:, i, :, e] * xh[:, i, :, e]
    den = torch.tensor(float(D - 1 if mutation == "means_div_d_minus_1" else D), dtype=F32)
    s1 = (_wave_sum(s1) / den)[:, None, None, None]
    s2 = (_wave_sum(s2) / den)[:, None, None, None]
    if contract:
        t = _fma32(-xh, s2.expand_as(xh), _fma32(dv, gm.expand_as(dv), -s1.expand_as(dv)))
        g = _fma32(rs4.expand_as(t), t, g0)
    else:
        t = dv * gm - s1 - xh * s2
        g = g0 + rs4 * t
    cols = lambda a: a.reshape(rows, -1)[:, :D].contiguous()
    gx = cols(g)
    dr = d32.clone()
    if mutation == "drop_last_row_of_block":
        dr[LNB_ROWS - 1::LNB_ROWS] = 0
    term_x = cols(xh)
    # dg += dy * xh row by row within the wave, then the 4 waves
    nb = bwd_blocks(rows)
    pad = torch.zeros(nb * LNB_ROWS - rows, D)
    a = torch.cat([dr, pad]).view(nb, 4, LNB_ROWS // 4, D)
    b = torch.cat([term_x, pad]).view(nb, 4, LNB_ROWS // 4, D)
    acc = torch.zeros(nb, 4, D)
    for r in range(LNB_ROWS // 4):
        acc = _fma32(a[:, :, r], b[:, :, r], acc) if contract else acc + a[:, :, r] * b[:, :, r]
    dgp = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    dbp = block_row_sums(dr, rows)
    gsp = block_row_sums(cols(rs4 * t) if mutation == "gsum_before_update" else gx, rows)
    bits = bf16_rne_bits(gx)
    if mutation == "bf16_truncate":
        bits = (gx.view(torch.int32) >> 16).to(torch.int16)
    return {"gx": gx, "gx_bf": bits, "partial": torch.stack([dgp, dbp], 1), "gsum_p": gsp}


# ------------------------------------------------------------------ the older tests' tolerances
OLD_TOL_MUTATIONS = ("fwd_var_div_d_minus_1", "fwd_eps_1e-3", "fwd_mean_bf16",
                     "fwd_stats_skip_last_float4", "bwd_means_div_d_minus_1",
                     "bwd_s1_skip_last_float4", "bwd_bf16_truncate")


def old_tolerance_ratio(rows, D, ld, mutation, draw=None):
    """What test_layernorm_fwd_bwd and test_kernel_edges_gpu.py's test_layernorm_fwd_shapes /
    test_layernorm_bwd_shapes accept: the named wrong kernel evaluated in fp64 against the right
    one, as the worst |err| / (atol + rtol |ref|) over the output it changes (out: 3e-2, 1e-2;
    dx: 1e-3, 1e-3; gx_bf16 against gx: 2e-2, 1e-2).  Below 1 passes.  draw None: the inputs the
    edge tests themselves draw (_ln_inputs: seed 300 + D, x = 3 randn(rows, ld) + 1, gamma, beta;
    bf16 dy seed 310 with lddy = ld + 4, gx0 seed 311); an integer: another draw of the same
    distributions."""
    assert mutation in OLD_TOL_MUTATIONS
    seeds = (300 + D, 310, 311) if draw is None else (9000 + 3 * draw, 9001 + 3 * draw,
                                                      9002 + 3 * draw)
    gen = torch.Generator().manual_seed(seeds[0])
    x = (torch.randn(rows, ld, generator=gen) * 3 + 1)[:, :D].double()
    g = torch.randn(D, generator=gen).double()
    b = torch.randn(D, generator=gen).double()
    dy = torch.randn(rows, ld + 4, generator=torch.Generator().manual_seed(seeds[1]))
    dy = dy.to(BF16)[:, :D].double()
    gx0 = torch.randn(rows, ld, generator=torch.Generator().manual_seed(seeds[2]))[:, :D].double()

    def stats(ncols, den, eps, mean_bf=False):
        mu = x[:, :ncols].sum(1, keepdim=True) / D
        if mean_bf:
            mu = mu.to(BF16).double()
        var = ((x[:, :ncols] - mu) ** 2).sum(1, keepdim=True) / den
        return mu, (var + eps) ** -0.5

    def ratio(got, ref, atol, rtol):
        return ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()

    mu, rs = stats(D, D, 1e-6)
    if mutation.startswith("fwd"):
        m2, r2 = stats(D - 4 if mutation == "fwd_stats_skip_last_float4" else D,
                       D - 1 if mutation == "fwd_var_div_d_minus_1" else D,
                       1e-3 if mutation == "fwd_eps_1e-3" else 1e-6, mutation == "fwd_mean_bf16")
        return ratio((x - m2) * r2 * g + b, (x - mu) * rs * g + b, 3e-2, 1e-2)
    xh, dg_ = (x - mu) * rs, dy * g
    s1, s2 = dg_.sum(1, keepdim=True) / D, (dg_ * xh).sum(1, keepdim=True) / D
    gx = gx0 + rs * (dg_ - s1 - xh * s2)
    if mutation == "bwd_bf16_truncate":
        f = gx.float()
        trunc = (f.view(torch.int32) & -65536).view(F32)
        return ratio(trunc.double(), gx, 2e-2, 1e-2)
    if mutation == "bwd_means_div_d_minus_1":
        s1, s2 = s1 * D / (D - 1), s2 * D / (D - 1)
    else:
        s1 = dg_[:, :D - 4].sum(1, keepdim=True) / D
    return ratio(gx0 + rs * (dg_ - s1 - xh * s2), gx, 1e-3, 1e-3)
