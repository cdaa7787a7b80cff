"""Shared helper of the attention conformance tests (test_attn_ref_cpu.py,
test_attn_conformance_gpu.py): fp64 references of what csrc/attn.hip computes, the error limits
of its kernels derived from the roundings they perform, four input regimes, and an fp32
emulation of k_attn_fwd and k_attn_bwd_fused with named mutations (the CPU test shows the limits
accept the emulation everywhere and reject every mutation).  Plain torch on whatever device the
inputs live on; helper module, no test.

Notation (gemm_ref's).  EPS = 2**-23 bounds the relative error of one fp32 operation in any
rounding mode.  UB = 2**-8 that of one round-to-nearest bf16 conversion (8 significand bits),
UH = 2**-11 that of an fp16 one, which below 2**-14 (fp16 subnormals) is 2**-25 absolute instead.
half_ulp is gemm_ref.half_ulp, for the rounding of a stored output.  An fp32-accumulated MFMA
contraction of K exactly representable products (bf16 x bf16 has 16 significant bits, fp16 x
fp16 22) is off by at most acc(K) sum |a| |b|, acc(K) = 2 (K + 5) EPS: gemm_ref.gemm_bound with
one split (K - 1 additions in whatever order the MFMA and the chain of MFMAs take; the factor 2
covers (1 + EPS)**K - 1 for every K here).  Factors (1 + x) are multiplied out instead of
linearised, so second-order terms stay inside every limit; TINY = 2**-100 per element covers
what is not relative at all (v_exp_f32 flushing results below 2**-126 to zero, bf16 subnormals).

Three assumptions, for want of a documented figure: v_exp_f32 (__builtin_amdgcn_exp2f) is
taken as accurate to 1 ulp (relative EPS) on normal results, which is what csrc/attn.hip's own
comment on fast_exp2 relies on; logf as accurate to 2 ulp (the HIP math API documents 1 ulp;
doubled); 1.0f / l as at most 3 ulp (hipcc's default is the correctly rounded division, 2.5 ulp
is the fast one).  None of them is near a dominant term of any limit.
"""
import math

import numpy as np
import torch

from gemm_ref import EPS, half_ulp

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
UB = 2.0 ** -8
UH = 2.0 ** -11
UH_ABS = 2.0 ** -25
X3 = 3.0 * 2.0 ** -16 * (1 + 2.0 ** -7)
TINY = 2.0 ** -100
LOG2E = math.log2(math.e)
LOG2E_F = float(np.float32(1.4426950408889634))  # csrc/attn.hip LOG2E
DH = 64
KINDS = ("bf16", "f16", "x3")
DTYPE = {"bf16": BF16, "f16": F16, "x3": F32}
REGIMES = ("gauss", "two_peak", "shifted", "far")
SHIFT = {"shifted": 1.9375, "far": 3.75}


def f32(x):
    """A Python float as the kernel receives it through a `float` parameter."""
    return float(np.float32(x))


def acc(K):
    return 2.0 * (K + 5) * EPS


def npad(N):
    """csrc/attn.hip dfu_attention_npad: N rounded up to a multiple of 32."""
    return (N + 31) // 32 * 32


# ------------------------------------------------------------------ inputs
def inputs(B, H, N, regime, seed=0, dtype=BF16):
    """CPU tensors of one case in the kernels' layout: qkv [B*N][3*H*64] and dout [B*N][H*64]
    (bf16), every value exactly representable in `dtype` (the operand type of the kernel under
    test: bf16, fp16, or fp32 for the x3 forward, whose lo halves are then non-zero).

    gauss     unit normals.
    two_peak  per (b, h): code = random +-1 [N][64], k = 1.5 code, q_i = code[s(i)] + code[t(i)]
              with s(i) = N - 1 - i, t(i) = (s(i) + ceil(N / 2)) mod N; v and dout unit normals.
              scale q_i . k_j is 12 at j = s(i) and j = t(i) (24 where they coincide: N = 1) and
              1.5 sqrt(2) standard normal elsewhere, so each query puts about half its mass on two
              keys and P (1 - P) is O(1) there: every output depends to first order on both.  The
              last query (alone in its tile at N = 16 m + 1) attends key 0, query 0 the last real
              key of a partially padded tile.
    shifted   q = 0.25 randn + 1.9375 u, k = 0.25 randn - 1.9375 u, u = random +-1 [64] per
              (b, h): every score is about -30, so a zero-score padding key outweighs the row.
    far       the same with 3.75: scores about -110, exp(-lse) overflows fp32.
    """
    assert regime in REGIMES
    gen = torch.Generator().manual_seed(1000 * seed + 7 * N + 13 * B + H + 97 * REGIMES.index(regime))

    def rn(*shape):
        return torch.randn(*shape, generator=gen, dtype=F64)

    def pm(*shape):
        return torch.randint(0, 2, shape, generator=gen).to(F64) * 2 - 1

    v, dout = rn(B, H, N, DH), rn(B, H, N, DH)
    if regime == "gauss":
        q, k = rn(B, H, N, DH), rn(B, H, N, DH)
    elif regime == "two_peak":
        code = pm(B, H, N, DH)
        s = N - 1 - torch.arange(N)
        t = (s + (N + 1) // 2) % N
        q, k = code[:, :, s] + code[:, :, t], 1.5 * code
    else:
        u = SHIFT[regime] * pm(B, H, 1, DH)
        q, k = 0.25 * rn(B, H, N, DH) + u, 0.25 * rn(B, H, N, DH) - u
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * DH)
    dout = dout.permute(0, 2, 1, 3).reshape(B * N, H * DH)
    return qkv.to(dtype), dout.to(BF16)


def heads(t, B, H, N):
    """[B*N][3*H*64] -> q, k, v as [B][H][N][64] (views)."""
    return t.view(B, N, 3, H, DH).permute(2, 0, 3, 1, 4).unbind(0)


def rows(t, B, H, N):
    """[B*N][H*64] -> [B][H][N][64] (view)."""
    return t.view(B, N, H, DH).permute(0, 2, 1, 3)


def unrows(t):
    """[B][H][N][64] -> [B*N][H*64]."""
    B, H, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * DH)


# ------------------------------------------------------------------ forward
def _exp_rel(ea):
    """Relative error of v_exp_f32 at an argument off by ea: 2**ea (1 + EPS) - 1."""
    return torch.expm1(math.log(2.0) * ea) * (1 + EPS) + EPS


def fwd_ref(q, k, v, scale, kind):
    """Softmax attention o = softmax(scale q k^T) v and lse = logsumexp(scale q k^T) in fp64 of
    q, k, v [..., N, 64] (values of the kernel's operand type), scale the fp32 value the kernel
    receives.  Returns {name: (reference, limit)}: "o" and "lse" (bf16); "o16", "o_bf", "lse"
    (f16); "o" = hi + lo, "o_bf", "lse" (x3).  Counted from k_attn_fwd / k_attn_fwd_x3:

    Scores.  s = sum_d k q on the MFMA: 64 exact products, eS = acc(64) A, A = sum_d |q| |k|.
    x3: x = hi + lo + r with |lo| <= UB |x| and |r| <= UB |x - hi| <= 2**-16 |x| (gemm_ref's
    2**-18 takes bf16's unit roundoff as 2**-9; bn_ref explains why it is 2**-8); the
    kernel forms lo hi + hi lo + hi hi and drops lo lo + r x' + x r' <= X3 |x| |x'|,
    X3 = 3 2**-16 (1 + 2**-7); 192 products are accumulated: eS = (acc(192) + X3) A.

    Exponent argument.  mx is the largest computed score (fmaxf and the shuffles are exact), so
    |mx - m| <= eSm = max_j eS.  With c0 = scale log2(e), pi_j = p*_j / sum p*_j for
    p*_j = 2**((S_j - mx) c0) whatever mx is.  The kernel has c = fl(scale LOG2E) (LOG2E's own
    rounding 2**-24 and the product's: |c - c0| <= EPS c0), b = fl(-mx c) and a_j = s_j c + b,
    either one fma or a rounded product and a rounded sum (the larger count is taken):
        |a_j - (S_j - mx) c0| <= c eS_j + EPS c0 |S_j - mx|      (score error, error of c)
                                 + EPS |mx c|                     (b)
                                 + EPS |s_j c| + EPS |a_j|        (product, sum)
    =: ea_j, evaluated with |mx| <= |m| + eSm, |s_j| <= |S_j| + eS_j, |S_j - mx| <= m - S_j + eSm
    and c <= (1 + EPS) c0.  v_exp_f32 adds EPS (assumed, see the module docstring):
    p_j = p*_j (1 + rho_j), |rho_j| <= rp_j = 2**ea_j (1 + EPS) - 1.  A masked key has
    a = -inf and p = 0 exactly.

    Row sum.  l adds NPAD terms in fp32, no term through more than n additions (bf16 / f16:
    two chains of 2 KT packed adds, their sum, two shuffles: n = NPAD / 8 + 3; x3: one chain of
    4 KT and two shuffles: n = NPAD / 4 + 2), of the unrounded p:
    l = l* (1 + lam), |lam| <= RL = sum_j pi_j ((1 + rp_j) (1 + EPS)**n - 1), l* = sum_j p*_j.

    P V.  P is rounded to the operand type: bf16 p (1 + UB); fp16 p (1 + UH) + UH_ABS (p <= 1
    can be an fp16 subnormal); x3 ph + pl with the three-product form again (1 + X3).  The
    products are exact and accumulated over NPAD (x3: 3 NPAD) terms: (1 + acc(.)) on each.
    o32 = fl(acc fl(1 / l)): (1 + 3 EPS) (1 + EPS).  Together
        |o32 - o| <= sum_j pi_j |v_jd| ((1 + rp_j) (1 + u_P) (1 + acc) (1 + 3 EPS) (1 + EPS)
                                       / (1 - RL) - 1)  [+ fp16: UH_ABS sum_j |v_jd| F / l*]
    =: e32 (F the same factors without rp; l* >= 2**(-c0 eSm) since the key at the true maximum
    has S_j - mx >= -eSm).  The dominant term is u_P sum_j pi_j |v_jd|.
    The store: half_ulp(|o| + e32) of bf16 (o, o_bf) or fp16 (o16); x3's hi + lo leaves
    a remainder <= UB * UB (|o| + e32) of the fp32 o32 (split_f4).

    lse = fl(fl(mx scale) + logf(l)) against mx scale + ln l*, which is the exact lse for any
    mx: EPS |mx scale| + |ln(1 + lam)| <= -log1p(-RL), + 2 EPS |ln l| for logf (assumed 2 ulp),
    + EPS |lse_computed| for the sum.
    """
    assert kind in KINDS
    q64, k64, v64 = q.double(), k.double(), v.double()
    N = q64.shape[-2]
    NP = npad(N)
    scale = f32(scale)
    c0 = scale * LOG2E
    S = q64 @ k64.transpose(-1, -2)
    A = q64.abs() @ k64.abs().transpose(-1, -2)
    eS = (acc(192) + X3) * A if kind == "x3" else acc(64) * A
    m = S.max(-1, keepdim=True).values
    eSm = eS.max(-1, keepdim=True).values
    lse_ref = torch.logsumexp(S * scale, -1)
    pi = torch.exp(S * scale - lse_ref.unsqueeze(-1))
    o_ref = pi @ v64

    c_hi = c0 * (1 + EPS)
    gap = (m - S) + eSm
    mxa = m.abs() + eSm
    a_abs = gap * c_hi
    ea = c_hi * eS + EPS * c0 * gap + EPS * mxa * c_hi + EPS * (S.abs() + eS) * c_hi
    ea = (ea + EPS * a_abs) / (1 - EPS)
    rp = _exp_rel(ea)
    n_sum = NP // 4 + 2 if kind == "x3" else NP // 8 + 3
    RL = (pi * ((1 + rp) * (1 + EPS) ** n_sum - 1)).sum(-1, keepdim=True)
    u_p = {"bf16": UB, "f16": UH, "x3": X3}[kind]
    F = (1 + u_p) * (1 + acc(3 * NP if kind == "x3" else NP)) * (1 + 3 * EPS) * (1 + EPS) / (1 - RL)
    W = pi * ((1 + rp) * F - 1)
    e32 = W @ v64.abs() + TINY
    if kind == "f16":
        lstar_min = torch.exp2(-c0 * eSm)
        e32 = e32 + UH_ABS * F / lstar_min * v64.abs().sum(-2, keepdim=True)

    lse_abs = lse_ref.abs()
    mxs = (mxa * scale).squeeze(-1)
    dl = -torch.log1p(-RL.squeeze(-1))
    ln_l = (lse_ref - m.squeeze(-1) * scale).abs() + eSm.squeeze(-1) * scale + dl
    e_lse = EPS * mxs + dl + 2 * EPS * ln_l
    e_lse = (e_lse + EPS * (lse_abs + e_lse)) * (1 + EPS) + TINY

    mag = o_ref.abs() + e32
    out = {"lse": (lse_ref, e_lse)}
    if kind == "bf16":
        out["o"] = (o_ref, e32 + half_ulp(mag, BF16))
    elif kind == "f16":
        out["o16"] = (o_ref, e32 + half_ulp(mag, F16))
        out["o_bf"] = (o_ref, e32 + half_ulp(mag, BF16))
    else:
        out["o"] = (o_ref, e32 + UB * UB * mag)
        out["o_bf"] = (o_ref, e32 + half_ulp(mag, BF16))
    return out


def pair_limit(o16):
    """o_bf and o16 are roundings of the same fp32 value x: |o_bf - o16| <= half_ulp_bf16(x) +
    half_ulp_f16(x), evaluated at |o16| + half_ulp_f16(o16) >= |x|."""
    x = o16.double().abs()
    x = x + half_ulp(x, F16)
    return half_ulp(x, BF16) + half_ulp(x, F16)


# ------------------------------------------------------------------ backward from givens
def bwd_ref(qkv, o_given, lse_given, dout, scale, B, H, N):
    """k_attn_bwd_fused as the exact fp64 function of what it is handed: qkv [B*N][3*H*64] and
    o_given, dout [B*N][H*64] (bf16 values), lse_given [B*H][>= N] fp32 (columns >= N are
    ignored, as the kernel ignores them), scale the fp32 value:

        P = exp(scale S - lse_given), Delta = sum_d dout o_given, dP = dout V^T,
        dS = P (dP - Delta), dq = scale dS K, dk = scale dS^T Q, dv = P^T dout.

    o_given and lse_given are whatever is passed: the kernel forward's own outputs, or an lse
    perturbed on purpose.  Returns {"dq" | "dk" | "dv": (reference, limit)} as [B][H][N][64].
    A non-finite value in any given makes every limit NaN, which check() counts as outside.

    Staging.  Delta: 8 exact products added serially from 0 and three shuffle additions, no term
    through more than 11: eD = ((1 + EPS)**11 - 1) sum_d |dout o|.  Ls = fl(lse LOG2E):
    |Ls - lse log2(e)| <= EPS |lse| log2(e) (LOG2E's rounding and the product's).

    P.  a = fmaf(s, c, -Ls), one rounding; s from 64 exact products: eS = acc(64) A.
        |a - (S scale - lse) log2(e)| <= c eS + EPS c0 |S| + EPS |lse| log2(e) + EPS |a|
    =: ea, p = P (1 + rho), |rho| <= rp = 2**ea (1 + EPS) - 1 (v_exp_f32 as in fwd_ref).

    dS.  dp from 64 exact products: eP = acc(64) sum_d |dout| |v|.  t = dp - Delta cancels, so
    its error is absolute: |t_k - t| <= (eP + eD) + EPS |t_k|; ds32 = fl(p t_k):
        |ds32 - dS| <= P ((1 + rp) (1 + EPS)**2 (|t| + eP + eD) - |t|) =: e32
    and the bf16 rounding in pack_frag: eS_b = e32 + UB (|dS| + e32).

    dq, dk.  sum over NPAD keys (queries) of exact products ds_b k, fp32-accumulated, times scale,
    stored in bf16:
        e = scale (1 + EPS) ((1 + acc(NPAD)) sum_j eS_b |k_jd| + acc(NPAD) sum_j |dS| |k_jd|)
        limit = e + half_ulp_bf16(|dq| + e)
    dv.  P rounded to bf16: eP_b = P ((1 + rp) (1 + UB) - 1); the same accumulation of
    P_b dout, no scale.
    Padding keys and queries contribute exact zeros (zero K, V, Q, dO rows; after the dQ-pass
    mask their dS is zero too).
    """
    scale = f32(scale)
    c0 = scale * LOG2E
    q, k, v = (t.double() for t in heads(qkv, B, H, N))
    do, og = rows(dout, B, H, N).double(), rows(o_given, B, H, N).double()
    lse = lse_given.reshape(B, H, -1)[:, :, :N].double().unsqueeze(-1)
    NP = npad(N)
    S = q @ k.transpose(-1, -2)
    A = q.abs() @ k.abs().transpose(-1, -2)
    P = torch.exp(S * scale - lse)
    delta = (do * og).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    t = dP - delta
    dS = P * t
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), P.transpose(-1, -2) @ do

    eD = ((1 + EPS) ** 11 - 1) * (do * og).abs().sum(-1, keepdim=True)
    eS = acc(64) * A
    eP = acc(64) * (do.abs() @ v.abs().transpose(-1, -2))
    c_hi = c0 * (1 + EPS)
    a_abs = (S * scale - lse).abs() * LOG2E
    ea = c_hi * eS + EPS * c0 * S.abs() + EPS * lse.abs() * LOG2E
    ea = (ea + EPS * a_abs) / (1 - EPS)
    rp = _exp_rel(ea)
    e32 = P * ((1 + rp) * (1 + EPS) ** 2 * (t.abs() + eP + eD) - t.abs()) + TINY
    eSb = e32 + UB * (dS.abs() + e32)
    ePb = P * ((1 + rp) * (1 + UB) - 1) + TINY
    g = acc(NP)

    def out(ref, err_mat, mag_mat, other, s):
        e = s * ((1 + g) * (err_mat @ other.abs()) + g * (mag_mat @ other.abs()))
        if s != 1.0:
            e = e * (1 + EPS)
        return ref, e + half_ulp(ref.abs() + e, BF16)

    res = {"dq": out(dq, eSb, dS.abs(), k, scale),
           "dk": out(dk, eSb.transpose(-1, -2), dS.abs().transpose(-1, -2), q, scale),
           "dv": out(dv, ePb.transpose(-1, -2), P.transpose(-1, -2), do, 1.0)}
    finite = all(bool(x.isfinite().all()) for x in (q, k, v, do, og, lse))
    if not finite:
        res = {n: (r, torch.full_like(b, float("nan"))) for n, (r, b) in res.items()}
    return res


# ------------------------------------------------------------------ comparison
def worst(got, ref_limit):
    """(largest error / limit, number of elements outside the limit): bn_ref.worst.  An element
    is inside only if err <= limit holds, so a NaN or inf in the output, the reference or the
    limit (a NaN given causes the last two) counts as outside with ratio inf."""
    ref, limit = ref_limit
    err = (got.double() - ref).abs()
    bad = ~(err <= limit)
    ratio = torch.where(err > 0, err / limit.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(bad & ~(ratio > 1), torch.full_like(ratio, float("inf")), ratio)
    return ratio.max().item(), int(bad.sum())


def check(got, ref_limit, what):
    """Assert |got - ref| <= limit at every element; returns the worst error / limit."""
    assert got.shape == ref_limit[0].shape, (what, got.shape, ref_limit[0].shape)
    ratio, n_bad = worst(got, ref_limit)
    assert n_bad == 0, (f"{what}: {n_bad} of {got.numel()} outside the limit, "
                        f"worst err/limit {ratio:.3g}")
    return ratio


class Worst:
    """Largest err / limit per (kernel, output) over a module's cases."""

    def __init__(self):
        self.worst = {}

    def add(self, key, ratio):
        if ratio > self.worst.get(key, -1.0):
            self.worst[key] = ratio
        return ratio

    def report(self, title):
        lines = [f"  {k:<28s} {v:.3f}" for k, v in sorted(self.worst.items())]
        return "\n".join([f"worst |err| / limit ({title}):"] + lines)


# ------------------------------------------------------------------ fp32 emulation
FWD_MUTATIONS = ("leak_pad_key", "drop_last_key")
BWD_MUTATIONS = ("drop_last_query", "drop_last_key_dq", "delta_56")


def _fma32(a, b, c):
    """fmaf on fp32 tensors (bn_ref._fma32): exact product in fp64, one rounding there and one
    to fp32.  An infinite c stays infinite."""
    return (a.double() * b.double() + c.double()).float()


def _pad(t, n):
    """[..., N, 64] -> [..., n, 64], zero rows appended (stage_rows: rows >= N are zero)."""
    z = torch.zeros(*t.shape[:-2], n - t.shape[-2], t.shape[-1], dtype=t.dtype, device=t.device)
    return torch.cat([t, z], -2)


def emulate_fwd(qkv, scale, B, H, N, mutation=None):
    """k_attn_fwd<KT> (bf16) in fp32 torch operations: K, V zero-padded to NPAD, the key mask
    at >= N, b = -mx c, a = s c + b, exp2, the fp32 row sum of the unrounded p, P rounded to
    bf16 before P V, o = acc (1 / l) stored in bf16, lse = mx scale + log(l).  An emulation for
    the CPU test of the limits (summation orders are torch's, not the MFMA's).

    mutation: "leak_pad_key" masks keys > N instead of >= N; "drop_last_key" masks key N - 1 too.
    Returns (o bf16 [B*N][H*64], lse fp32 [B*H][NPAD], columns >= N NaN)."""
    assert mutation is None or mutation in FWD_MUTATIONS
    NP = npad(N)
    q, k, v = (t.float() for t in heads(qkv, B, H, N))
    k, v = _pad(k, NP), _pad(v, NP)
    sc = torch.tensor(f32(scale), dtype=F32)
    c = sc * torch.tensor(LOG2E_F, dtype=F32)
    s = q @ k.transpose(-1, -2)
    first_masked = {None: N, "leak_pad_key": N + 1, "drop_last_key": N - 1}[mutation]
    s[..., first_masked:] = float("-inf")
    mx = s.max(-1, keepdim=True).values
    a = s * c + (-mx * c)
    p = torch.exp2(a)
    l = p.sum(-1, keepdim=True)
    o = (p.to(BF16).float() @ v) * (1.0 / l)
    lse = torch.full((B * H, NP), float("nan"), dtype=F32)
    lse[:, :N] = (mx * sc + torch.log(l)).reshape(B * H, N)
    return unrows(o).to(BF16), lse


def emulate_bwd(qkv, o, lse, dout, scale, B, H, N, mutation=None, mask_pad_keys=False):
    """k_attn_bwd_fused<KT> in fp32 torch operations: Delta as an fp32 sum, Ls = lse LOG2E with
    +inf for padding queries, p = exp2(fmaf(s, c, -Ls)), ds = p (dp - Delta) rounded to bf16,
    the second products on the rounded values, scale, bf16 stores.

    The dQ pass as the source stood before the padding mask: key tiles t with 16 t < N are
    computed whole, so the padding keys N .. 16 ceil(N / 16) - 1 carry p = exp2(-Ls) (their K row
    is 0) and ds = p (0 - Delta), multiplied by their zero K rows.  mask_pad_keys=True zeroes
    that ds instead (the kernel after the fix).

    mutation: "drop_last_query" (dK/dV pass: Ls[N - 1] = +inf), "drop_last_key_dq" (the dQ pass
    skips key N - 1), "delta_56" (Delta over 56 of the 64 features: a missing shuffle step).
    Returns dqkv bf16 [B*N][3*H*64]."""
    assert mutation is None or mutation in BWD_MUTATIONS
    q, k, v = (t.float() for t in heads(qkv, B, H, N))
    do, og = rows(dout, B, H, N).float(), rows(o, B, H, N).float()
    sc = torch.tensor(f32(scale), dtype=F32)
    c = sc * torch.tensor(LOG2E_F, dtype=F32)
    prod = do * og
    if mutation == "delta_56":
        prod = prod[..., :56]
    delta = prod.sum(-1, keepdim=True)
    Ls = (lse.reshape(B, H, -1)[:, :, :N] * torch.tensor(LOG2E_F, dtype=F32)).unsqueeze(-1)

    # dQ pass: keys of every computed tile
    NK = (N + 15) // 16 * 16
    kp, vp = _pad(k, NK), _pad(v, NK)
    p = torch.exp2(_fma32(q @ kp.transpose(-1, -2), c, -Ls))
    ds = p * (do @ vp.transpose(-1, -2) - delta)
    if mask_pad_keys:
        ds[..., N:] = 0
    if mutation == "drop_last_key_dq":
        ds[..., N - 1] = 0
    dq = (ds.to(BF16).float() @ kp) * sc

    # dK/dV pass: real keys, real queries (a padding query has Ls = +inf: p = 0, ds = 0)
    Lk = Ls.clone()
    if mutation == "drop_last_query":
        Lk[..., N - 1, :] = float("inf")
    p = torch.exp2(_fma32(q @ k.transpose(-1, -2), c, -Lk))
    ds = p * (do @ v.transpose(-1, -2) - delta)
    dv = p.to(BF16).float().transpose(-1, -2) @ do
    dk = (ds.to(BF16).float().transpose(-1, -2) @ q) * sc
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * DH).to(BF16)
