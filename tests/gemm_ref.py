"""Shared helper of the dfu_gemm conformance tests (test_gemm_matrix_gpu.py,
test_conv_geometry_gpu.py, test_gemm_kernel_list_cpu.py): guarded buffers, two data regimes with
an fp64 reference, the derived error bound, the case builders (one per operand-mode pair) and the
runner that launches a case with its tile forced.

Guarded buffers.  Every operand and output is a view into a larger flat allocation with guard
elements before and after it and a leading dimension larger than the row.  Outputs: guards and
ld padding hold a sentinel bit pattern (a NaN), compared as integers after the launch.  Operands:
guards, ld padding and the columns MN..ld-1 of an MN-major operand hold NaN, so a loader that
masks one operand only (0 * garbage) shows.

Integer regime.  Operands, bias, aux and the initial C are small integers (operands in [-3, 3],
alpha in {1, 0.5}): every product and partial sum is exact in fp32 in any order for K <= 1024
(|sum| <= 9 * 1024 < 2^24), so the result must equal the fp64 reference rounded once to the
output type -- whatever the tile, split, schedule or atomics order.

Gaussian regime.  Operands are bf16-exact (fp16-exact) normals, the reference is fp64, and the
bound is gemm_bound() below.
"""
import ctypes
import json
import math
import os
import zlib

import torch

from dfu_hip import _lib as L
from dfu_hip.ops import TILE_DIMS  # dfu_gemm_desc.tile -> (TM, TN, phased)

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS_JSON = os.path.join(HERE, "golden", "gemm_kernels.json")

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
EPS = 2.0 ** -23  # bound on the relative error of one fp32 operation, any rounding mode

GELU_EPIS = (L.EPI_BF16_GELU, L.EPI_X3_GELU, L.EPI_F16_GELU)
BIAS_EPIS = (L.EPI_BF16, L.EPI_BF16_RELU, L.EPI_BF16_GELU, L.EPI_F32, L.EPI_F32_RESID,
             L.EPI_PATCH, L.EPI_X3_GELU, L.EPI_F16_DUAL, L.EPI_F16_GELU)
F32_OUT = (L.EPI_F32, L.EPI_F32_RESID, L.EPI_F32_ACC, L.EPI_PATCH, L.EPI_F32_STATS)
AUX_DTYPE = {L.EPI_F32_RESID: F32, L.EPI_PATCH: F32, L.EPI_BF16_DGELU: BF16, L.EPI_BF16_ADD: BF16}
EPI_NAME = {v: k[4:] for k, v in vars(L).items() if k.startswith("EPI_")}
MODE_NAME = {v: k[5:] for k, v in vars(L).items() if k.startswith("OPND_")}


def kernels():
    """The committed kernel list: (tile, a_mode, b_mode, epilogue, key) tuples."""
    with open(KERNELS_JSON) as f:
        return [tuple(k) for k in json.load(f)["kernels"]]


def kernel_id(k):
    return f"t{k[0]}-{MODE_NAME[k[1]]}x{MODE_NAME[k[2]]}-{EPI_NAME[k[3]]}-{k[4]}"


def round8(x):
    return (x + 7) & ~7


# ------------------------------------------------------------------------- guarded buffers
SENTINEL = {2: 0x7FD5, 4: 0x7FC0D5D5, 1: 0xA5}  # bf16 / fp16 / fp32 NaNs with a marked payload
INT_OF = {2: torch.int16, 4: torch.int32, 1: torch.uint8}
GUARD = 64  # elements before and after (64 x 2 B = 128 B: the view keeps 16-B alignment)


class Guarded:
    """A [rows][cols] view of row stride ld, `offset` elements into a flat allocation filled
    with the sentinel (outputs) or NaN (operands)."""

    def __init__(self, rows, cols, ld, dtype, device, offset=0, keep_rows=None):
        assert ld >= cols
        self.rows, self.cols, self.ld = rows, cols, ld
        self.size = torch.empty(0, dtype=dtype).element_size()
        n = GUARD + offset + rows * ld + GUARD
        self.bits = torch.full((n,), self._sentinel(), dtype=INT_OF[self.size], device=device)
        self.flat = self.bits.view(dtype)
        self.view = self.flat[GUARD + offset:GUARD + offset + rows * ld].view(rows, ld)[:, :cols]
        inside = torch.zeros(n, dtype=torch.bool, device=device)
        iv = inside[GUARD + offset:GUARD + offset + rows * ld].view(rows, ld)[:, :cols]
        if keep_rows is None:
            iv[:] = True
        else:  # rows the kernel may write (PATCH: every row but the class tokens)
            iv[keep_rows] = True
        self.outside = ~inside

    def _sentinel(self):
        s = SENTINEL[self.size]
        return s - (1 << (8 * self.size)) if self.size > 1 and s >= 1 << (8 * self.size - 1) else s

    def set(self, x):
        self.view.copy_(x.to(self.view.dtype))
        return self

    def ptr(self):
        return self.view.data_ptr()

    def untouched(self):
        """Everything outside the view still holds the sentinel bit pattern."""
        return bool((self.bits[self.outside] == self._sentinel()).all())


def operand(x64, dtype, ld):
    """x64 [rows][cols] as a NaN-guarded operand of row stride ld."""
    g = Guarded(x64.shape[0], x64.shape[1], ld, dtype, x64.device)
    return g.set(x64)


# ------------------------------------------------------------------------- data and bounds
def draw(gen, shape, regime, dtype, device, lo=-3, hi=3):
    """fp64 values exactly representable in `dtype`: integers in [lo, hi] or unit normals."""
    if regime == "int":
        return torch.randint(lo, hi + 1, shape, generator=gen, device=device).to(F64)
    return torch.randn(shape, generator=gen, device=device, dtype=F32).to(dtype).to(F64)


def half_ulp(x, dtype):
    """Half a unit in the last place of `dtype` at |x| (fp64 tensor)."""
    p, emin = {BF16: (8, -126), F16: (11, -14), F32: (24, -126), F64: (53, -1022)}[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - p)


def gemm_bound(absprod, addends, K, splits=1, x3=False):
    """|fp32 result - exact| of alpha * sum_k a b + addends, before the output rounding.

    Each of the K products is exact in fp32 (bf16 x bf16 and fp16 x fp16 have <= 22 significant
    bits); the K - 1 additions of the accumulation, the S - 1 additions of the split partials, the
    alpha multiply and up to three epilogue additions (bias, aux, C) are one fp32 operation each,
    of relative error < 2^-23 = EPS on a partial result bounded by |A|.|B| + |addends| (absprod
    includes |alpha|).  First order that is (K + S + 3) EPS (|A|.|B| + |addends|); the factor 2
    and the + 4 cover the second-order terms (1 + EPS)^(K + S + 3) - 1 <= 2 (K + S + 3) EPS for
    every K used here and MFMA-internal summation orders.
        |err| <= 2 (K + S + 4) EPS (|A|.|B| + |addends|)
    Interleaved-pair bf16x3 kernels (against the product of the unsplit fp32 operands): a =
    hi + lo + ra with |lo| <= 2^-9 |a|, |ra| <= 2^-18 |a| (same for b); the kernel forms hi hi +
    lo hi + hi lo, dropping lo lo + ra b + a rb <= 3 2^-18 |a| |b|.
    """
    b = 2.0 * (K + splits + 4) * EPS * (absprod + addends)
    if x3:
        b = b + 3.0 * 2.0 ** -18 * absprod
    return b


def gelu_ref(u):
    cdf = 0.5 * torch.erfc(-u / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return u * cdf, cdf + u * pdf


def gelu_bounds(u, du):
    """Error of the kernel's GELU g = u Phi(u) and g' = Phi(u) + u phi(u) at a pre-activation of
    error du.  common.h: |Phi error| <= 3e-7, so |g error| <= 3e-7 |u| and |g' error| <= 3e-7
    (u phi(u) from the same exponential: its error is below Phi's); the input error propagates
    through |g'| <= 1.13 and |g''| = |phi(u) (2 - u^2)| <= 0.8; each value is then formed by two
    fp32 operations (4 EPS of its magnitude, second order included)."""
    g, d = gelu_ref(u)
    return (1.13 * du + 3e-7 * u.abs() + 4 * EPS * g.abs(),
            0.8 * du + 3e-7 + 4 * EPS * d.abs())


class Ratios:
    """Largest err / bound per epilogue family over a module's Gaussian-regime cases."""

    def __init__(self):
        self.worst = {}

    def add(self, family, err, bound):
        r = float((err / bound.clamp_min(1e-300)).max())
        if r > self.worst.get(family, (0.0,))[0]:
            self.worst[family] = (r,)
        return r

    def report(self, title):
        rows = [f"  {k:<22s} {v[0]:.3f}" for k, v in sorted(self.worst.items())]
        return "\n".join([f"worst |err| / bound, Gaussian regime ({title}):"] + rows)


RATIOS = Ratios()


# ------------------------------------------------------------------------------- cases
class Case:
    """One launch: a kernel identity, a shape and how its buffers are laid out."""

    def __init__(self, kernel, M, N, K, regime="int", bias=False, alpha=1.0, inplace=False,
                 ldpad=8, ldaux_pad=None, split_k=0, seg=0, geom=None, pair_out=False,
                 atomics=False, inkernel=False, expect_ws=False, dstats=False, c_nonzero=None,
                 no_aux_out=False, offsets=(0, 0, 0), note=""):
        self.kernel, self.M, self.N, self.K = kernel, M, N, K
        self.regime, self.bias, self.alpha, self.inplace = regime, bias, alpha, inplace
        self.ldpad, self.ldaux_pad = ldpad, ldpad if ldaux_pad is None else ldaux_pad
        self.split_k, self.seg, self.geom, self.pair_out = split_k, seg, geom, pair_out
        self.atomics, self.inkernel, self.expect_ws, self.dstats = atomics, inkernel, expect_ws, dstats
        self.c_nonzero = kernel[3] == L.EPI_F32_ACC if c_nonzero is None else c_nonzero
        self.no_aux_out, self.note = no_aux_out, note
        self.offsets = offsets  # elements from a 16-B aligned base: C, aux, aux_out

    @property
    def tile(self):
        return self.kernel[0]

    def __repr__(self):
        g = "" if self.geom is None else f" conv={self.geom}"
        return (f"{kernel_id(self.kernel)} M={self.M} N={self.N} K={self.K} {self.regime}"
                f" bias={int(self.bias)} alpha={self.alpha} inplace={int(self.inplace)}"
                f" ldpad={self.ldpad}/{self.ldaux_pad} split_k={self.split_k} seg={self.seg}"
                f" pair={int(self.pair_out)} atomics={int(self.atomics)}"
                f" inkernel={int(self.inkernel)} offsets={self.offsets}{g} {self.note}")


def _has_aux(e):
    return e in AUX_DTYPE


def _has_aux_out(k):
    return k[3] in GELU_EPIS or k[3] == L.EPI_F16_DUAL


def linear_cases(k, gaussian=True):
    """The matrix of a linear kernel (K-contiguous or MN-major A and B): see the issue text in
    test_gemm_matrix_gpu.py's docstring for the shape rules."""
    tile, a_mode, b_mode, epi, key = k
    TM, TN, _ = TILE_DIMS[tile]
    integer = epi not in GELU_EPIS
    regimes = (["int"] if integer else []) + (["gauss"] if gaussian else [])
    if key == "x3":
        Ks = [64, 192]  # a_seg 32, 96
    elif a_mode == L.OPND_MNMAJOR and b_mode == L.OPND_MNMAJOR:
        Ks = [5, 64, 150]
    else:
        Ks = [8, 64, 136, 200]
    if epi == L.EPI_PATCH:
        Ms = [59 * (TM // 59 + 1)]  # ep_tokens = 59, the smallest batch with M > TM
    else:
        Ms = [24, TM + 37]
    out = []
    n = 0
    for regime in regimes:
        # the Gaussian regime walks a diagonal of the shape grid (every M, N class and K once),
        # the integer regime the whole grid
        for mi, M in enumerate(Ms):
            for ni, N in enumerate((TN + 8, TN + 12, TN + 13)):
                for ki, K in enumerate(Ks):
                    if regime == "gauss" and (mi + ni + ki) % 2:
                        continue
                    n += 1
                    alpha = 1.0 if (not integer or epi in GELU_EPIS or n % 2) else 0.5
                    out.append(Case(k, M, N, K, regime, bias=epi in BIAS_EPIS and n % 3 != 0,
                                    alpha=alpha, seg=K // 2 if key == "x3" else 0,
                                    pair_out=epi == L.EPI_F32_STATS and n % 2 == 0))
        M, K = Ms[-1], Ks[-1]
        seg = K // 2 if key == "x3" else 0
        bias = epi in BIAS_EPIS
        if _has_aux(epi) or _has_aux_out(k) or epi == L.EPI_F32_STATS:
            # ldaux (ldaux_out) in another class than ldc: still 8-B aligned rows under the
            # 16-B merged store, and odd (everything scalar)
            for pad in (12, 13):
                out.append(Case(k, M, TN + 8, K, regime, bias=bias, ldaux_pad=pad, seg=seg,
                                pair_out=epi == L.EPI_F32_STATS, note="ldaux class"))
        if epi not in F32_OUT or epi == L.EPI_F32_STATS:
            out.append(Case(k, M, 2, K, regime, bias=bias, seg=seg,
                            pair_out=epi == L.EPI_F32_STATS, note="N=2"))
        if epi in (L.EPI_BF16_ADD, L.EPI_F32_RESID):
            for N in (TN + 8, TN + 13):
                out.append(Case(k, M, N, K, regime, bias=bias, inplace=True, seg=seg))
        if epi == L.EPI_BF16_DGELU and tile == 8 and regime == "int":
            out.append(Case(k, M, TN + 8, K, regime, dstats=True, note="column sums"))
    if epi == L.EPI_F32_ACC:
        out += splitk_cases(k)
    if epi == L.EPI_F16_DUAL:
        out.append(Case(k, Ms[-1], TN + 8, Ks[-1], "int", bias=True, no_aux_out=True))
    if epi != L.EPI_F32_ACC and tile in (1, 5):
        # tail split: 4 tiles (a last, partial round) x 16 K-steps (PATCH: M = 3 x 59)
        for regime in regimes:
            out.append(Case(k, 177 if epi == L.EPI_PATCH else 165, 136, 1024, regime,
                            bias=epi in BIAS_EPIS, expect_ws=True,
                            seg=512 if key == "x3" else 0, note="tail split"))
    return out


def splitk_cases(k):
    """F32_ACC split-K: the last split short (K = 1000) or absent (K = 150: 3 K-steps), the three
    reduce kernels (vector; scalar at N = 147; wide at >= 8 splits of a small plane), the
    in-kernel reduction and fp32 atomics on the generic tiles."""
    tile = k[0]
    TM, TN, phased = TILE_DIMS[tile]
    out = []
    for K in (150, 1000):
        for s in (2, 3, 7):
            out.append(Case(k, TM + 37, TN + 12, K, "int", split_k=s, note="reduce: vector"))
    out.append(Case(k, 40, 147, 1000, "int", split_k=3, note="reduce: scalar"))
    out.append(Case(k, 64, 64, 1000, "int", split_k=8, note="reduce: wide vector"))
    out.append(Case(k, 64, 147, 1000, "int", split_k=8, note="reduce: wide scalar"))
    out.append(Case(k, TM + 37, TN + 12, 1000, "gauss", split_k=7))
    if not phased:
        for s in (2, 7):
            out.append(Case(k, TM + 37, TN + 12, 1000, "int", split_k=s, inkernel=True))
        out.append(Case(k, TM + 37, TN + 13, 150, "int", split_k=3, inkernel=True))
        for s in (2, 5):
            out.append(Case(k, TM + 37, TN + 13, 1000, "int", split_k=s, atomics=True))
    return out


# kernels of the output-alignment cases: 16-bit C with aux_out, with a 16-bit and an fp32 aux, on
# a generic, the phased and both persistent tiles, fp16 operands and the split-pair output
ALIGN_KERNELS = [(1, 0, 0, L.EPI_BF16_GELU, "bf16"), (7, 0, 0, L.EPI_BF16_GELU, "bf16"),
                 (8, 0, 0, L.EPI_BF16_GELU, "bf16"), (1, 0, 1, L.EPI_BF16_ADD, "bf16"),
                 (8, 0, 1, L.EPI_BF16_ADD, "bf16"), (1, 0, 0, L.EPI_F32_RESID, "bf16"),
                 (9, 0, 0, L.EPI_F32_RESID, "bf16"), (8, 0, 0, L.EPI_F16_DUAL, "f16"),
                 (1, 0, 0, L.EPI_F32_STATS, "bf16")]


def alignment_cases(k):
    """C, aux and aux_out as column slices of a wider row: 8, 4, 2 and 1 elements from a 16-byte
    aligned base, one pointer at a time and all together, on a shape of the merged-store class
    (N, ld % 8 == 0).  8 keeps every class, 4 elements of 16 bits (8 B) leave the 4-column vectors,
    anything else is served by the scalar class (include/dfu_hip.h)."""
    TM, TN, _ = TILE_DIMS[k[0]]
    regime = "gauss" if k[3] in GELU_EPIS else "int"
    offs = [(o if i == j else 0 for j in range(3)) for i in range(3) for o in (8, 4, 2, 1)]
    offs = [tuple(o) for o in offs] + [(8, 8, 8), (4, 4, 4), (2, 2, 2), (1, 1, 1)]
    return [Case(k, TM + 37, TN + 8, 136, regime, bias=k[3] in BIAS_EPIS, offsets=o,
                 pair_out=k[3] == L.EPI_F32_STATS, note="alignment") for o in offs]


class Geom:
    """Conv geometry: NHWC input n, h, w, c; k filters r x s; stride; pad."""

    def __init__(self, h, w, r, s, stride, pad, c=64, k=128, n=2):
        self.n, self.h, self.w, self.c, self.k = n, h, w, c, k
        self.r, self.s, self.stride, self.pad = r, s, stride, pad
        self.p = (h + 2 * pad - r) // stride + 1
        self.q = (w + 2 * pad - s) // stride + 1

    def __repr__(self):
        return (f"{self.n}x{self.h}x{self.w}x{self.c}->{self.k} {self.r}x{self.s}/"
                f"{self.stride}/{self.pad}")


# H x W, R x S / stride / pad of test_conv_geometry_gpu.py (never square in both)
GEOMS = [(9, 13, 3, 3, 1, 1), (9, 14, 3, 3, 2, 1), (7, 10, 3, 3, 1, 0), (9, 14, 1, 1, 2, 0),
         (10, 7, 5, 5, 2, 2), (8, 11, 3, 3, 3, 1), (6, 9, 1, 3, 1, 0), (6, 9, 3, 1, 1, 0)]


def conv_direction(k):
    a, b = k[1], k[2]
    return "fwd" if a == L.OPND_CONV_FWD else "dgrad" if a == L.OPND_CONV_DGRAD else "wgrad"


def conv_case(k, g, regime="int", inplace=False, split_k=0, bias=False):
    d = conv_direction(k)
    seg = g.c // 2 if k[4] == "x3" else 0
    if d == "fwd":
        M, N, K = g.n * g.p * g.q, g.k, g.r * g.s * g.c
    elif d == "dgrad":
        M, N, K = g.n * g.h * g.w, g.c, g.r * g.s * g.k
    else:
        M, N, K = g.k, g.r * g.s * g.c, g.n * g.p * g.q
    return Case(k, M, N, K, regime, inplace=inplace, split_k=split_k, geom=g, seg=seg, bias=bias,
                pair_out=k[3] == L.EPI_F32_STATS and regime == "gauss")


def conv_cases(k, gaussian=True):
    """The matrix's cases of an implicit-conv kernel: two of the geometries (stride 1 and 2), the
    whole list is test_conv_geometry_gpu.py's."""
    out = []
    d = conv_direction(k)
    for gi in (0, 1):
        g = Geom(*GEOMS[gi], c=128 if k[4] == "x3" and gi else 64)
        for regime in ["int"] + (["gauss"] if gaussian else []):
            out.append(conv_case(k, g, regime, bias=d == "fwd" and k[3] == L.EPI_BF16))
            if k[3] == L.EPI_BF16_ADD:
                out.append(conv_case(k, g, regime, inplace=True))
            if d == "wgrad":
                out.append(conv_case(k, g, regime, split_k=3))
    return out


# one case builder per (a_mode, b_mode) pair that has kernels
BUILDERS = {
    (L.OPND_KMAJOR, L.OPND_KMAJOR): linear_cases,
    (L.OPND_KMAJOR, L.OPND_MNMAJOR): linear_cases,
    (L.OPND_MNMAJOR, L.OPND_MNMAJOR): linear_cases,
    (L.OPND_CONV_FWD, L.OPND_KMAJOR): conv_cases,
    (L.OPND_CONV_DGRAD, L.OPND_CONV_DGRAD_W): conv_cases,
    (L.OPND_MNMAJOR, L.OPND_CONV_WGRAD_X): conv_cases,
}


def cases_for(k):
    """The matrix's cases of a kernel of the list; never empty, never another tile's (there is
    no fallback: a kernel without a builder is an error)."""
    fn = BUILDERS.get((k[1], k[2]))
    if fn is None:
        raise LookupError(f"no case builder for {kernel_id(k)}")
    cases = fn(k)
    if not cases or any(c.kernel != k for c in cases):
        raise LookupError(f"case builder of {kernel_id(k)} returned no case of that kernel")
    return cases


# ------------------------------------------------------------------------------- runner
def planned(lib, d):
    t, sk = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.dfu_gemm_plan(ctypes.byref(d), ctypes.byref(t), ctypes.byref(sk))
    return rc, t.value, sk.value


def _seed(c):
    return zlib.crc32(repr(c).encode())  # the same data in every process


def _im2col(x, g):
    """x fp64 NHWC -> [n p q][r s c] (zero padding)."""
    xp = torch.zeros(g.n, g.h + 2 * g.pad, g.w + 2 * g.pad, g.c, dtype=F64, device=x.device)
    xp[:, g.pad:g.pad + g.h, g.pad:g.pad + g.w] = x
    col = torch.empty(g.n, g.p, g.q, g.r, g.s, g.c, dtype=F64, device=x.device)
    for r in range(g.r):
        for s in range(g.s):
            col[:, :, :, r, s] = xp[:, r:r + g.stride * (g.p - 1) + 1:g.stride,
                                    s:s + g.stride * (g.q - 1) + 1:g.stride]
    return col.view(g.n * g.p * g.q, g.r * g.s * g.c)


def _col2im(dcol, g):
    """The adjoint of _im2col: [n p q][r s c] -> fp64 NHWC."""
    dcol = dcol.view(g.n, g.p, g.q, g.r, g.s, g.c)
    xp = torch.zeros(g.n, g.h + 2 * g.pad, g.w + 2 * g.pad, g.c, dtype=F64, device=dcol.device)
    for r in range(g.r):
        for s in range(g.s):
            xp[:, r:r + g.stride * (g.p - 1) + 1:g.stride,
               s:s + g.stride * (g.q - 1) + 1:g.stride] += dcol[:, :, :, r, s]
    return xp[:, g.pad:g.pad + g.h, g.pad:g.pad + g.w].reshape(g.n * g.h * g.w, g.c)


def _pairs(hi, lo):
    """[rows][seg] hi and lo -> the interleaved-pair B operand [rows][2 seg]: per 32 columns
    [hi 32 | lo 32] (dfu_split_x3 pattern 2)."""
    rows, seg = hi.shape
    return torch.stack((hi.view(rows, seg // 32, 32), lo.view(rows, seg // 32, 32)),
                       dim=2).reshape(rows, 2 * seg)


def _split(x64):
    """fp64 -> (hi, lo) bf16-exact fp64: hi = bf16(x), lo = bf16(x - hi), x taken as fp32."""
    x = x64.to(F32)
    hi = x.to(BF16)
    lo = (x - hi.to(F32)).to(BF16)
    return hi.to(F64), lo.to(F64)


def _x3_operand(gen, shape, regime, dev):
    """(value the product is compared against, hi, lo) of a split operand: independent integer
    hi and lo (the kernel's hi hi + lo hi + hi lo is then exact and checked term by term), or a
    unit normal fp32 split into its pair."""
    if regime == "int":
        hi, lo = draw(gen, shape, "int", BF16, dev), draw(gen, shape, "int", BF16, dev)
        return None, hi, lo
    x = torch.randn(shape, generator=gen, device=dev, dtype=F32).to(F64)
    hi, lo = _split(x)
    return x, hi, lo


def _x3_product(a, b, regime):
    """(product, |A|.|B|) of split operands a = (x, hi, lo), b likewise, both [rows][K]."""
    (ax, ah, al), (bx, bh, bl) = a, b
    if regime == "int":
        prod = ah @ bh.T + al @ bh.T + ah @ bl.T
        absprod = ah.abs() @ bh.abs().T + al.abs() @ bh.abs().T + ah.abs() @ bl.abs().T
        return prod, absprod
    return ax @ bx.T, ax.abs() @ bx.abs().T


def run_case(c, dev="cuda"):
    """Launch the case with its tile forced and check everything; raises AssertionError naming
    the case."""
    try:
        _run(c, torch.device(dev))
    except AssertionError as e:
        raise AssertionError(f"{c!r}: {e}") from None


def _check(cond, msg):
    if not cond:
        raise AssertionError(msg)


def _run(c, dev):
    from dfu_hip import streams
    lib = L.load()
    tile, a_mode, b_mode, epi, key = c.kernel
    M, N, K, g = c.M, c.N, c.K, c.geom
    odt = F16 if key == "f16" else BF16
    gen = torch.Generator(device=dev)
    gen.manual_seed(_seed(c))
    x3 = key == "x3"
    keep = []  # buffers kept alive until the final synchronisation
    d = L.GemmDesc()
    d.M, d.N, d.K, d.a_mode, d.b_mode, d.epilogue, d.tile = M, N, K, a_mode, b_mode, epi, tile
    d.alpha = c.alpha
    d.operand_type = L.OPERAND_F16 if key == "f16" else L.OPERAND_BF16
    if g is not None:
        d.conv_n, d.conv_h, d.conv_w, d.conv_c, d.conv_k = g.n, g.h, g.w, g.c, g.k
        d.conv_r, d.conv_s, d.conv_stride, d.conv_pad = g.r, g.s, g.stride, g.pad
        d.conv_p, d.conv_q = g.p, g.q
        if x3:
            d.conv_c = 2 * c.seg

    # ---- operands and the exact product ------------------------------------------------
    def kmajor(x64, pad=8):
        b = operand(x64, odt, x64.shape[1] + pad)
        keep.append(b)
        return b

    def mnmajor(x64):  # x64 [MN][K] stored [K][ld], columns MN..ld-1 NaN
        b = operand(x64.T.contiguous(), odt, round8(x64.shape[0]) + 8)
        keep.append(b)
        return b

    if g is None:
        if x3:
            a3 = _x3_operand(gen, (M, c.seg), c.regime, dev)
            b3 = _x3_operand(gen, (N, c.seg), c.regime, dev)
            prod, absprod = _x3_product(a3, b3, c.regime)
            ah, al = kmajor(a3[1], 0), kmajor(a3[2], 0)
            bb = kmajor(_pairs(b3[1], b3[2]))
            d.A, d.lda, d.a_lo, d.a_seg, d.x3_pairs = ah.ptr(), c.seg, al.ptr(), c.seg, 1
            d.B, d.ldb = bb.ptr(), bb.ld
        else:
            A = draw(gen, (M, K), c.regime, odt, dev)
            B = draw(gen, (N, K), c.regime, odt, dev)
            prod, absprod = A @ B.T, A.abs() @ B.abs().T
            ab = kmajor(A) if a_mode == L.OPND_KMAJOR else mnmajor(A)
            bb = kmajor(B) if b_mode == L.OPND_KMAJOR else mnmajor(B)
            d.A, d.lda, d.B, d.ldb = ab.ptr(), ab.ld, bb.ptr(), bb.ld
    else:
        direction = conv_direction(c.kernel)
        cin = c.seg if x3 else g.c
        gg = Geom(g.h, g.w, g.r, g.s, g.stride, g.pad, c=cin, k=g.k, n=g.n)
        if direction == "fwd":
            if x3:
                x3o = _x3_operand(gen, (g.n * g.h * g.w, cin), c.regime, dev)
                w3o = _x3_operand(gen, (g.k, g.r * g.s * cin), c.regime, dev)
                cols = tuple(None if t is None else _im2col(t.view(g.n, g.h, g.w, cin), gg)
                             for t in x3o)
                prod, absprod = _x3_product(cols, w3o, c.regime)
                xh, xl = kmajor(x3o[1], 0), kmajor(x3o[2], 0)
                wp = _pairs(w3o[1].reshape(-1, cin), w3o[2].reshape(-1, cin)).view(g.k, -1)
                wb = kmajor(wp)
                d.A, d.a_lo, d.a_seg, d.x3_pairs = xh.ptr(), xl.ptr(), c.seg, 1
            else:
                x = draw(gen, (g.n * g.h * g.w, cin), c.regime, odt, dev)
                w = draw(gen, (g.k, g.r * g.s * cin), c.regime, odt, dev)
                col = _im2col(x.view(g.n, g.h, g.w, cin), gg)
                prod, absprod = col @ w.T, col.abs() @ w.abs().T
                xb, wb = kmajor(x, 0), kmajor(w)  # NHWC: pixel stride = channels, NaN around it
                d.A = xb.ptr()
            d.lda, d.B, d.ldb = cin, wb.ptr(), wb.ld
        elif direction == "dgrad":
            dy = draw(gen, (g.n * g.p * g.q, g.k), c.regime, odt, dev)
            w = draw(gen, (g.k, g.r * g.s * g.c), c.regime, odt, dev)
            prod, absprod = _col2im(dy @ w, gg), _col2im(dy.abs() @ w.abs(), gg)
            yb, wb = kmajor(dy, 0), kmajor(w, 0)
            d.A, d.lda, d.B, d.ldb = yb.ptr(), g.k, wb.ptr(), g.r * g.s * g.c
        else:
            dy = draw(gen, (g.n * g.p * g.q, g.k), c.regime, odt, dev)
            x = draw(gen, (g.n * g.h * g.w, g.c), c.regime, odt, dev)
            col = _im2col(x.view(g.n, g.h, g.w, g.c), gg)
            prod, absprod = dy.T @ col, dy.T.abs() @ col.abs()
            yb, xb = mnmajor(dy.T.contiguous()), kmajor(x, 0)
            d.A, d.lda, d.B, d.ldb = yb.ptr(), yb.ld, xb.ptr(), g.c
    _check(tuple(prod.shape) == (M, N), f"reference shape {tuple(prod.shape)}")
    P = c.alpha * prod
    absP = abs(c.alpha) * absprod

    # ---- epilogue inputs ---------------------------------------------------------------
    bias64 = torch.zeros(N, dtype=F64, device=dev)
    if c.bias:
        bias64 = draw(gen, (N,), c.regime, F32, dev, -4, 4)
        bt = bias64.to(F32)
        keep.append(bt)
        d.bias = bt.data_ptr()
    ldc = N + c.ldpad
    planes = {L.EPI_X3_GELU: 3, L.EPI_F16_GELU: 2}.get(epi, 1)
    if planes > 1:
        ldc = planes * N + c.ldpad
    pair = c.pair_out and epi == L.EPI_F32_STATS
    cdt = (BF16 if pair else F32) if epi in F32_OUT else (F16 if epi in (L.EPI_F16_DUAL, L.EPI_F16_GELU) else BF16)
    c_rows, keep_rows, T = M, None, 59
    if epi == L.EPI_PATCH:
        nb = M // T
        c_rows = nb * (T + 1)
        keep_rows = torch.ones(c_rows, dtype=torch.bool, device=dev)
        keep_rows[::T + 1] = False
        d.ep_tokens = T
    cb = Guarded(c_rows, planes * N, ldc, cdt, dev, offset=c.offsets[0], keep_rows=keep_rows)
    d.C, d.ldc = cb.ptr(), ldc
    aux64 = torch.zeros(M, N, dtype=F64, device=dev)
    auxb = None
    if epi in AUX_DTYPE:
        adt = AUX_DTYPE[epi]
        rows = T + 1 if epi == L.EPI_PATCH else M
        av = draw(gen, (rows, N), c.regime, adt, dev, -4, 4)
        if epi == L.EPI_PATCH:
            aux64 = av[1:].repeat(M // T, 1)
        else:
            aux64 = av
        if c.inplace:
            cb.set(av)
            d.aux, d.ldaux = cb.ptr(), ldc
        else:
            auxb = Guarded(rows, N, N + c.ldaux_pad, adt, dev, offset=c.offsets[1])
            auxb.set(av)
            d.aux, d.ldaux = auxb.ptr(), auxb.ld
    c0 = torch.zeros(M, N, dtype=F64, device=dev)
    if epi == L.EPI_F32_ACC and c.c_nonzero:
        c0 = draw(gen, (M, N), c.regime, F32, dev, -4, 4)
        cb.set(c0)
    ob = None
    if (_has_aux_out(c.kernel) and not c.no_aux_out) or pair:
        ob = Guarded(M, N, N + c.ldaux_pad, BF16, dev, offset=c.offsets[2])
        d.aux_out, d.ldaux_out = ob.ptr(), ob.ld
    sb = None
    if epi in (L.EPI_BF16_STATS, L.EPI_F32_STATS):
        sb = Guarded((M + 127) // 128, 2 * N, 2 * N, F32, dev)
    elif c.dstats:
        sb = Guarded(2 * ((M + 255) // 256), N, N, F32, dev)
    if sb is not None:
        d.stats = sb.ptr()

    # ---- plan, workspace, launch -------------------------------------------------------
    d.split_k = c.split_k if epi == L.EPI_F32_ACC else 0
    rc, ptile, psplit = planned(lib, d)
    _check(rc == 0 and ptile == tile, f"dfu_gemm_plan rc={rc} tile={ptile}: not the forced tile")
    need = lib.dfu_gemm_workspace_bytes(ctypes.byref(d))
    if c.expect_ws:
        _check(need > 0, "the case no longer reaches the tail split (workspace bytes 0)")
    if epi == L.EPI_F32_ACC and c.split_k > 1:
        kt = -(-K // 64)
        se = -(-kt // -(-kt // c.split_k))
        _check(psplit == se and need == (se * M * N * 4 if se > 1 else 0),
               f"split plan {psplit} (expected {se}), workspace {need}")
    wb_ = None
    cnt = streams.tile_counters(dev)
    if need > 0 and not c.atomics:
        slack = 256
        wb_ = torch.full((need + slack,), SENTINEL[1], dtype=torch.uint8, device=dev)
        d.workspace, d.workspace_bytes = wb_.data_ptr(), need
        d.tile_counters, d.tile_counters_len = cnt.data_ptr(), cnt.numel()
    old = lib.dfu_gemm_set_inkernel_reduce(1 if c.inkernel else 0)
    try:
        rc = lib.dfu_gemm(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    finally:
        lib.dfu_gemm_set_inkernel_reduce(old)
    _check(rc == 0, f"dfu_gemm rc={rc}: {(lib.dfu_last_error_string() or b'').decode()}")
    torch.cuda.synchronize()

    # ---- what the kernel must not have written -----------------------------------------
    _check(cb.untouched(), "C: guard, ld padding or rows past M overwritten")
    for b, name in ((ob, "aux_out"), (sb, "stats")):
        if b is not None:
            _check(b.untouched(), f"{name}: guard or padding overwritten")
    if wb_ is not None:
        _check(bool((wb_[need:] == SENTINEL[1]).all()), "workspace written past its size")
    _check(not bool(cnt.any()), "tile_counters not returned zeroed")
    if c.expect_ws:
        # the tail-split slabs hold whole accumulator tiles, the columns past N and rows past M
        # included: zeros from the loaders' masks, never the NaN around the operands (the only
        # place where an MN-major chunk fetched at column round8(MN) shows)
        _check(bool(torch.isfinite(wb_[:need].view(F32)).all()),
               "tail-split slabs hold non-finite partial sums (an operand read past its bound)")

    # ---- the values --------------------------------------------------------------------
    splits = psplit if epi == L.EPI_F32_ACC else (8 if c.expect_ws else 1)
    Keff = 3 * c.seg * (K // (2 * c.seg)) if x3 else K
    fam = EPI_NAME[epi] + ("" if key == "bf16" else "/" + key)
    got = cb.view
    if epi == L.EPI_PATCH:
        got = got[keep_rows]

    def compare(name, out, ref, out_dt, bound):
        """Integer regime: out == ref rounded once to the output type; Gaussian: |out - ref| <=
        bound + half an ulp of the output type at the reference."""
        o = out.to(F64)
        if c.regime == "int":
            want = ref.to(out_dt).to(F64)
            bad = o != want
            if bool(bad.any()):
                raise AssertionError(
                    f"{name}: {int(bad.sum())} of {bad.numel()} values differ from the "
                    f"once-rounded fp64 reference (first at {bad.nonzero()[0].tolist()}: "
                    f"{o[bad][0].item()} vs {want[bad][0].item()})")
            return
        _check(bool(torch.isfinite(o).all()), f"{name}: non-finite output")
        err = (o - ref).abs()
        lim = bound + half_ulp(ref.abs() + bound, out_dt)
        r = RATIOS.add(fam + ":" + name, err, lim)
        _check(r <= 1.0, f"{name}: |err| / bound = {r:.3f} (max err {float(err.max()):.3e})")

    add = bias64.abs()[None, :] + aux64.abs() + c0.abs()
    dP = gemm_bound(absP, add, Keff, splits, x3 and c.regime == "gauss")
    if epi in (L.EPI_BF16, L.EPI_F32, L.EPI_F16_DUAL):
        compare("C", got, P + bias64, cdt, dP)
        if ob is not None:
            compare("aux_out", ob.view, P + bias64, BF16, dP)
    elif epi == L.EPI_BF16_RELU:
        compare("C", got, torch.relu(P + bias64), cdt, dP)
    elif epi in (L.EPI_F32_RESID, L.EPI_BF16_ADD, L.EPI_PATCH):
        compare("C", got, P + bias64 + aux64, cdt, dP)
    elif epi == L.EPI_F32_ACC:
        compare("C", got, P + c0, cdt, dP)
    elif epi == L.EPI_BF16_DGELU:
        # (alpha acc) * aux: the product bound times |aux|, + one more fp32 operation
        ref = P * aux64
        compare("C", got, ref, cdt, dP * aux64.abs() + 2 * EPS * ref.abs())
        if c.dstats:
            # two partial column sums of the stored C per 256-row tile (the bias gradient's
            # partials: the consumer adds them all, so their sum per tile is what is defined)
            st = got.to(F64)
            for t in range((M + 255) // 256):
                rows = st[256 * t:min(M, 256 * t + 256)]
                part = sb.view[2 * t].to(F64) + sb.view[2 * t + 1].to(F64)
                _check(bool((part == rows.sum(0)).all()), f"dGELU column sums of row tile {t}")
    elif epi in GELU_EPIS:
        gref, dref = gelu_ref(P + bias64)
        bg, bd = gelu_bounds(P + bias64, dP)
        compare("aux_out", ob.view, dref, BF16, bd)
        if epi == L.EPI_BF16_GELU:
            compare("C", got, gref, BF16, bg)
        elif epi == L.EPI_F16_GELU:
            compare("C.f16", got[:, :N], gref, F16, bg)
            compare("C.bf16", got[:, N:].contiguous().view(BF16), gref, BF16, bg)
        else:
            hi, lo = got[:, :N].to(F64), got[:, N:2 * N].to(F64)
            compare("C.hi", got[:, :N], gref, BF16, bg)
            # lo = bf16(g - hi): |lo| <= 2^-8 |g|, its rounding <= 2^-9 |lo| <= 2^-17 |g|
            compare("C.hi+lo", hi + lo, gref, F64, bg + 2.0 ** -17 * gref.abs())
            _check(torch.equal(got[:, :N], got[:, 2 * N:]), "X3_GELU: segment 2 != segment 0")
    elif epi in (L.EPI_BF16_STATS, L.EPI_F32_STATS):
        if pair:
            hi, lo = got.to(F64), ob.view.to(F64)
            compare("C.hi", got, P, BF16, dP)
            stored = hi + lo
            if c.regime == "int":
                compare("C.hi+lo", stored, P, F64, dP)
            else:
                compare("C.hi+lo", stored, P, F64, dP + 2.0 ** -17 * P.abs())
        else:
            compare("C", got, P, cdt, dP)
            stored = got.to(F64)
        _check_stats(c, sb.view.view(-1, 2, N).to(F64), stored, M, N, fam, pair)
    else:
        raise AssertionError(f"no reference for epilogue {epi}")


def _check_stats(c, stats, stored, M, N, fam, pair):
    """The (sum, M2) records of each 128-row block against the header's definition, taken over the
    stored values: sum = sum_i v_i, M2 = sum_i (v_i - mean)^2.

    Integer regime: the sum is exact (integers below 2^24).  Otherwise, with n <= 128 rows and
    EPS per fp32 operation: |sum error| <= n EPS sum|v| (any summation order; a split pair adds
    the 2^-17 |v| by which hi + lo differs from the fp32 value the statistics are taken over),
    so the kernel's mean is off by dm <= EPS sum|v| (+ 2^-17 mean|v|); each deviation then by
    dm + EPS |d_i|, so sum d_i^2 by 2 sqrt(n M2) dm + n dm^2 + (n + 8) 2 EPS M2 (the squares, the
    n - 1 additions, second order); Chan's merge of the row-waves is algebraically exact and adds
    terms of the same form (means off by dm, weights <= n / 4): 4 sqrt(n M2) dm + n dm^2 more.
        |M2 error| <= (n + 8) 2 EPS M2 + 6 sqrt(n M2) dm + 2 n dm^2
    """
    for blk in range((M + 127) // 128):
        v = stored[128 * blk:min(M, 128 * blk + 128)]
        n = v.shape[0]
        s_ref = v.sum(0)
        m2_ref = ((v - s_ref / n) ** 2).sum(0)
        sabs = v.abs().sum(0)
        extra = 2.0 ** -17 * sabs if (pair and c.regime == "gauss") else 0.0
        s_err = (stats[blk, 0] - s_ref).abs()
        if c.regime == "int":
            _check(bool((s_err == 0).all()), f"stats sum of block {blk} not exact")
        else:
            lim = n * EPS * sabs + extra + half_ulp(s_ref, F32)
            r = RATIOS.add(fam + ":sum", s_err, lim)
            _check(r <= 1.0, f"stats sum of block {blk}: |err| / bound = {r:.3f}")
        dm = EPS * sabs + extra / n
        lim = ((n + 8) * 2 * EPS * m2_ref + 6 * torch.sqrt(n * m2_ref) * dm + 2 * n * dm * dm
               + half_ulp(m2_ref, F32))
        m2_err = (stats[blk, 1] - m2_ref).abs()
        _check(bool(torch.isfinite(stats[blk]).all()), f"stats of block {blk} not finite")
        if c.regime == "gauss":
            r = RATIOS.add(fam + ":M2", m2_err, lim)
        else:
            r = float((m2_err[lim > 0] / lim[lim > 0]).max()) if bool((lim > 0).any()) else 0.0
            _check(bool((m2_err[lim <= 0] == 0).all()), f"stats M2 of block {blk}: nonzero at M2 = 0")
        _check(r <= 1.0, f"stats M2 of block {blk}: |err| / bound = {r:.3f}")
