"""Run one GEMM of the step repeatedly (for rocprofv3 --pmc counter passes on a single kernel).

  python tools/gemm_one.py <case> [--tile T] [--iters N]
  cases: fc1_fwd (12608x3072x768, KM x KM, BF16), fc1_gelu (same, GELU epilogue),
         fc2_dgrad (12608x3072x768, KM x MN, DGELU), fc1_wgrad (3072x768x12608, MN x MN, F32_ACC),
         l1c3_fwd (200704x256x64 1x1 conv, STATS), fc2_fwd_resid (12608x768x3072, F32_RESID),
         fc2_wgrad / qkv_wgrad / proj_wgrad (768x3072 / 2304x768 / 768x768 x 12608, F32_ACC),
         l1c3x3_fwd / l1c1x3_fwd / l3c2x3_fwd (bf16x3 pair convs; FLOPs: the MFMA work, 3 products)
"""
import argparse

import _harness
import torch

from dfu_hip import _lib as L
from dfu_hip import ops


def T(*s, dtype=torch.bfloat16):
    return (torch.randn(*s, device="cuda") * 0.1).to(dtype)


CHECK = []  # (HIP result, fp32 reference) thunks for --check


def vit(case):
    """(M, N, K) of a ViT case <layer>_<kind>: the forward's _harness.VIT_SHAPES entry, N and K
    swapped for an input gradient, N x K x M for a weight gradient."""
    layer, kind = case.split("_", 1)
    M, N, K = _harness.VIT_SHAPES[layer.replace("x3", "")]
    if kind.startswith("dgrad"):
        return M, K, N
    return (N, K, M) if kind == "wgrad" else (M, N, K)


def build(case, tile):
    if case in ("qkv_fwd", "proj_fwd", "fc2_fwd"):
        M, N, K = vit(case)
        A, B, C = T(M, K), T(N, K), T(M, N)
        bias = T(N, dtype=torch.float32)
        CHECK.append(lambda: (C.float(), A.float() @ B.float().t() + bias))
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, K, C, N, epilogue=L.EPI_BF16,
                                               bias=bias, tile=tile)
    if case in ("fc1_fwd", "fc1_gelu"):
        M, N, K = vit("fc1_fwd")
        A, B, C, pre = T(M, K), T(N, K), T(M, N), T(M, N)
        epi = L.EPI_BF16_GELU if case == "fc1_gelu" else L.EPI_BF16
        kw = dict(aux_out=pre, ldaux_out=N) if case == "fc1_gelu" else {}
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, K, C, N, epilogue=epi, tile=tile, **kw)
    if case == "fc2_dgrad":
        M, N, K = vit(case)
        A, B, C, h = T(M, K), T(K, N), T(M, N), T(M, N)
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, N, C, N, b_mode=L.OPND_MNMAJOR,
                                               epilogue=L.EPI_BF16_DGELU, aux=h, ldaux=N, tile=tile)
    if case in ("fc1_dgrad", "qkv_dgrad"):
        M, N, K = vit(case)
        A, B, C = T(M, K), T(K, N), T(M, N)
        CHECK.append(lambda: (C.float(), A.float() @ B.float()))
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, N, C, N, b_mode=L.OPND_MNMAJOR,
                                               epilogue=L.EPI_BF16, tile=tile)
    if case in ("fc1_dgrad_t", "qkv_dgrad_t", "fc2_dgrad_t", "proj_dgrad_t"):
        # the dgrads with a pre-transposed weight: B K-contiguous (KM x KM)
        M, N, K = vit(case)
        A, B, C, h = T(M, K), T(N, K), T(M, N), T(M, N)
        if case == "fc2_dgrad_t":
            return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, K, C, N,
                                                   epilogue=L.EPI_BF16_DGELU, aux=h, ldaux=N,
                                                   tile=tile)
        CHECK.append(lambda: (C.float(), A.float() @ B.float().t()))
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, K, C, N, epilogue=L.EPI_BF16,
                                               tile=tile)
    if case in ("proj_fwd_resid", "fc2_fwd_resid", "fc2x3_fwd_resid", "projx3_fwd_resid"):
        # fc2_fwd_resid is the step's fc2 forward (fp32 residual-stream epilogue); x3: K tripled
        M, N, K = vit(case)
        K *= 3 if "x3" in case else 1
        A, B = T(M, K), T(N, K)
        C, X = T(M, N, dtype=torch.float32), T(M, N, dtype=torch.float32)
        bias = T(N, dtype=torch.float32)
        CHECK.append(lambda: (C - X, A.float() @ B.float().t() + bias))
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, K, C, N,
                                               epilogue=L.EPI_F32_RESID, bias=bias, aux=X,
                                               ldaux=N, tile=tile)
    if case in ("fc1_wgrad", "fc2_wgrad", "qkv_wgrad", "proj_wgrad"):
        M, N, K = vit(case)
        A, B = T(K, M), T(K, N)
        C = torch.zeros(M, N, device="cuda")
        if case != "fc1_wgrad":
            CHECK.append(lambda: (C.clone(), A.float().t() @ B.float()))
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, M, B, N, C, N, a_mode=L.OPND_MNMAJOR,
                                               b_mode=L.OPND_MNMAJOR, epilogue=L.EPI_F32_ACC,
                                               tile=tile)
    if case in ("l1c3x3_fwd", "l1c1x3_fwd", "l3c2x3_fwd"):
        # the parity mode's bf16x3 ResNet convs on interleaved hi/lo pairs (functional.conv_fwd_x3):
        # layer-1 conv3 (1x1, 64 -> 256) and conv1 (1x1, 256 -> 64), layer-3 conv2 (3x3, 256)
        n, h, w, c, k, r = {"l1c3x3_fwd": (64, 56, 56, 64, 256, 1),
                            "l1c1x3_fwd": (64, 56, 56, 256, 64, 1),
                            "l3c2x3_fwd": (64, 14, 14, 256, 256, 3)}[case]
        M = n * h * w
        hi, lo = T(M, c), T(M, c)
        w3 = T(k, r * r * 2 * c)
        y, y_lo = T(M, k), T(M, k)
        st = torch.empty(ops.stats_tiles(M), 2, k, device="cuda")
        xk = dict(x3=True, a_lo=lo, x3_pairs=True, aux_out=y_lo, ldaux_out=k)
        if r == 1:
            return 2 * M * k * c * 3, lambda: ops.gemm(M, k, 2 * c, hi, c, w3, 2 * c, y, k,
                                                       epilogue=L.EPI_F32_STATS, stats=st,
                                                       tile=tile, **xk)
        g3 = ops.ConvGeom(n, h, w, 2 * c, k, r, r, 1, 1)
        K3 = r * r * 2 * c
        return 2 * M * k * r * r * c * 3, lambda: ops.gemm(M, k, K3, hi, 0, w3, K3, y, k,
                                                           a_mode=L.OPND_CONV_FWD,
                                                           epilogue=L.EPI_F32_STATS, stats=st,
                                                           conv=g3, tile=tile, **xk)
    if case == "l1c3_fwd":
        M, N, K = 200704, 256, 64
        A, B, C = T(M, K), T(N, K), T(M, N)
        st = torch.empty(ops.stats_tiles(M), 2, N, device="cuda")
        return 2 * M * N * K, lambda: ops.gemm(M, N, K, A, K, B, K, C, N,
                                               epilogue=L.EPI_BF16_STATS, stats=st, tile=tile)
    raise SystemExit(f"unknown case {case}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--check", action="store_true", help="one launch checked against torch fp32")
    a = ap.parse_args()
    flops, fn = build(a.case, a.tile)
    fn()
    torch.cuda.synchronize()
    if a.check:
        if not CHECK:
            raise SystemExit(f"--check: no reference for {a.case}")
        got, ref = CHECK[0]()
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"{a.case} tile {a.tile}: max rel err {err:.2e}")
        if not err < 1e-2:
            raise SystemExit(f"{a.case}: CHECK FAILED")
        return
    us = _harness.time_us(fn, a.iters, 0)
    print(f"{a.case} tile {a.tile}: {us:.1f} us  {flops / us / 1e6:.0f} TFLOP/s")


if __name__ == "__main__":
    main()
