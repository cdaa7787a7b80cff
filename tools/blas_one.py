"""Calibration only (not a product path): one ViT GEMM of the B = 64 step through torch.matmul
(-> hipBLASLt), repeated, for rocprofv3 kernel-trace / --pmc passes beside tools/gemm_one.py's
dfu run of the same case (profiles/r16_blas_counters.md).
  python tools/blas_one.py <case> [--iters N]
  cases: qkv_fwd, fc1_fwd, fc2_fwd (A [M,K] W[N,K]^T), qkv_dgrad_t, fc1_dgrad_t (dY [M,K] W [K,N])"""
import argparse

import _harness
import torch

CASES = ("qkv_fwd", "fc1_fwd", "fc2_fwd", "qkv_dgrad_t", "fc1_dgrad_t")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=sorted(CASES))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    M, N, K = _harness.VIT_SHAPES[a.case.split("_")[0]]
    fwd = a.case.endswith("_fwd")
    if not fwd:  # the input gradient: N and K swapped
        N, K = K, N
    bf = torch.bfloat16
    A = (torch.randn(M, K, device="cuda") * 0.1).to(bf)
    C = torch.empty(M, N, dtype=bf, device="cuda")
    if fwd:
        W = (torch.randn(N, K, device="cuda") * 0.1).to(bf)
        fn = lambda: torch.matmul(A, W.t(), out=C)  # noqa: E731
    else:
        W = (torch.randn(K, N, device="cuda") * 0.1).to(bf)
        fn = lambda: torch.matmul(A, W, out=C)  # noqa: E731
    us = _harness.time_us(fn, a.iters, 3)
    print(f"blas {a.case} {M}x{N}x{K}: {us:.1f} us {2 * M * N * K / us / 1e6:.0f} TFLOP/s")


if __name__ == "__main__":
    main()
