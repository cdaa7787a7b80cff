"""Yardstick: the persistent 256x256 GEMM (tile 8) and the library's plan on square shapes and
the ViT forward shapes, beside torch.matmul (hipBLASLt) on the same random bf16 operands.
Separates what the K-loop delivers (long K, many tiles) from what the ViT shapes cost (K = 768,
150-600 tiles).  HIP events, 20 launches each.
  python tools/gemm_square.py"""
import _harness
import torch
from _harness import VIT_SHAPES, time_us

from dfu_hip import _lib as L
from dfu_hip import ops

SHAPES = [(4096, 4096, 4096), (8192, 8192, 8192), VIT_SHAPES["qkv"], VIT_SHAPES["fc1"],
          VIT_SHAPES["fc2"], VIT_SHAPES["proj"], (16384, 4096, 768),
          (_harness.VIT_ROWS, 768, 12288)]


def main():
    print(f"{'shape':>22s} {'tile':>6s} {'us':>9s} {'TF/s':>7s}")
    for M, N, K in SHAPES:
        A = (torch.rand(M, K, device="cuda") * 2 - 1).to(torch.bfloat16)
        B = (torch.rand(N, K, device="cuda") * 2 - 1).to(torch.bfloat16)
        C = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        fl = 2.0 * M * N * K
        for tile in (0, 8):
            us = time_us(lambda: ops.gemm(M, N, K, A, K, B, K, C, N, epilogue=L.EPI_BF16,
                                          tile=tile), 20, 1)
            print(f"{M:>6d}x{N:>5d}x{K:>5d} {('auto' if tile == 0 else tile):>6} {us:9.1f} "
                  f"{fl / us / 1e6:7.0f}", flush=True)
        us = time_us(lambda: torch.matmul(A, B.t(), out=C), 20, 1)
        print(f"{M:>6d}x{N:>5d}x{K:>5d} {'blaslt':>6s} {us:9.1f} {fl / us / 1e6:7.0f}", flush=True)


if __name__ == "__main__":
    main()
