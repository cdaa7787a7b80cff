"""Calibration only (not a product path): the library GEMM (torch.matmul -> hipBLASLt) against
dfu's MFMA template on the ViT GEMM shapes of the B=64 step, same layouts, bf16 in, plain bf16
(fwd/dgrad) or fp32 (wgrad) out, random operands.  Tells how far the template is from what the
vendor library reaches on this chip and clock.
Usage (GPU box): python tools/blas_compare.py"""
import _harness
import torch
from _harness import time_us

from dfu_hip import _lib as L
from dfu_hip import ops


def main():
    dev, bf = "cuda", torch.bfloat16

    def T(*s):
        return (torch.randn(*s, device=dev) * 0.1).to(bf)

    print(f"{'case':34s} {'hipBLASLt':>16s} {'dfu':>16s}")
    for name, (M, N, K) in _harness.VIT_SHAPES.items():
        A, W, dY = T(M, K), T(N, K), T(M, N)
        C, dX = torch.empty(M, N, dtype=bf, device=dev), torch.empty(M, K, dtype=bf, device=dev)
        dW = torch.zeros(N, K, device=dev)
        fl = 2 * M * N * K
        rows = [
            (f"fwd  {name} {M}x{N}x{K}", lambda: torch.matmul(A, W.t(), out=C),
             lambda: ops.gemm(M, N, K, A, K, W, K, C, N, epilogue=L.EPI_BF16)),
            (f"dgrd {name} {M}x{K}x{N}", lambda: torch.matmul(dY, W, out=dX),
             lambda: ops.gemm(M, K, N, dY, N, W, K, dX, K, b_mode=L.OPND_MNMAJOR,
                              epilogue=L.EPI_BF16)),
            (f"wgrd {name} {N}x{K}x{M}", lambda: torch.mm(dY.t(), A, out_dtype=torch.float32),
             lambda: ops.gemm(N, K, M, dY, N, A, K, dW, K, a_mode=L.OPND_MNMAJOR,
                              b_mode=L.OPND_MNMAJOR, epilogue=L.EPI_F32_ACC)),
        ]
        for label, blas, ours in rows:
            try:
                tb = time_us(blas, 30, 3)
                sb = f"{tb:7.1f}us {fl / tb / 1e6:5.0f}T"
            except Exception as e:  # out_dtype may be unsupported: fall back to a bf16 product
                if label.startswith("wgrd"):
                    tb = time_us(lambda: torch.mm(dY.t(), A), 30, 3)
                    sb = f"{tb:7.1f}us {fl / tb / 1e6:5.0f}T*"
                else:
                    sb = f"err {type(e).__name__}"
            to = time_us(ours, 30, 3)
            print(f"{label:34s} {sb:>16s} {to:7.1f}us {fl / to / 1e6:5.0f}T", flush=True)
    print("(* = bf16 output: torch.mm out_dtype=float32 unavailable)")


if __name__ == "__main__":
    main()
