"""Time the persistent 256x256 GEMM (tile 8) under a timing-ablation build of the library
(tools/build_exp.sh ablate_<mask> gemm_ps -DDFU_PS_ABLATE=<mask> ->
dfu_hip/libdfu_exp_ablate_<mask>.so; results wrong by design): what the K-loop's MFMAs, LDS
reads, DMA, barrier and epilogue each cost on a square and the ViT forward shapes.  One process
per library ('zero': all-zero operands; a non-numeric tag is the experiment build
dfu_hip/libdfu_exp_<tag>.so, whose results are checked against torch):
  for m in full 1 2 4 8 12 16; do python tools/gemm_ablate.py $m; done"""
import os
import sys

import _harness
from _harness import VIT_SHAPES


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "full"
    zero = len(sys.argv) > 2 and sys.argv[2] == "zero"  # zero operands: the chip's clock rises
    if tag != "full":  # before dfu_hip is imported: it reads the variable once
        name = f"ablate_{tag}" if tag.isdigit() else tag
        os.environ["DFU_HIP_LIB"] = os.path.join(_harness.PKG, "dfu_hip", f"libdfu_exp_{name}.so")
    import torch

    from dfu_hip import _lib as L
    from dfu_hip import ops
    out = []
    for M, N, K in [(4096, 4096, 4096), VIT_SHAPES["fc1"], VIT_SHAPES["fc2"], VIT_SHAPES["qkv"]]:
        A = ((torch.rand(M, K, device="cuda") * 2 - 1) * (0 if zero else 1)).to(torch.bfloat16)
        B = ((torch.rand(N, K, device="cuda") * 2 - 1) * (0 if zero else 1)).to(torch.bfloat16)
        C = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        us = _harness.time_us(lambda: ops.gemm(M, N, K, A, K, B, K, C, N, epilogue=L.EPI_BF16,
                                               tile=8), 20, 1)
        if not tag.isdigit():  # an experiment build (not a timing ablation): check the result too
            ref = (A.float() @ B.float().t())
            err = ((C.float() - ref).abs().max() / ref.abs().max()).item()
            assert err < 1e-2, (tag, M, N, K, err)
        out.append(f"{M}x{N}x{K} {us:7.1f} us {2.0 * M * N * K / us / 1e6:6.0f} TF")
    print(f"[{tag + (' zero' if zero else ''):>9s}] " + " | ".join(out), flush=True)


if __name__ == "__main__":
    main()
