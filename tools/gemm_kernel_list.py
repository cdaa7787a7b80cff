"""List every compiled dfu_gemm kernel (no GPU needed): dfu_gemm_plan with a tile hint returns
DFU_E_UNSUPPORTED exactly when that tile has no entry for the descriptor's (a_mode, b_mode,
epilogue, operand key), so probing tiles 1..11 x a_mode x b_mode x epilogues 0..15 x the three
operand keys (bf16; operand_type 1; x3_pairs 1 with a_seg) recovers the dispatch tables of
csrc/gemm_t*.hip, gemm_p8.hip and gemm_ps.hip from the built library.

tests/test_gemm_kernel_list_cpu.py compares the live probe with tests/golden/gemm_kernels.json
(a kernel added or dropped without regenerating the list fails), and tests/test_gemm_matrix_gpu.py
is parametrised over the same file: one forced-tile case per kernel.

    python tools/gemm_kernel_list.py > tests/golden/gemm_kernels.json
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dfu-multimodal_amd")]
from dfu_hip import _lib as L  # noqa: E402

FIELDS = ["tile", "a_mode", "b_mode", "epilogue", "key"]
KEYS = ["bf16", "f16", "x3"]  # dfu_gemm_desc.operand_type 0 / 1 / x3_pairs 1 with a_seg
NTILES, NMODES, NEPIS = 11, 6, 16


def probe_desc(tile, a_mode, b_mode, epilogue, key):
    """A descriptor the planner accepts for any kernel of that identity (never launched)."""
    d = L.GemmDesc()
    d.M, d.N, d.K = 256, 256, 256
    d.a_mode, d.b_mode, d.epilogue, d.tile = a_mode, b_mode, epilogue, tile
    d.lda = d.ldb = 256
    d.ldc = 3 * d.N  # (F16_GELU, X3_GELU: C holds two / three planes)
    d.alpha = 1.0
    if epilogue in (L.EPI_F16_GELU, L.EPI_X3_GELU):
        d.aux_out, d.ldaux_out = 1 << 20, d.N  # never dereferenced by the planner
    if key == "f16":
        d.operand_type = L.OPERAND_F16
    elif key == "x3":
        d.x3_pairs, d.a_seg, d.a_lo = 1, d.K // 2, 1 << 20
    return d


def supported(lib, tile, a_mode, b_mode, epilogue, key):
    d = probe_desc(tile, a_mode, b_mode, epilogue, key)
    t, sk = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.dfu_gemm_plan(ctypes.byref(d), ctypes.byref(t), ctypes.byref(sk))
    if rc == 0:
        assert t.value == tile, (tile, t.value)
    return rc == 0


def probe(lib):
    """Every supported [tile, a_mode, b_mode, epilogue, key], in probe order."""
    out = []
    for tile in range(1, NTILES + 1):
        for a in range(NMODES):
            for b in range(NMODES):
                for e in range(NEPIS):
                    for key in KEYS:
                        # (the F16 epilogues with bf16 operands: DFU_E_INVALID, no kernel either)
                        if supported(lib, tile, a, b, e, key):
                            out.append([tile, a, b, e, key])
    return out


def dumps(kernels):
    head = json.dumps({"fields": FIELDS, "count": len(kernels)}, separators=(",", ":"))[:-1]
    return (head + ',"kernels":[\n' +
            ",\n".join(json.dumps(k, separators=(",", ":")) for k in kernels) + "\n]}\n")


if __name__ == "__main__":
    sys.stdout.write(dumps(probe(L.load())))
