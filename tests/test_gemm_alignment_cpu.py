"""Alignment rules of dfu_gemm that are refusals (include/dfu_hip.h): checked without a GPU, the
descriptors fail validation before anything is launched.  The store classes that alignment only
demotes are test_gemm_matrix_gpu.py::test_output_pointer_alignment."""
import ctypes

import pytest

from dfu_hip import _lib as L

BASE = 1 << 20  # never dereferenced


def _dgrad(**kw):
    """2x9x14x64 <- 128 filters 1x1 / stride 2: three of the four stride phases have no tap."""
    d = L.GemmDesc()
    d.conv_n, d.conv_h, d.conv_w, d.conv_c, d.conv_k = 2, 9, 14, 64, 128
    d.conv_r = d.conv_s = 1
    d.conv_stride, d.conv_pad, d.conv_p, d.conv_q = 2, 0, 5, 7
    d.M, d.N, d.K = 2 * 9 * 14, 64, 128
    d.a_mode, d.b_mode, d.epilogue = L.OPND_CONV_DGRAD, L.OPND_CONV_DGRAD_W, L.EPI_BF16_ADD
    d.A = d.B = d.C = d.aux = BASE
    d.lda, d.ldb, d.ldc, d.ldaux = 128, 64, 72, 72
    d.alpha = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw", [dict(ldc=68), dict(C=BASE + 8), dict(ldaux=68),
                                dict(aux=BASE + 8), dict(C=BASE + 2)])
def test_tapless_phase_fill_refuses_misaligned_outputs(kw):
    lib = L.load()
    d = _dgrad(**kw)
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_INVALID
    assert "tapless phase" in lib.dfu_last_error_string().decode()


def test_tapless_phase_fill_ignores_aux_without_the_add():
    """BF16 has no addend: a stale aux pointer does not matter, the output still does."""
    lib = L.load()
    d = _dgrad(epilogue=L.EPI_BF16, aux=BASE + 2, ldaux=3, C=BASE + 8)
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_INVALID
    assert "tapless phase" in lib.dfu_last_error_string().decode()


def test_workspace_and_column_sum_alignment():
    lib = L.load()
    d = L.GemmDesc()
    d.M = d.N = d.K = 256
    d.A = d.B = d.C = BASE
    d.lda = d.ldb = d.ldc = 256
    d.a_mode = d.b_mode = L.OPND_MNMAJOR
    d.epilogue, d.split_k, d.tile = L.EPI_F32_ACC, 2, 1
    d.workspace, d.workspace_bytes = BASE + 8, 1 << 20
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_INVALID
    assert "workspace must be 16-byte aligned" in lib.dfu_last_error_string().decode()
    d = L.GemmDesc()
    d.M = d.N = d.K = 256
    d.A = d.B = d.C = d.aux = BASE
    d.lda = d.ldb = d.ldc = d.ldaux = 256
    d.epilogue, d.tile, d.stats = L.EPI_BF16_DGELU, 8, BASE + 4
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_INVALID
    assert "column sums" in lib.dfu_last_error_string().decode()
