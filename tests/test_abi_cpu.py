"""dfu_hip._lib derives the Python side of the C ABI from include/dfu_hip.h and the tile table
from csrc/gemm_table.h.  Checked here without a GPU: every derived struct against the C
compiler's layout, a set of ABI values written out as literals (a reader that misparses cannot
agree with itself), that the reader refuses what it does not recognise, and that the header and
the built library declare and export the same functions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from dfu_hip import _lib as L
from dfu_hip import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float


def test_struct_layouts_match_c(tmp_path):
    """sizeof and every offsetof of every typedef struct of the header, from gcc."""
    assert {n: ctypes.sizeof(s) for n, s in L.STRUCTS.items()} == {
        "dfu_gemm_desc": 240, "dfu_transpose_job": 40, "dfu_reduce_entry": 32,
        "dfu_resize_desc": 40, "dfu_aug_params": 92}
    assert len(L.GemmDesc._fields_) == 41
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "dfu_hip.h"', "int main(void){"]
    want = []
    for name, s in L.STRUCTS.items():
        src.append(f'printf("%zu\\n", sizeof({name}));')
        want.append((f"sizeof({name})", ctypes.sizeof(s)))
        for f, _ in s._fields_:
            src.append(f'printf("%zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
            want += [(f"offsetof({name}, {f})", getattr(s, f).offset),
                     (f"sizeof({name}.{f})", getattr(s, f).size)]
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert len(out) == len(want)
    assert [(w, o) for (w, _), o in zip(want, out)] == want


def test_numpy_views_of_the_device_tables():
    """The staging records of data.gpu_transforms are the derived structs, field for field."""
    for s in (L.ResizeDesc, L.AugParams):
        dt = np.dtype(s)
        assert dt.itemsize == ctypes.sizeof(s) and dt.names == tuple(f for f, _ in s._fields_)
        assert [dt.fields[f][1] for f in dt.names] == [getattr(s, f).offset for f in dt.names]
    aug = np.dtype(L.AugParams)
    assert aug["rot"].shape == (6,) and aug["rot"].base == "<i4" and aug["factor"].base == "<f4"


def test_frozen_abi_values():
    assert L.OPND_CONV_WGRAD_X == 5
    assert (L.EPI_F32_ACC, L.EPI_F32_STATS, L.EPI_F16_GELU) == (7, 11, 15)
    assert (L.DFU_E_INVALID, L.DFU_E_UNSUPPORTED, L.REDUCE_BATCH) == (1001, 1002, 8)
    assert (L.OPERAND_BF16, L.OPERAND_F16) == (0, 1)
    assert (ops.X3_A, ops.X3_B, ops.X3_PAIRS) == (0, 1, 2)
    assert (L.DFU_AUG_BRIGHTNESS, L.DFU_AUG_CONTRAST, L.DFU_AUG_SATURATION) == (0, 1, 2)
    assert (L.DFU_AUG_ORDER_FLIP_ROTATE, L.DFU_AUG_ORDER_ROTATE_FLIP) == (0, 1)
    assert len(L.ENUMS["dfu_epilogue"]) == 16 and len(L.ENUMS["dfu_operand_mode"]) == 6
    assert ops.TILES["auto"] == 0 and ops.TILES["192x256ps"] == 9 and ops.TILES["128x64o2"] == 11
    assert len(ops.TILES) == 12 and sorted(ops.TILES.values()) == list(range(12))
    assert ops.TILE_DIMS[7] == (256, 256, True)
    assert ops.TILE_DIMS[9] == (192, 256, True)
    assert ops.TILE_DIMS[10] == (256, 64, False)
    assert L.FUNCTIONS["dfu_gemm_f32"] == (
        I32, [I32, I32, I32, P, I64, I64, P, I64, I64, P, I64, P, I32, I32, P, I64, P])
    assert L.FUNCTIONS["dfu_dropout_fwd"] == (
        I32, [P, P, P, I64, F, ctypes.c_uint64, P, I32, P])
    assert L.FUNCTIONS["dfu_bn_bwd_ws_bytes"] == (I64, [I64, I32])
    assert L.FUNCTIONS["dfu_last_error_string"] == (ctypes.c_char_p, [])
    lib = L.load()
    assert lib.dfu_gemm_f32.argtypes == L.FUNCTIONS["dfu_gemm_f32"][1]
    assert lib.dfu_bn_bwd_ws_bytes.restype is I64


ACCEPTED = """
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define DFU_N 0x10 /* a constant; with ( and ; in the comment */
enum dfu_e { DFU_A = 0, // one; (
             DFU_B = -3 };
typedef struct dfu_s {
  int32_t a, b;     /* two declarators; */
  const void* p;
  float f[3];       // an array (
  int64_t n;
} dfu_s;
const char* dfu_name(void);
int64_t dfu_three(const dfu_s* s,
                  void* const* streams,   /* ; */
                  uint64_t seed, float x, int32_t* out);
#ifdef __cplusplus
}
#endif
#endif /* X_H */
"""


def test_reader_accepts_the_header_grammar():
    functions, structs, enums, constants = L.parse_header(ACCEPTED)
    assert constants == {"DFU_N": 16} and enums == {"dfu_e": {"DFU_A": 0, "DFU_B": -3}}
    assert functions == {"dfu_name": (ctypes.c_char_p, []),
                         "dfu_three": (I64, [P, P, ctypes.c_uint64, F, P])}
    s = structs["dfu_s"]
    assert [f for f, _ in s._fields_] == ["a", "b", "p", "f", "n"]
    assert (s.a.offset, s.b.offset, s.p.offset, s.f.offset, s.n.offset) == (0, 4, 8, 16, 32)
    assert s.f.size == 12
    assert ctypes.sizeof(s) == 40


@pytest.mark.parametrize("text,msg", [
    ("int dfu_f(size_t n);", "size_t"),                                  # an unknown type
    ("int dfu_f(unsigned int n);", "unsigned"),
    ("double dfu_f(int32_t n);", "double"),                              # an unknown return type
    ("typedef struct dfu_s { int32_t a; char c; } dfu_s;", "char"),
    ("enum dfu_e { DFU_A = 0, DFU_B };", "DFU_B"),                       # no value
    ("int dfu_f(int32_t (*cb)(int32_t), void* stream);", "dfu_f"),       # a function pointer
    ("typedef struct dfu_s { int32_t a; struct { int32_t b; } in; } dfu_s;", "dfu_s"),
    ("typedef struct dfu_s { int32_t a; union { int32_t b; float c; } u; } dfu_s;", "dfu_s"),
    ("typedef struct dfu_s { int32_t a : 3; } dfu_s;", "a : 3"),         # a bit-field
    ("typedef struct dfu_s { void *p, *q; } dfu_s;", "*q"),
    ("typedef struct dfu_s { int32_t a; } dfu_t;", "dfu_t"),
    ("int dfu_f(int32_t);", "int32_t"),                                  # an unnamed parameter
    ("int dfu_f();", "unrecognised parameter"),                          # not (void)
    ("extern int dfu_counter;", "dfu_counter"),                          # matches no rule
    ("int dfu_f(int32_t n)", "dfu_f"),                                   # no semicolon
    ("#define DFU_X (1 << 4)", "DFU_X"),
    ("#define DFU_X 1.5", "DFU_X"),
    ("#if 1\nint dfu_f(void);\n#endif", "#if 1"),
])
def test_reader_refuses_what_it_does_not_recognise(text, msg):
    with pytest.raises(L.HeaderError) as e:
        L.parse_header(text)
    assert msg in str(e.value)


def test_tile_table_reader():
    table = ("#define DFU_TILES(X)   \\\n  X(8x8, 8, 16, 1, false, true, 0.5, 4.8) /* a; ( */ \\\n"
             "  X(16x8ps, 16, 8, 2, true, false, 3.0, 20.0)\n\nnamespace dfu {}\n")
    assert L.parse_tiles(table) == [("8x8", 8, 16, False), ("16x8ps", 16, 8, True)]
    for bad in ("", table.replace("true, 0.5", "maybe, 0.5"), table.replace(", 4.8", "")):
        with pytest.raises(L.HeaderError):
            L.parse_tiles(bad)


def test_library_exports_no_undeclared_function():
    """The reverse of test_host_cpu's export check: every dfu_ function the built library exports
    is declared in the header -- but for the error setter its translation units share
    (csrc/common.h), which has C linkage and no caller outside the library."""
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    symbols = [ln.split() for ln in out.splitlines()]  # address, type, name
    exported = {s[2] for s in symbols if len(s) == 3 and s[1] == "T" and s[2].startswith("dfu_")}
    assert len(exported) >= 100
    assert exported - {"dfu_set_error"} == set(L.header_symbols())
