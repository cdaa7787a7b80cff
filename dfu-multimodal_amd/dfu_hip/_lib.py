"""ctypes binding of libdfu_hip.so — the C ABI declared in include/dfu_hip.h.

This is the only place the host touches the native library.  Loading fails loudly: there is
no CPU or ATen fallback for any op on the hot path (SURVEY.md §7 design stance).

Nothing of the ABI is written out here.  The header is read once at import by parse_header, a
strict reader of the restricted grammar the header uses (not a C parser): prototypes, `typedef
struct`s of scalars, pointers and scalar arrays, enums whose enumerators all carry `= n`, and
integer `#define`s.  Text it does not recognise raises HeaderError; it never guesses or skips.
The GEMM tile ids come the same way from the DFU_TILES rows of csrc/gemm_table.h (parse_tiles).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# DFU_HIP_LIB: another build of the library (A/B timing of two builds); default: in-tree
LIB_PATH = os.environ.get("DFU_HIP_LIB") or os.path.join(_HERE, "libdfu_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "dfu_hip.h"))
TILE_TABLE_PATH = os.path.normpath(os.path.join(_HERE, "..", "csrc", "gemm_table.h"))

c_float = ctypes.c_float
c_void_p = ctypes.c_void_p

_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "float": c_float}
_POINTEES = set(_SCALARS) | {"void", "double", "uint8_t"}  # and every struct declared so far
_RETURNS = {"int": ctypes.c_int32, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_PREPROCESSOR = re.compile(r"#\s*(ifndef\s+\w+_H|define\s+\w+_H|include\s+<stdint\.h>)")
_DEFINE = re.compile(r"#\s*define\s+(\w+)\s+(\S+)")
_DECLARATION = re.compile(
    r"\s*(?:enum\s+(\w+)\s*\{([^{}]*)\}"
    r"|typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)"
    r"|(const\s+char\s*\*|\w+)\s+(\w+)\s*\(([^()]*)\))\s*;")
# `[const] T name`, `[const] T* name`, `T* const* name`: base type, pointer part, the rest
_TYPED = re.compile(r"(?:const\s+)?(\w+)(\s+|\s*(?:\*\s*(?:const\b\s*)?)+)(.+)", re.S)
_DECLARATOR = re.compile(r"(\w+)(?:\s*\[\s*(\d+)\s*\])?")


class HeaderError(ValueError):
    """include/dfu_hip.h (or the tile table) holds text the reader does not recognise."""


def _integer(text, where):
    try:
        return int(text, 0)
    except ValueError:
        raise HeaderError(f"not an integer constant: {where.strip()!r}") from None


def _typed(text, structs):
    """`[const] T [*...] rest` -> (ctypes type, rest); any pointer is a c_void_p."""
    m = _TYPED.fullmatch(text.strip())
    if not m:
        raise HeaderError(f"unrecognised parameter or field: {text.strip()!r}")
    base, pointer = m[1], "*" in m[2]
    if base not in (_POINTEES | set(structs) if pointer else _SCALARS):
        raise HeaderError(f"unknown type {base!r} in {text.strip()!r}")
    return (c_void_p if pointer else _SCALARS[base]), m[3]


def _struct(name, body, structs):
    fields = []
    *stmts, tail = body.split(";")
    for stmt in stmts:
        ctype, rest = _typed(stmt, structs)
        declarators = [_DECLARATOR.fullmatch(d.strip()) for d in rest.split(",")]
        if not all(declarators) or (ctype is c_void_p and len(declarators) > 1):
            raise HeaderError(f"unrecognised field in struct {name}: {stmt.strip()!r}")
        fields += [(d[1], ctype * int(d[2]) if d[2] else ctype) for d in declarators]
    if tail.strip() or not fields:
        raise HeaderError(f"unrecognised text in struct {name}: {tail.strip()!r}")
    return type(name, (ctypes.Structure,), {"_fields_": fields,
                                            "__doc__": f"`{name}` of include/dfu_hip.h."})


def _function(ret, params, structs):
    ret = " ".join(ret.replace("*", " *").split())
    if ret not in _RETURNS:
        raise HeaderError(f"unknown return type {ret!r}")
    argtypes = []
    if params.strip() != "void":
        for p in params.split(","):
            ctype, name = _typed(p, structs)
            if not re.fullmatch(r"\w+", name):
                raise HeaderError(f"unrecognised parameter: {p.strip()!r}")
            argtypes.append(ctype)
    return _RETURNS[ret], argtypes


def parse_header(text):
    """The header's text -> (functions: name -> (restype, argtypes), structs: name ->
    ctypes.Structure class, enums: name -> {enumerator: value}, constants: #define -> value)."""
    functions, structs, enums, constants = {}, {}, {}, {}
    lines, cplusplus = [], False
    for line in _COMMENT.sub(" ", text).splitlines():
        s = line.strip()
        if not s.startswith("#"):
            if not cplusplus:  # `extern "C" {` and its `}`: not part of the C view
                lines.append(line)
        elif s == "#ifdef __cplusplus":
            cplusplus = True
        elif s == "#endif":
            cplusplus = False
        elif m := _DEFINE.fullmatch(s):
            constants[m[1]] = _integer(m[2], s)
        elif not _PREPROCESSOR.fullmatch(s):
            raise HeaderError(f"unrecognised preprocessor line: {s!r}")
    src, pos = "\n".join(lines), 0
    while src[pos:].strip():
        m = _DECLARATION.match(src, pos)
        if not m:
            raise HeaderError(f"unrecognised declaration: {src[pos:].split(';')[0].strip()!r}")
        pos = m.end()
        if m[1]:
            enums[m[1]] = {}
            for item in m[2].split(","):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*(\S+)\s*", item)
                if not e:
                    raise HeaderError(f"enum {m[1]}: enumerator without `= n`: {item.strip()!r}")
                enums[m[1]][e[1]] = _integer(e[2], item)
        elif m[3]:
            if m[3] != m[5]:
                raise HeaderError(f"typedef struct {m[3]} is named {m[5]}")
            structs[m[3]] = _struct(m[3], m[4], structs)
        else:
            functions[m[7]] = _function(m[6], m[8], structs)
    return functions, structs, enums, constants


def parse_tiles(text):
    """csrc/gemm_table.h -> [(name, TM, TN, phased)], the DFU_TILES rows: tile id = row + 1."""
    m = re.search(r"^#define DFU_TILES\(X\)((?:.*\\\n)*.*)", _COMMENT.sub(" ", text), re.M)
    if not m:
        raise HeaderError("no DFU_TILES table")
    rows = []
    for line in m[1].replace("\\\n", "\n").split("\n"):
        r = re.fullmatch(r"X\((\w+), (\d+), (\d+), \d+, (true|false), (?:true|false), [\d.]+, "
                         r"[\d.]+\)", line.strip())
        if r:
            rows.append((r[1], int(r[2]), int(r[3]), r[4] == "true"))
        elif line.strip():
            raise HeaderError(f"unrecognised DFU_TILES row: {line.strip()!r}")
    return rows


with open(HEADER_PATH) as _f:
    FUNCTIONS, STRUCTS, ENUMS, CONSTANTS = parse_header(_f.read())
with open(TILE_TABLE_PATH) as _f:
    TILE_ROWS = parse_tiles(_f.read())

GemmDesc = STRUCTS["dfu_gemm_desc"]
ReduceEntry = STRUCTS["dfu_reduce_entry"]
TransposeJob = STRUCTS["dfu_transpose_job"]
ResizeDesc = STRUCTS["dfu_resize_desc"]
AugParams = STRUCTS["dfu_aug_params"]

# Every enumerator and #define, by its header name (DFU_E_INVALID, DFU_AUG_CONTRAST) and by that
# name without the DFU_ (OPND_KMAJOR, EPI_F32_ACC, OPERAND_F16, X3_PAIRS, REDUCE_BATCH).
for _values in (CONSTANTS, *ENUMS.values()):
    globals().update(_values)
    globals().update({k.removeprefix("DFU_"): v for k, v in _values.items()})


def header_symbols():
    """Every function name declared in include/dfu_hip.h."""
    return sorted(FUNCTIONS)


class DfuError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


_lib = None


def load():
    """Load libdfu_hip.so once; raise if it is missing (never fall back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DfuError(
            f"libdfu_hip.so not found at {LIB_PATH}; build it with "
            f"`make -C dfu-multimodal_amd` (or __graft_entry__.build()). There is no fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().dfu_last_error_string()
        msg = msg.decode() if msg else ""
        raise DfuError(f"{what or 'dfu call'} failed (rc={rc}): {msg}", rc)
