"""Every global name the package's code reads exists: for each module of dfu_hip, models,
training and data, the source is compiled and every code object in it (functions, methods,
closures, comprehensions) is walked; each LOAD_GLOBAL / LOAD_NAME operand must be an attribute of
the imported module or a builtin.  A function that still calls a class renamed or removed long
ago (nn.Conv2d once ended in a Function that no longer existed) fails here, on a machine without
a GPU, instead of at its first call."""
import builtins
import dis
import importlib
import pathlib
import types

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1] / "dfu-multimodal_amd"
PACKAGES = ("dfu_hip", "models", "training", "data")


def _module_names():
    names = []
    for pkg in PACKAGES:  # the Python sources only (dfu_hip also holds the built library)
        for path in sorted((ROOT / pkg).rglob("*.py")):
            parts = path.relative_to(ROOT).with_suffix("").parts
            names.append(".".join(parts[:-1] if parts[-1] == "__init__" else parts))
    return names


def _code_objects(code):
    yield code
    for const in code.co_consts:
        if isinstance(const, types.CodeType):
            yield from _code_objects(const)


MODULES = _module_names()


def test_every_package_is_walked():
    assert {"dfu_hip.functional", "dfu_hip.nn", "dfu_hip.ops"} <= set(MODULES)
    assert all(any(m.startswith(p + ".") for m in MODULES) for p in PACKAGES), MODULES


@pytest.mark.parametrize("name", MODULES)
def test_global_names_resolve(name):
    mod = importlib.import_module(name)
    code = compile(pathlib.Path(mod.__file__).read_text(), mod.__file__, "exec")
    unresolved = []
    for co in _code_objects(code):
        # a class body reads its own earlier attributes, and the module a name it later
        # deletes, by LOAD_NAME: a name the same code object binds counts as known there
        stored = {i.argval for i in dis.get_instructions(co) if i.opname == "STORE_NAME"}
        for ins in dis.get_instructions(co):
            if ins.opname not in ("LOAD_GLOBAL", "LOAD_NAME"):
                continue
            n = ins.argval
            if hasattr(mod, n) or hasattr(builtins, n):
                continue
            if ins.opname == "LOAD_NAME" and n in stored:
                continue
            unresolved.append(f"{co.co_name}: {n}")
    assert not unresolved, f"{name} reads names that do not exist: {sorted(set(unresolved))}"
