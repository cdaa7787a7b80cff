"""dfu_hip.streams without a GPU: the capture recorder and the guard it arms, and the rule that
no module of the package reads another module's private stream, ops, functional, graphs or
grads state."""
import ast
import glob
import os

import pytest

from dfu_hip import _lib as L
from dfu_hip import streams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWNERS = ("streams", "ops", "functional", "graphs", "grads")


def test_the_recorder_arms_the_capture_guard():
    streams.refuse_in_capture("x")  # not recording, no GPU context: nothing to refuse
    with streams.recording():
        with pytest.raises(L.DfuError, match="inside a HIP-graph capture"):
            streams.refuse_in_capture("x")
        with pytest.raises(L.DfuError, match="inside a HIP-graph capture"):
            streams.new_stream(0)  # refused before any library or GPU call
    streams.refuse_in_capture("x")


def test_the_recorder_ends_when_its_body_raises():
    with pytest.raises(KeyError):
        with streams.recording():
            raise KeyError("step failed")
    assert streams.seen_streams() == []
    streams.refuse_in_capture("x")  # not recording any more


def _private_accesses(path):
    """(line, "alias._name") of every private attribute read through a name this file bound
    to one of the OWNERS modules by an import."""
    with open(path) as f:
        tree = ast.parse(f.read())
    me = os.path.splitext(os.path.basename(path))[0]
    aliases = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):  # from . import functional as Fn
            aliases |= {a.asname or a.name for a in node.names
                        if a.name in OWNERS and a.name != me}
        elif isinstance(node, ast.Import):  # import dfu_hip.ops as ops
            aliases |= {a.asname for a in node.names
                        if a.asname and a.name.rsplit(".", 1)[-1] in OWNERS}
    return [(n.lineno, f"{n.value.id}.{n.attr}") for n in ast.walk(tree)
            if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
            and n.value.id in aliases and n.attr.startswith("_") and not n.attr.startswith("__")]


def test_no_module_reads_another_modules_private_state():
    files = sorted(glob.glob(os.path.join(REPO, "dfu-multimodal_amd", "**", "*.py"),
                             recursive=True))
    assert len(files) >= 20
    found = {os.path.relpath(p, REPO): hits for p in files if (hits := _private_accesses(p))}
    assert not found, found


def test_the_private_access_walk_sees_what_it_should(tmp_path):
    p = tmp_path / "user.py"
    p.write_text("from . import functional as Fn, _lib as L\nimport torch.nn as nn\n"
                 "Fn._grad_streams.clear()\nL._handle\nm = nn.Linear(1, 1)\nm._parameters\n"
                 "Fn.__name__\n")
    assert _private_accesses(str(p)) == [(3, "Fn._grad_streams")]
