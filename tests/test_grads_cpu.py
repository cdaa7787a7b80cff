"""dfu_hip.grads without a GPU: the per-parameter producer protocol, the grad-ready hooks, the
end-of-backward join's arming outside a backward pass, and two source rules -- the producer and
self-joining attributes are named in grads.py alone, and the package's import graph is acyclic
with functional above optim, parallel, graphs and grads."""
import ast
import glob
import os

import torch

from dfu_hip import grads

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "dfu-multimodal_amd", "dfu_hip")


def test_producer_protocol():
    p = torch.nn.Parameter(torch.zeros(3))
    a, b = object(), object()
    assert grads.producer(p) is None
    grads.note_producer(p, a)
    assert grads.producer(p) is a
    grads.note_producer(p, a)
    assert grads.producer(p) is a
    grads.note_producer(p, b)
    assert grads.producer(p) is grads.MIXED
    grads.note_producer(p, a)
    assert grads.producer(p) is grads.MIXED
    grads.clear_producers([p])
    assert grads.producer(p) is None
    assert grads.MIXED is not None and grads.MIXED is not a


def test_wants_and_grad_or_none_on_the_host():
    p = torch.nn.Parameter(torch.zeros(3), requires_grad=False)
    assert not grads.wants(None) and not grads.wants(p)
    assert grads.grad_or_none(None) is None and grads.grad_or_none(p) is None and p.grad is None


def test_grad_ready_hooks_run_in_order_once_per_parameter():
    p, q = torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))
    calls = []
    first = grads.register_grad_ready_hook(lambda t: calls.append(("first", id(t))))
    second = grads.register_grad_ready_hook(lambda t: calls.append(("second", id(t))))
    try:
        grads.grads_done(p, None, q)
    finally:
        grads.remove_grad_ready_hook(first)
        grads.remove_grad_ready_hook(second)
    assert calls == [("first", id(p)), ("second", id(p)), ("first", id(q)), ("second", id(q))]
    calls.clear()
    grads.grads_done(p)  # both removed
    assert calls == []


def test_a_hook_removed_by_another_hook_still_runs_in_that_notification():
    p, q = torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))
    calls = []

    def victim(t):
        calls.append(("victim", id(t)))

    def remover(t):
        calls.append(("remover", id(t)))
        grads.remove_grad_ready_hook(victim)
    grads.register_grad_ready_hook(remover)
    grads.register_grad_ready_hook(victim)
    try:
        grads.grads_done(p, q)  # the snapshot taken at entry is notified to its end
        assert calls == [("remover", id(p)), ("victim", id(p)),
                         ("remover", id(q)), ("victim", id(q))]
        calls.clear()
        grads.grads_done(p)
        assert calls == [("remover", id(p))]
    finally:
        grads.remove_grad_ready_hook(remover)
        grads.remove_grad_ready_hook(victim)


def test_removing_an_unknown_hook_is_a_no_op():
    def never_registered(*a):
        raise AssertionError("called")
    grads.remove_grad_ready_hook(never_registered)
    grads.remove_backward_end_hook(never_registered)
    grads.grads_done(torch.nn.Parameter(torch.zeros(1)))


def test_arming_outside_a_backward_pass_leaves_the_join_unarmed(monkeypatch):
    # without a GPU arm_backward_join returns before it asks the engine; with this patch it goes
    # on to queue_callback, which raises RuntimeError outside a backward pass
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(grads, "current_stream", lambda: None)
    assert not grads.join_armed()
    grads.arm_backward_join()
    assert not grads.join_armed()
    grads.disarm_backward_join()
    grads.disarm_backward_join()
    assert not grads.join_armed()


def test_the_producer_attributes_are_named_in_grads_alone():
    files = []
    for top in ("dfu-multimodal_amd", "tools", "tests"):
        files += glob.glob(os.path.join(REPO, top, "**", "*.py"), recursive=True)
    assert len(files) >= 60
    skip = {os.path.join(PKG, "grads.py"), os.path.abspath(__file__)}
    found = []
    for path in sorted(set(files) - skip):
        with open(path) as f:
            text = f.read()
        found += [(os.path.relpath(path, REPO), name)
                  for name in ("_dfu_grad_stream", "_dfu_joins_itself") if name in text]
    assert not found, found


def _package_imports(path, modules):
    """The modules of dfu_hip that the file imports, at any nesting depth."""
    with open(path) as f:
        tree = ast.parse(f.read())
    out = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            if node.level == 1 and node.module is None:  # from . import ops, streams
                out |= {a.name for a in node.names}
            elif node.level == 1:  # from .streams import x / from .a.b import x
                out.add(node.module.split(".")[0])
            elif node.level == 0 and node.module == "dfu_hip":  # from dfu_hip import ops
                out |= {a.name for a in node.names}
            elif node.level == 0 and (node.module or "").startswith("dfu_hip."):
                out.add(node.module.split(".")[1])
        elif isinstance(node, ast.Import):  # import dfu_hip.ops as ops
            out |= {a.name.split(".")[1] for a in node.names if a.name.startswith("dfu_hip.")}
    return out & modules


def _cycle(graph):
    """One import cycle of `graph` as a list of module names, or None."""
    done, path = set(), []

    def visit(m):
        if m in path:
            return path[path.index(m):] + [m]
        if m in done:
            return None
        path.append(m)
        for n in sorted(graph[m]):
            c = visit(n)
            if c:
                return c
        path.pop()
        done.add(m)
        return None
    for m in sorted(graph):
        c = visit(m)
        if c:
            return c
    return None


def test_the_package_import_graph_is_acyclic_and_functional_is_on_top():
    paths = {os.path.splitext(os.path.basename(p))[0]: p
             for p in glob.glob(os.path.join(PKG, "*.py"))}
    paths.pop("__init__")
    modules = set(paths)
    assert {"functional", "grads", "graphs", "nn", "ops", "optim", "parallel",
            "streams"} <= modules
    graph = {m: _package_imports(p, modules) - {m} for m, p in paths.items()}
    assert graph["grads"] == {"ops", "streams"}
    assert _cycle(graph) is None, _cycle(graph)
    for m in ("optim", "parallel", "graphs", "grads"):
        assert "functional" not in graph[m], m


def test_the_cycle_search_sees_what_it_should():
    assert _cycle({"a": {"b"}, "b": {"c"}, "c": set()}) is None
    assert _cycle({"a": {"b"}, "b": {"c"}, "c": {"a"}}) == ["a", "b", "c", "a"]
    assert _cycle({"a": {"c"}, "b": {"c"}, "c": set(), "d": {"d"}}) == ["d", "d"]
