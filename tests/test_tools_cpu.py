"""tools/ without a GPU: every tool imports without doing work, kernel_time.py's case table
declares the shapes and the algorithmic bytes / FLOPs the former per-kernel scripts stated, the
shared pieces live in tools/_harness.py alone, and the shell runners parse."""
import ast
import glob
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
CASES = ["adamw", "attn", "bn_apply", "bn_apply_x3", "bn_bwd", "colsum", "ln_fwd", "ln_bwd", "pool",
         "stem", "t1x1", "dgrad_strided", "epi"]

IMPORT_ALL = """
import glob, importlib.util, os, sys
tools = sys.argv[1]
sys.path.insert(0, tools)
import torch
for path in sorted(glob.glob(os.path.join(tools, "*.py"))):
    name = os.path.basename(path)[:-3]
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules.setdefault(name, mod)
    spec.loader.exec_module(mod)
    assert not torch.cuda.is_initialized(), name
    print("imported", name)
"""


def _kernel_time(*args):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "kernel_time.py"), *args],
                       capture_output=True, text=True, env=NO_GPU, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_every_tool_imports_without_a_gpu_and_does_no_work():
    r = subprocess.run([sys.executable, "-c", IMPORT_ALL, TOOLS], capture_output=True, text=True,
                       env=NO_GPU, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    files = glob.glob(os.path.join(TOOLS, "*.py"))
    lines = r.stdout.splitlines()
    assert len(files) >= 30
    assert lines == [f"imported {os.path.basename(p)[:-3]}" for p in sorted(files)]  # no output


def test_kernel_time_lists_the_thirteen_cases():
    assert _kernel_time("--list") == CASES


def _expected_plan(B):
    """The former scripts' shapes and closed formulas, per case: [(text in the shape, work)]."""
    bn_apply = [(B * 112 * 112, 64, 0), (B * 56 * 56, 64, 0), (B * 56 * 56, 256, 1),
                (B * 28 * 28, 512, 1), (B * 14 * 14, 1024, 1), (B * 7 * 7, 2048, 1)]
    bn_x3 = [(B * 56 * 56, 64, 0), (B * 56 * 56, 256, 1), (B * 28 * 28, 128, 0),
             (B * 28 * 28, 512, 1), (B * 14 * 14, 256, 0), (B * 14 * 14, 1024, 1),
             (B * 7 * 7, 512, 0), (B * 7 * 7, 2048, 1)]
    bn_bwd = [(B * 112 * 112, 64, 2, 0), (B * 56 * 56, 64, 2, 0), (B * 56 * 56, 256, 1, 1),
              (B * 28 * 28, 128, 2, 0), (B * 28 * 28, 512, 1, 1), (B * 14 * 14, 256, 2, 0),
              (B * 14 * 14, 1024, 1, 1), (B * 7 * 7, 512, 2, 0), (B * 7 * 7, 2048, 1, 1)]
    rows, D, n = B * 197, 768, 110_750_000
    attn = 4 * 197 * 197 * 64 * B * 12
    return {
        "adamw": [(f"n={n}", 30 * n)],
        "attn": [(f"B={B} N=197 H=12 dh=64", attn), (f"B={B} N=197 H=12 dh=64", 2.5 * attn)],
        "bn_apply": [(f"M={M} C={C} ", M * C * 2 * (3 if res else 2)) for M, C, res in bn_apply],
        "bn_apply_x3": [(f"M={M} C={C} ", M * C * ((8 if res else 4) + 4 + 0.125))
                        for M, C, res in bn_x3],
        "bn_bwd": [(f"M={M} C={C} relu={relu}", M * C * 2 * (2 * (3 if relu == 1 else 2) + 1 + res))
                   for M, C, relu, res in bn_bwd],
        "colsum": [(f"rows={rows} N={N}", 2 * rows * N) for N in (768, 2304, 3072)],
        "ln_fwd": [(f"rows={rows} D={D}", 6 * D * rows)],
        "ln_bwd": [(f"rows={rows} D={D}", 16 * D * rows)],
        "pool": [(f"{B}x112x112x64", B * 112 * 112 * 64 * 2 + B * 56 * 56 * 64 * 3)],
        "stem": [(f"{B * 112 * 112}x64x147", 2 * B * 112 * 112 * 64 * 147)],
        "t1x1": [(f"{B * 56 * 56}x64x{K}", 2 * B * 56 * 56 * 64 * K) for K in (64, 256, 256)],
        "dgrad_strided": [(f"{B * H * H}x{C}x{9 * C}", 2 * B * H * H * C * 9 * C / 4)
                          for H, C in ((56, 128), (28, 256), (14, 512))],
        "epi": [(f"{rows}x3072x768", 2 * rows * 3072 * 768)],
    }


def test_kernel_time_plans_state_the_former_scripts_shapes_and_formulas():
    for B in (64, 2):
        got = {}
        for line in _kernel_time("--plan", "--batch", str(B)):
            m = re.fullmatch(r"(\w+) (.+): (\d+) (B|FLOP)", line)
            assert m, line
            got.setdefault(m.group(1), []).append((m.group(2), int(m.group(3))))
        want = _expected_plan(B)
        assert list(got) == CASES
        for case in CASES:
            assert len(got[case]) == len(want[case]), case
            for (shape, work), (text, exp) in zip(got[case], want[case]):
                assert text in shape and work == exp, (case, B, shape, work, text, exp)


def _calls_and_keywords(path):
    tree = ast.parse(open(path).read(), path)
    names, timed = set(), False
    for node in ast.walk(tree):
        if isinstance(node, ast.Call):
            f = node.func
            names.add(f.id if isinstance(f, ast.Name) else getattr(f, "attr", None))
            timed |= any(k.arg == "enable_timing" and getattr(k.value, "value", None) is True
                         for k in node.keywords)
    return names, timed


def test_the_step_and_the_event_window_live_in_the_harness():
    adamw, events = [], []
    for path in sorted(glob.glob(os.path.join(TOOLS, "**", "*.py"), recursive=True)):
        names, timed = _calls_and_keywords(path)
        rel = os.path.relpath(path, TOOLS)
        if "FusedAdamW" in names:
            adamw.append(rel)
        if timed:
            events.append(rel)
    assert adamw == ["_harness.py"]
    assert events == ["_harness.py", "head_time.py", "host_step_time.py", "step_timeline.py"]


def test_shell_runners_parse_and_carry_no_default_round_tag():
    scripts = sorted(glob.glob(os.path.join(TOOLS, "*.sh")))
    assert {"ab.sh", "profile.sh", "measure.sh"} <= {os.path.basename(s) for s in scripts}
    for s in scripts:
        r = subprocess.run(["bash", "-n", s], capture_output=True, text=True)
        assert r.returncode == 0, (s, r.stderr)
        assert not re.search(r":-r[0-9]", open(s).read()), s
