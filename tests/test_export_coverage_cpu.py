"""Every function include/dfu_hip.h exports is named by some GPU test: by its own name, or
through a dfu_hip.ops wrapper that calls it (`ops.<wrapper>(` / PartialReductions), or it is on
the short allow-list below of exports that launch no kernel.  A new kernel entry point without
a direct test, or the deletion of the only test of an old one, fails here (no GPU needed)."""
import ast
import glob
import os
import re

from dfu_hip import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the modules that bind the library, and the names GPU tests know them by
BINDINGS = [
    (os.path.join(REPO, "dfu-multimodal_amd", "dfu_hip", "ops.py"), "ops"),
    (os.path.join(REPO, "dfu-multimodal_amd", "data", "gpu_transforms.py"), "GT"),
]

# Exports that launch no kernel, with the reason none of them needs a numerical GPU test.
ALLOWED = {
    "dfu_last_error_string": "returns the host-side message of the last failed call",
    "dfu_version": "a constant; checked by test_host_cpu.py",
    "dfu_stream_create": "host-side hipStreamCreate; used by every two-stream GPU test",
    "dfu_stream_destroy": "host-side hipStreamDestroy",
    "dfu_stream_capture_status": "host-side hipStreamIsCapturing query (dfu_hip.graphs)",
    "dfu_streams_abort_capture": "host-side capture recovery (dfu_hip.graphs.try_capture)",
    "dfu_resize_ksize": "host-only arithmetic; checked by test_augment_cpu.py",
    "dfu_resize_coeffs": "host-only arithmetic; checked by test_augment_cpu.py",
    "dfu_gemm_plan": "the host-side planner; checked against a snapshot by test_host_cpu.py",
}


def _wrappers():
    """"<alias>.<function or class>" of every binding module -> the set of dfu_* exports its
    body calls through the library (`lib().dfu_x`, or `lb.dfu_x` on a local alias of it)."""
    out = {}
    for path, alias in BINDINGS:
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in tree.body:
            if not isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                continue
            names = {n.attr for n in ast.walk(node)
                     if isinstance(n, ast.Attribute) and n.attr.startswith("dfu_")}
            if names:
                out[f"{alias}.{node.name}"] = names
    return out


def _gpu_test_text():
    files = sorted(glob.glob(os.path.join(REPO, "tests", "test_*_gpu.py")))
    assert len(files) >= 10
    text = []
    for p in files:
        with open(p) as f:
            text.append(f.read())
    return "\n".join(text)


def _uncovered(text, wrappers, exports):
    used = {w for w in wrappers
            if re.search(r"\b" + re.escape(w) + r"\(", text) or
            (w == "ops.PartialReductions" and "PartialReductions" in text)}
    via = set().union(*[wrappers[w] for w in used]) if used else set()
    return sorted(e for e in exports
                  if e not in ALLOWED and e not in via and not re.search(r"\b" + e + r"\b", text))


def test_every_export_is_named_by_a_gpu_test():
    exports = L.header_symbols()
    assert len(exports) >= 89
    wrappers = _wrappers()
    assert "dfu_gemm_f32" in wrappers["ops.gemm_f32"]
    assert "dfu_colsum" in wrappers["ops.colsum_partial"]
    assert "dfu_reduce_partials_batch" in wrappers["ops.PartialReductions"]
    assert "dfu_gather_rows_f32" in wrappers["ops.concat2_f32"]
    assert "dfu_resize_batch" in wrappers["GT.GpuPreprocessor"]
    missing = _uncovered(_gpu_test_text(), wrappers, exports)
    assert not missing, f"exports no GPU test names, directly or through an ops wrapper: {missing}"


def test_allow_list_is_short_and_launches_nothing():
    exports = set(L.header_symbols())
    assert set(ALLOWED) <= exports, sorted(set(ALLOWED) - exports)
    assert len(ALLOWED) <= 9 and all(len(r) > 10 for r in ALLOWED.values())
    # an allow-listed export's definition holds no kernel launch
    csrc = os.path.join(REPO, "dfu-multimodal_amd", "csrc")
    for name in ALLOWED:
        body = None
        for p in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")):
            with open(p) as f:
                src = f.read()
            m = re.search(r'extern "C"[^;{]*\b' + name + r"\s*\([^)]*\)\s*\{", src)
            if m:
                depth, i = 1, m.end()
                while depth:
                    depth += {"{": 1, "}": -1}.get(src[i], 0)
                    i += 1
                body = src[m.end():i]
        assert body is not None, f"{name}: definition not found"
        assert not any(k in body for k in ("hipLaunchKernelGGL", "LAUNCH(", "<<<")), name


def test_the_check_notices_a_deleted_test():
    """Without the GPU tests of the ViT embedding backward, the export is reported."""
    text = re.sub(r"vit_embed_bwd", "x", _gpu_test_text())
    assert "dfu_vit_embed_bwd" in _uncovered(text, _wrappers(), L.header_symbols())
