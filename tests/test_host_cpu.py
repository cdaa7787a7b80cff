"""Host-side checks that need no GPU: the C ABI library loads and exports every symbol
include/dfu_hip.h declares (the struct layouts: test_abi_cpu.py), argument validation fails
loudly, the GEMM planner's host logic, and the flat-parameter layout."""
import ctypes
import os

import pytest
import torch

from dfu_hip import _lib as L
from dfu_hip import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    lib = L.load()
    declared = L.header_symbols()
    assert len(declared) >= 40
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, f"declared in include/dfu_hip.h but not exported: {missing}"
    unbound = [s for s in declared if getattr(lib, s).argtypes != L.FUNCTIONS[s][1]]
    assert not unbound, f"loaded without the header's argument types: {unbound}"
    assert lib.dfu_version() >= 1


def _desc(**kw):
    d = L.GemmDesc()
    d.M, d.N, d.K = 256, 256, 256
    d.A = d.B = d.C = 1 << 20  # never dereferenced: validation fails before any launch
    d.lda = d.ldb = d.ldc = 256
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,msg", [
    (dict(M=0), "bad shape"),
    (dict(K=100), "multiple of 8"),
    (dict(tile=99), "bad tile"),
    (dict(split_k=4), "needs the F32_ACC"),
    (dict(lda=100), "lda"),
    (dict(epilogue=L.EPI_BF16_STATS), "stats slab"),
    (dict(a_mode=L.OPND_CONV_FWD, epilogue=L.EPI_BF16_STATS, stats=1 << 20, conv_n=1),
     "conv geometry"),
    (dict(A=(1 << 20) + 4), "16-byte aligned"),
])
def test_gemm_validation_errors(kw, msg):
    lib = L.load()
    d = _desc(**kw)
    rc = lib.dfu_gemm(ctypes.byref(d), None)
    assert rc == L.DFU_E_INVALID
    assert msg in lib.dfu_last_error_string().decode()
    with pytest.raises(L.DfuError):
        L.check(rc, "dfu_gemm")


@pytest.mark.parametrize("tile", [7, 8])
def test_gemm_phased_split_k_needs_a_workspace(tile):
    """Split-K without a workspace is the fp32-atomics path, which the phased tiles do not have:
    the descriptor is refused in launch(), before any kernel."""
    lib = L.load()
    d = _desc(a_mode=L.OPND_MNMAJOR, b_mode=L.OPND_MNMAJOR, epilogue=L.EPI_F32_ACC, split_k=2,
              tile=tile)
    assert lib.dfu_gemm_workspace_bytes(ctypes.byref(d)) == 2 * 256 * 256 * 4
    rc = lib.dfu_gemm(ctypes.byref(d), None)
    assert rc == L.DFU_E_INVALID
    assert "phased 256x256 tile needs a workspace" in lib.dfu_last_error_string().decode()


def test_x3_pairs_validation_and_plan():
    """Interleaved-pair bf16x3 descriptors (dfu_gemm_desc.x3_pairs): they need split-pair A with
    K = 2 a_seg, a_seg % 32 == 0; the planner picks one of the tiles that instantiate them."""
    lib = L.load()
    base = dict(epilogue=L.EPI_F32_STATS, stats=1 << 20, x3_pairs=1)
    d = _desc(**base)  # no a_seg
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_INVALID
    assert "x3_pairs" in lib.dfu_last_error_string().decode()
    d = _desc(a_seg=128, a_lo=(1 << 21), lda=128, **base)  # K = 256 = 2 a_seg: valid
    t, sk = ctypes.c_int32(), ctypes.c_int32()
    assert lib.dfu_gemm_plan(ctypes.byref(d), ctypes.byref(t), ctypes.byref(sk)) == 0
    assert t.value in (1, 2, 10, 11)
    d = _desc(a_seg=128, a_lo=(1 << 21), lda=128, K=384, **base)  # K = 3 a_seg: not pairs
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_INVALID
    assert "split-pair A" in lib.dfu_last_error_string().decode()
    d = _desc(a_seg=120, a_lo=(1 << 21), lda=120, K=240, **base)  # a_seg % 32 != 0
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_INVALID
    d = _desc(a_seg=128, a_lo=(1 << 21), lda=128, tile=8, **base)  # no persistent-tile pairs
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_UNSUPPORTED


def test_gemm_unsupported_combination():
    lib = L.load()
    d = _desc(epilogue=L.EPI_F32, tile=4)  # EPI_F32 is built for 128x128 only
    assert lib.dfu_gemm(ctypes.byref(d), None) == L.DFU_E_UNSUPPORTED


def test_gemm_planner_workspace():
    MN = L.OPND_MNMAJOR
    # ViT fc1 weight gradient at B=64: 36 output tiles of 256x256 for 256 CUs -> split-K slabs
    ws = ops.gemm_workspace_bytes(3072, 768, 64 * 197, MN, MN)
    assert ws > 0 and ws % (3072 * 768 * 4) == 0
    splits = ws // (3072 * 768 * 4)
    assert 2 <= splits <= 32
    # a forced split is honoured exactly
    assert ops.gemm_workspace_bytes(768, 768, 12608, MN, MN, split_k=8) == 8 * 768 * 768 * 4
    # no split -> no workspace; non-accumulating epilogues never need one
    assert ops.gemm_workspace_bytes(768, 768, 12608, MN, MN, split_k=1) == 0
    assert ops.gemm_workspace_bytes(12608, 768, 768, L.OPND_KMAJOR, L.OPND_KMAJOR,
                                    epilogue=L.EPI_BF16) == 0


def test_gemm_plans_match_snapshot_under_every_schedule():
    """Every case of tests/golden/gemm_plans.json (tools/gemm_plan_snapshot.py: recorded from the
    commit before the dispatch refactor, at the default schedule) plans to the recorded return
    code, tile, split-K and workspace bytes (with and without the tail split) -- under each
    dfu_gemm_set_persistent mode: the schedule switch does not reach the planner."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location(
        "gemm_plan_snapshot", os.path.join(REPO, "tools", "gemm_plan_snapshot.py"))
    snap = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(snap)
    with open(os.path.join(REPO, "tests", "golden", "gemm_plans.json")) as f:
        fix = json.load(f)
    assert (fix["linear"], fix["conv"], fix["result"]) == (snap.LINEAR, snap.CONV, snap.RESULT)
    nres = len(snap.RESULT)
    assert len(fix["cases"]) > 1500
    assert [tuple(c[:3]) for c in fix["cases"][-2:]] == snap.SCHEDULE_SENSITIVE
    lib = L.load()
    for mode in (0, 1, 2, 3):
        old = lib.dfu_gemm_set_persistent(mode)
        try:
            bad = [(c[:-nres], c[-nres:], got) for c in fix["cases"]
                   for got in [snap.answers(lib, c[:-nres])] if got != c[-nres:]]
        finally:
            lib.dfu_gemm_set_persistent(old)
        assert not bad, f"persistent mode {mode}: {len(bad)} plans moved (case, recorded, got), " \
                        f"first: {bad[:3]}"


@pytest.mark.parametrize("M,tiles", [(1, 1), (128, 1), (129, 2), (200704, 1568), (3136, 25)])
def test_stats_tiles_are_128_row_blocks(M, tiles):
    assert ops.stats_tiles(M) == tiles


def test_ops_reject_host_tensors():
    a = torch.zeros(128, 128, dtype=torch.bfloat16)
    c = torch.zeros(128, 128, dtype=torch.float32)
    with pytest.raises((ValueError, TypeError)):
        ops.gemm(128, 128, 128, a, 128, a, 128, c, 128, epilogue=L.EPI_F32)


def test_conv_geometry():
    g = ops.ConvGeom(64, 56, 56, 128, 128, 3, 3, 2, 1)
    assert (g.p, g.q) == (28, 28)
    g = ops.ConvGeom(64, 224, 224, 3, 64, 7, 7, 2, 3)
    assert (g.p, g.q) == (112, 112)


def test_flat_params_layout():
    from dfu_hip.optim import FlatParams
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (3, 8, 5, 1)]
    vals = [p.detach().clone() for p in ps]
    fp = FlatParams(ps)
    for p, v, o in zip(ps, vals, fp.offsets):
        # 128-byte aligned views: the vectorised kernels, and the x3 pair shadow's 32-element
        # blocks coincide with every parameter's (FlatParams.enable_x3)
        assert o % 32 == 0
        assert torch.equal(p.data, v)
        assert p.data.data_ptr() == fp.data.data_ptr() + 4 * o
        assert p.grad.data_ptr() == fp.grad.data_ptr() + 4 * o
    assert fp.numel == 4 * 32


def test_flat_params_store_spatial_conv_weights_krsc():
    """Spatial conv weights live channels-last (KRSC) in the flat buffers with their OIHW shape
    and values; 1x1 and 3-channel (stem) weights and everything else keep the plain order; the
    optimizer's state_dict moments read back in parameter order."""
    from dfu_hip.optim import FlatParams
    w3 = torch.nn.Parameter(torch.randn(16, 8, 3, 3))
    w1 = torch.nn.Parameter(torch.randn(16, 8, 1, 1))
    stem = torch.nn.Parameter(torch.randn(4, 3, 7, 7))
    lin = torch.nn.Parameter(torch.randn(5, 7))
    vals = [p.detach().clone() for p in (w3, w1, stem, lin)]
    fp = FlatParams([w3, w1, stem, lin])
    assert fp.krsc == [True, False, False, False]
    for p, v in zip((w3, w1, stem, lin), vals):
        assert torch.equal(p.detach(), v)
    o = fp.offsets[0]
    krsc = fp.data[o:o + w3.numel()].view(16, 3, 3, 8)
    assert torch.equal(krsc, vals[0].permute(0, 2, 3, 1))
    assert w3.is_contiguous(memory_format=torch.channels_last) and not w3.is_contiguous()
    assert w3.grad.stride() == w3.stride() and w3.grad.data_ptr() == fp.grad.data_ptr() + 4 * o
    assert fp.grad_view(0).stride() == w3.stride()
    # a gradient written through the parameter-shaped view lands in KRSC order
    g = torch.randn(16, 8, 3, 3)
    w3.grad.copy_(g)
    assert torch.equal(fp.grad[o:o + w3.numel()].view(16, 3, 3, 8), g.permute(0, 2, 3, 1))
    # FusedAdamW.state_dict's moments are these views of its flat moment buffers
    m = torch.zeros_like(fp.data)
    m[o:o + w3.numel()] = torch.arange(w3.numel(), dtype=torch.float32)
    v = fp.view(m, 0)
    assert v.shape == w3.shape and torch.equal(v.permute(0, 2, 3, 1).reshape(-1),
                                               torch.arange(w3.numel(), dtype=torch.float32))


def test_gradcam_target_layer_rule():
    """grad_cam_visualization.py:389-392: the target is the LAST module name containing the
    target string — the block output ReLU of layer4 and the ViT's last drop_path2 (a 3-D token
    tensor, hence the input-saliency fallback); both are called by our forward when hooked."""
    from models.fusion import MultimodalFusionModel
    from models.gradcam import GradCAM
    m = MultimodalFusionModel()
    rc, tc = GradCAM(m.resnet, ["layer4"]), GradCAM(m.vit, ["blocks"])
    assert rc.target_name() == "layer4.2.relu"
    assert tc.target_name() == "blocks.11.drop_path2"
    assert len(rc.handles) > 0 and len(tc.handles) > 0
    rc.remove()
    tc.remove()
    assert not m.resnet.layer4[-1].relu._forward_hooks


def test_fusion_head_hidden_dims_list_or_tuple():
    """the head depends on the hidden widths, not on the container type; None picks
    each layout's reference head (eval 2816->512->2, train 2816->512->256->2)."""
    from models.fusion import MultimodalFusionModel
    from dfu_hip import nn as hnn
    widths = lambda m: [l.out_features for l in m.fusion.modules() if isinstance(l, hnn.Linear)]  # noqa: E731,E741
    for layout, ref in (("eval", [512, 2]), ("train", [512, 256, 2])):
        assert widths(MultimodalFusionModel(layout=layout)) == ref
        assert widths(MultimodalFusionModel(layout=layout, hidden_dims=[512])) == [512, 2]
        assert widths(MultimodalFusionModel(layout=layout, hidden_dims=(512,))) == [512, 2]
    keys = [k for k in MultimodalFusionModel(layout="train").state_dict() if k.startswith("fusion")]
    assert keys == ["fusion.0.weight", "fusion.0.bias", "fusion.3.weight", "fusion.3.bias",
                    "fusion.6.weight", "fusion.6.bias"]


def test_default_precision_is_the_parity_mode():
    """The drop-in surface meets north_star's bar without any precision call (VERDICT round 4
    item 1): the library default is "parity", as INTEGRATION.md §1 states."""
    from dfu_hip import functional as Fn
    assert Fn.DEFAULT_PRECISION == "parity" and Fn.get_precision() == "parity"
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "INTEGRATION.md")).read()
    assert '"parity" (the default' in doc
    with Fn.precision("bf16"):
        assert Fn.get_precision() == "bf16"
    assert Fn.get_precision() == "parity"


def test_vit_parity_policy_safe_by_construction():
    """a ViT runs Blocks 0-8 bf16x3 in the parity mode unless a fusion
    model marks it as its feature extractor -- whichever object holds the head (ViT head,
    Identity head + a caller's Linear, ThermalViTEncoder).  Only the policy's own attributes
    are rewritten."""
    from dfu_hip import functional as Fn
    from models import encoders
    from models import models as M
    from models import precision as P
    from models.fusion import MultimodalFusionModel
    safe = ["bf16x3"] * 9 + ["fp16"] * 3

    def modes(v):
        v._parity_policy()
        return [Fn.stage_mode(b) for b in v.blocks]

    assert modes(encoders.create_model("vit_base_patch16_224", num_classes=2)) == safe
    assert modes(encoders.create_model("vit_base_patch16_224", num_classes=0)) == safe
    assert modes(M.ThermalViTEncoder().vit) == safe
    for layout in ("eval", "train"):
        m = MultimodalFusionModel(layout=layout)
        _, v = P.encoders(m)
        assert v.dfu_feature_extractor and modes(v) == ["fp16"] * 12
    v = encoders.create_model("vit_base_patch16_224", num_classes=0)
    P.mark_feature_extractor(v)
    assert modes(v) == ["fp16"] * 12
    v.blocks[3].dfu_parity_precision = "bf16x3"  # a user's per-instance override
    P.mark_feature_extractor(v, on=False)
    assert modes(v) == safe
    P.mark_feature_extractor(v)
    assert modes(v)[3] == "bf16x3" and modes(v).count("fp16") == 11
    from models.resnet import ResNet
    with pytest.raises(ValueError):
        P.mark_feature_extractor(ResNet())
