"""What every measurement tool shares: the import path, the one HIP-event window, the benchmark's
training step and the GEMM descriptor helpers.  Every tool starts with `import _harness`.
Nothing here touches the GPU at import."""
import collections
import ctypes
import os
import sys

# torch before anything loads libdfu_hip.so: the library then binds to the HIP runtime torch
# ships; loaded first it brings in the system's copy and runs beside torch's on a second runtime
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dfu-multimodal_amd")
for _p in (PKG, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def lib_tag():
    """The library a run timed, as the tools' result lines end: lib=<DFU_HIP_LIB or in-tree>."""
    return os.environ.get("DFU_HIP_LIB", "in-tree")


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a GPU (torch.cuda.is_available() is false); "
                           "HIP events are the only clock, there is no host-clock fallback")


def time_us(fn, iters, warmup, sync=True):
    """Mean microseconds per call of fn: `warmup` calls, synchronise, event, `iters` calls, event,
    synchronise.  sync=False leaves the first synchronise out, as the tools did whose window
    opened behind their queued warm-up calls: the device then does not wait for the window's
    first launch (with it, dgrad_strided's 60-130 us launches read 0.5 us longer at 20 calls)."""
    require_gpu()
    for _ in range(warmup):
        fn()
    if sync:
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


Step = collections.namedtuple("Step", "model fwd opt crit inputs step")


def fusion_step(config="fusion", batch=64, precision=None, seed=42, *, model=None, inputs=None):
    """The benchmark's training step: bench.py's model and synthetic batch, FusedAdamW and the
    class-weighted loss.  Returns the parts (model, fwd, opt, crit, inputs = (rgb, thermal, y))
    and step(), one whole step.  `model` / `inputs`: a study's own fusion model or batch."""
    import bench
    from dfu_hip import functional as Fn
    from dfu_hip import nn as hnn
    from dfu_hip.optim import FusedAdamW
    require_gpu()
    dev = torch.device("cuda", 0)
    if precision:
        Fn.set_precision(precision)
    if model is None:
        torch.manual_seed(seed)
        model, fwd = bench.build(config, dev)
    else:
        fwd = lambda m, r, t: m(r, t)  # noqa: E731
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    crit = hnn.CrossEntropyLoss(weight=torch.tensor([2.0, 2.0], device=dev))
    rgb, th, y = inputs or bench.synthetic(batch, dev, seed=seed)

    def step():
        opt.zero_grad()
        crit(fwd(model, rgb, th), y).backward()
        Fn.join_grad_streams()
        opt.step()
    return Step(model, fwd, opt, crit, (rgb, th, y), step)


def record_step_gemms(s, precision):
    """Every dfu_gemm launch of one step of `s` (a fusion_step) with forward and backward in
    `precision`: ops.gemm_record's (descriptor, flops, bytes, refs, _) entries."""
    from dfu_hip import functional as Fn
    from dfu_hip import ops
    ops.gemm_record = []
    s.opt.zero_grad()
    with Fn.precision(precision):
        s.crit(s.fwd(s.model, *s.inputs[:2]), s.inputs[2]).backward()
    s.opt.step()
    rec, ops.gemm_record = ops.gemm_record, None
    torch.cuda.synchronize()
    return rec


# ---- GEMM descriptors -------------------------------------------------------------------------
# (short, long) name per operand mode and epilogue id: the short ones in gemm_step_profile.py's
# table, the long ones (the header's, without DFU_OPND_ / DFU_EPI_) in gemm_tune.py's entries
OPND_NAMES = [("KM", "KM"), ("MN", "MN"), ("CFWD", "CONV_FWD"), ("CDGD", "CONV_DGRAD"),
              ("CDGW", "CONV_DGRAD_W"), ("CWGX", "CONV_WGRAD_X")]
EPI_NAMES = [("BF16", "BF16"), ("RELU", "BF16_RELU"), ("GELU", "BF16_GELU"), ("F32", "F32"),
             ("RESID", "F32_RESID"), ("DGELU", "BF16_DGELU"), ("ADD", "BF16_ADD"),
             ("ACC", "F32_ACC"), ("ACCW", "F32_ACC_CONVW"), ("STATS", "BF16_STATS"),
             ("PATCH", "PATCH"), ("F32STATS", "F32_STATS"), ("DSTATS", "BF16_DSTATS"),
             ("X3GELU", "X3_GELU"), ("F16DUAL", "F16_DUAL"), ("F16GELU", "F16_GELU")]
CONV_FIELDS = ("conv_n", "conv_h", "conv_w", "conv_c", "conv_k", "conv_r", "conv_s",
               "conv_stride", "conv_pad")

# the ViT-B/16 GEMMs of the B = 64 step (64 x 197 = 12608 token rows): name -> (M, N, K) of the
# forward; the input gradient is M x K x N, the weight gradient N x K x M
VIT_ROWS = 64 * 197
VIT_SHAPES = {"qkv": (VIT_ROWS, 2304, 768), "proj": (VIT_ROWS, 768, 768),
              "fc1": (VIT_ROWS, 3072, 768), "fc2": (VIT_ROWS, 768, 3072)}


def gemm_label(d, long=False):
    """'<A>x<B>-><epilogue>' of a descriptor in the short or the long names."""
    i = int(long)
    return f"{OPND_NAMES[d.a_mode][i]}x{OPND_NAMES[d.b_mode][i]}->{EPI_NAMES[d.epilogue][i]}"


def gemm_key(d):
    """What makes two recorded launches the same GEMM."""
    return (d.a_mode, d.b_mode, d.epilogue, d.M, d.N, d.K) + tuple(
        getattr(d, f) for f in CONV_FIELDS) + (d.operand_type,)


def copy_desc(d):
    from dfu_hip import _lib as L
    n = L.GemmDesc()
    ctypes.memmove(ctypes.byref(n), ctypes.byref(d), ctypes.sizeof(d))
    return n


def time_desc(d, iters, ws=None):
    """Mean us of one descriptor's launch, back to back (2 checked warm-up launches).  `ws`, a
    one-element list holding a uint8 device tensor: give the descriptor its own workspace (grown
    in place when too small) and hand-off counters, for a descriptor whose plan was changed."""
    from dfu_hip import ops
    lib = ops.lib()
    if ws is not None:
        need = lib.dfu_gemm_workspace_bytes(ctypes.byref(d))
        if need > ws[0].numel():
            ws[0] = torch.empty(need, dtype=torch.uint8, device="cuda")
        d.workspace = ws[0].data_ptr() if need > 0 else None
        d.workspace_bytes = int(need)
        cnt = ops.tile_counters(torch.device("cuda", 0))  # split-K / tail-split hand-off counters
        d.tile_counters, d.tile_counters_len = cnt.data_ptr(), cnt.numel()
    s = ops.stream_ptr()
    for _ in range(2):
        ops.check(lib.dfu_gemm(ctypes.byref(d), s), "dfu_gemm")
    return time_us(lambda: lib.dfu_gemm(ctypes.byref(d), s), iters, 0, sync=False)
