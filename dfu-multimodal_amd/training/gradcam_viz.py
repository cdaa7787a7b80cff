"""The reference's Grad-CAM visualisation pass (notebooks/grad_cam_visualization.py:432-859) on
the HIP modules, shaped for a GPU.

Reference loop shape (three copies of one loop, :712-741, :766-793, :818-846), one test sample
at a time, the first 5 healthy and the first 5 ulcer samples of each test set:
  forward under no_grad -> softmax -> argmax, confidence               (:471-475)
  GradCAM(...).generate_cam: a second forward and a backward           (:478-479, :575-580)
  image .cpu().numpy(), min-max scaled on the host, * 255 -> uint8     (:485-487)
  cv2.resize of the map, * 255 -> uint8, cv2.applyColorMap(JET), cv2.addWeighted   (:432-462)
  a matplotlib figure, saved as {healthy|ulcer}_{count:02d}.png        (:493-510, :729-735)

Here each model makes one pass over its (up to) ten samples: one batched forward for prediction
and confidence, one batched GradCAM.generate_cams per encoder, dfu_image_minmax and
dfu_cam_overlay (ops.cam_overlay) for the three pictures of every sample of a modality, and one
device -> host read (evalpass.read_once).  OpenCV is not available to this project: the pixel
arithmetic is the definition in include/dfu_hip.h, restated from OpenCV's documented behaviour,
and its agreement with cv2 is unverified (tests pin the kernel to a numpy restatement of that
definition).  The default colour table (ops.jet_lut) has the ends of OpenCV's JET and may differ
from it by a level or two in between; ops.cam_overlay takes a caller's table.

Single process only: the pass is not sharded over data-parallel ranks.
"""
import os

import numpy as np
import torch

from dfu_hip import ops
from dfu_hip.ops import jet_lut, linear_taps  # noqa: F401  (part of this module's surface)
from models.gradcam import GradCAM

from .evalpass import read_once

KINDS = ("rgb_only", "thermal_only", "multimodal")
CLASS_NAMES = ("healthy", "ulcer")  # label 0, 1: the file names
PRED_NAMES = ("Healthy", "Ulcer")   # the titles
_PICTURES = ("image", "heatmap", "overlay")


def overlay_gradcam_on_image(image_np, cam, alpha=0.5):
    """grad_cam_visualization.py:432 overlay_gradcam_on_image: image (H, W, 3), uint8 or float
    in [0, 1] / [0, 255]; cam (h, w) in [0, 1].  Returns (overlay, heatmap), uint8 (H, W, 3)
    numpy arrays, computed on the device by ops.cam_overlay.  The uint8 coercion is the script's
    (:445-449), on the host; the image enters the blend as given (it is not min-max scaled
    again)."""
    image_np = np.asarray(image_np)
    if image_np.dtype != np.uint8:
        if image_np.max() <= 1.0:
            image_np = (image_np * 255).astype(np.uint8)
        else:
            image_np = image_np.astype(np.uint8)
    if image_np.ndim != 3 or image_np.shape[2] != 3:
        raise ValueError(f"image is (H, W, 3), got {image_np.shape}")
    dev = torch.device("cuda")
    # the kernel's image is trunc(((x - min) / (max - min)) * 255): with (min, max) = (0, 255)
    # and x = u + 0.5 that is u for every uint8 u (the two roundings move u + 0.5 by < 1e-4)
    x = torch.from_numpy(image_np.transpose(2, 0, 1)[None].astype(np.float32) + np.float32(0.5))
    minmax = torch.tensor([[0.0, 255.0]], dtype=torch.float32)
    cam_t = torch.from_numpy(np.ascontiguousarray(cam, dtype=np.float32)[None])
    _, heatmap, overlay = ops.cam_overlay(x.to(dev), cam_t.to(dev), alpha=alpha,
                                          minmax=minmax.to(dev))
    both = torch.stack([overlay[0], heatmap[0]]).cpu().numpy()
    return both[0], both[1]


def select_samples(labels, num_healthy=5, num_ulcer=5):
    """The samples the script's loop visualises (:712-741): the first num_healthy of label 0 and
    the first num_ulcer of the other label, in dataset order.  Returns [(index, label, count)],
    count the sample's number within its class (the file name's).  Needs no image."""
    taken, want, out = [0, 0], (num_healthy, num_ulcer), []
    for index, label in enumerate(labels):
        if taken[0] >= want[0] and taken[1] >= want[1]:
            break
        cls = 0 if int(label) == 0 else 1
        if taken[cls] >= want[cls]:
            continue
        out.append((index, cls, taken[cls]))
        taken[cls] += 1
    return out


def visualize_batch(model, kind, rgb=None, thermal=None):
    """visualize_rgb_only / visualize_thermal_only / visualize_multimodal (:465-632) up to the
    figure, for a batch: `kind` in KINDS, `rgb` / `thermal` the normalised fp32 [B, 3, H, W]
    inputs on the device that the kind takes.  The model runs in eval mode; prediction and
    confidence come from one no_grad forward (softmax -> argmax, the predicted class's
    probability); the maps from GradCAM(model, ['layer4']) (RGB-only), GradCAM(model.vit,
    ['blocks']) (thermal-only), or GradCAM(model.resnet, ['layer4']) and GradCAM(model.vit,
    ['blocks']) on their own inputs (fusion), one generate_cams call each, the hooks removed
    afterwards; the pictures from one ops.cam_overlay call per modality.  Returns one host dict
    of numpy arrays, read from the device once: 'prediction' int64 [B], 'confidence' fp32 [B],
    and 'cam', 'image', 'heatmap', 'overlay' (fusion: each with '_rgb' and '_thermal')."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    need = {"rgb_only": (rgb,), "thermal_only": (thermal,), "multimodal": (rgb, thermal)}[kind]
    if any(t is None for t in need):
        raise ValueError(f"{kind}: missing input")
    if kind == "thermal_only" and not hasattr(model, "vit"):
        raise ValueError("thermal_only: the model needs its encoder as .vit "
                         "(ThermalOnlyModel(layout='eval'))")
    model.eval()
    with torch.no_grad():
        probs = torch.softmax(model(*need).float(), dim=1)
        prediction = torch.argmax(probs, dim=1)
        confidence = probs.gather(1, prediction[:, None])[:, 0]
    if kind == "rgb_only":
        jobs = [("", GradCAM(model, ["layer4"]), rgb)]
    elif kind == "thermal_only":
        jobs = [("", GradCAM(model.vit, ["blocks"]), thermal)]
    else:
        jobs = [("_rgb", GradCAM(model.resnet, ["layer4"]), rgb),
                ("_thermal", GradCAM(model.vit, ["blocks"]), thermal)]
    named = [("prediction", prediction), ("confidence", confidence)]
    try:
        for suffix, grad_cam, x in jobs:
            cams = grad_cam.generate_cams(x)
            if cams is None:
                raise RuntimeError(f"Could not find layer {grad_cam.target_layers}")
            named.append(("cam" + suffix, cams))
            pictures = ops.cam_overlay(x.detach().float(), cams)
            named += [(name + suffix, p) for name, p in zip(_PICTURES, pictures)]
    finally:
        for _, grad_cam, _ in jobs:
            grad_cam.remove()
    return read_once(named)


def sample_at(batch, i):
    """Sample i of a visualize_batch dict, as the figure functions take it."""
    out = {k: v[i] for k, v in batch.items()}
    out["prediction"], out["confidence"] = int(out["prediction"]), float(out["confidence"])
    return out


# ------------------------------------------------------------------------------- figures
def _subplots(rows, cols, figsize):
    """(Figure, axes) on an Agg canvas of its own: matplotlib's object API, so no pyplot state
    and no global backend is touched (as training.metrics)."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError as e:
        raise ImportError("the figures of training.gradcam_viz need the matplotlib package, "
                          "which is not installed (visualize_batch does not need it)") from e
    fig = Figure(figsize=figsize)
    FigureCanvasAgg(fig)
    return fig, fig.subplots(rows, cols)


def _show(ax, picture, title, gray=False):
    ax.imshow(picture, cmap="gray") if gray else ax.imshow(picture)
    ax.set_title(title)
    ax.axis("off")


def _single_figure(sample, original_title, suptitle, gray):
    fig, axes = _subplots(1, 3, (15, 5))
    pred, conf = sample["prediction"], sample["confidence"]
    _show(axes[0], sample["image"], original_title, gray)
    _show(axes[1], sample["heatmap"], "Grad-CAM Heatmap")
    _show(axes[2], sample["overlay"], f"Overlay\nPred: {PRED_NAMES[pred == 1]} ({conf:.3f})")
    fig.suptitle(suptitle, fontsize=14, fontweight="bold")
    fig.tight_layout()
    return fig


def figure_rgb_only(sample):
    """The figure of visualize_rgb_only (:493-510) from one sample (sample_at)."""
    return _single_figure(sample, "Original RGB Image", "RGB-Only Model Grad-CAM", False)


def figure_thermal_only(sample):
    """The figure of visualize_thermal_only (:541-558)."""
    return _single_figure(sample, "Original Thermal Image", "Thermal-Only Model Grad-CAM", True)


def figure_multimodal(sample):
    """The figure of visualize_multimodal (:599-632): the RGB row above the thermal row."""
    fig, axes = _subplots(2, 3, (18, 10))
    for row, (suffix, name, gray) in enumerate((("_rgb", "RGB", False),
                                                ("_thermal", "Thermal", True))):
        _show(axes[row, 0], sample["image" + suffix], f"{name} Image", gray)
        _show(axes[row, 1], sample["heatmap" + suffix], f"{name} Grad-CAM")
        _show(axes[row, 2], sample["overlay" + suffix], f"{name} Overlay")
    pred_text = PRED_NAMES[sample["prediction"] == 1]
    fig.suptitle(f"Multimodal Fusion Grad-CAM\nPrediction: {pred_text} "
                 f"(Confidence: {sample['confidence']:.3f})", fontsize=14, fontweight="bold")
    fig.tight_layout()
    return fig


FIGURES = {"rgb_only": figure_rgb_only, "thermal_only": figure_thermal_only,
           "multimodal": figure_multimodal}


# ---------------------------------------------------------------------------------- main
_BANNERS = {"rgb_only": ("🔴 ", "VISUALIZING RGB-ONLY MODEL", "RGB-only"),
            "thermal_only": ("🔵 ", "VISUALIZING THERMAL-ONLY MODEL", "Thermal-only"),
            "multimodal": ("🟣 ", "VISUALIZING MULTIMODAL FUSION MODEL", "Multimodal")}


def _build_model(kind):
    """The script's model of a kind (:257-320): the encoders as .resnet / .vit."""
    from models.fusion import MultimodalFusionModel
    from models.single import RGBOnlyModel, ThermalOnlyModel
    if kind == "rgb_only":
        return RGBOnlyModel(layout="eval")
    if kind == "thermal_only":
        return ThermalOnlyModel(layout="eval")
    return MultimodalFusionModel()


def _labels(dataset):
    labels = dataset.labels
    return list(labels() if callable(labels) else labels)


def load_samples(dataset, kind, indices, device="cuda"):
    """Samples `indices` of a test set, decoded and preprocessed as the script's transforms do
    (:650-660: Resize((224, 224)), ToTensor, Normalize with the ImageNet / 0.5 statistics)
    through data.gpu_transforms' loaders, as one batch: (rgb, thermal) fp32 [B, 3, 224, 224] on
    the device, None for a modality the kind does not take."""
    from data import gpu_transforms as GT
    if kind == "multimodal":
        loader = GT.GpuPairLoader(dataset, len(indices), sampler=list(indices), device=device)
        rgb, thermal, _ = next(iter(loader))
        return rgb, thermal
    spec = GT.rgb_val_test_transform if kind == "rgb_only" else GT.thermal_val_test_transform
    loader = GT.GpuImageLoader(dataset, len(indices), sampler=list(indices), spec=spec,
                               device=device)
    images, _ = next(iter(loader))
    return (images, None) if kind == "rgb_only" else (None, images)


def run_gradcam_visualization(models, datasets, output_dir, num_healthy=5, num_ulcer=5,
                              device="cuda"):
    """The script's main (:639-855) without its hard-coded paths.  `models` maps a kind (KINDS)
    to a model or to a checkpoint path, loaded into the script's model of that kind with
    models.checkpoint.load_checkpoint_flexible; `datasets` maps the kind to its test set
    (data.single_modality.RGBDataset / ThermalDataset, data.multimodal.MultimodalDataset).  For
    each kind: select_samples, load_samples, visualize_batch, and one figure per sample saved as
    <output_dir>/<kind>/{healthy|ulcer}_{count:02d}.png (dpi 150, tight bounding box).  A kind
    without an entry in `models`, or whose checkpoint file does not exist, prints the script's
    "Checkpoint not found" line and is skipped.  Prints the script's progress lines; returns
    the list of files written."""
    bar = "=" * 70
    print(bar)
    print("GRAD-CAM VISUALIZATION FOR DFU MODELS")
    print(bar)
    print(f"Device: {device}\n")
    print(f"✓ Will visualize {num_healthy} healthy + {num_ulcer} ulcer samples per model\n")
    written = []
    for kind in KINDS:
        mark, title, name = _BANNERS[kind]
        print("\n" + mark * 35)
        print(title)
        print(mark * 35)
        entry = models.get(kind)
        if entry is None or (isinstance(entry, (str, os.PathLike)) and not os.path.exists(entry)):
            print(f"❌ Checkpoint not found: {entry}")
            continue
        if isinstance(entry, (str, os.PathLike)):
            from models.checkpoint import load_checkpoint_flexible
            print(f"Loading: {entry}")
            model = _build_model(kind).to(device)
            if not load_checkpoint_flexible(model, entry, device):
                raise ValueError(f"{entry}: no model_state_dict in the checkpoint")
        else:
            model = entry
        out_dir = os.path.join(str(output_dir), kind)
        os.makedirs(out_dir, exist_ok=True)
        selected = select_samples(_labels(datasets[kind]), num_healthy, num_ulcer)
        counts = [0, 0]
        if selected:
            rgb, thermal = load_samples(datasets[kind], kind, [s[0] for s in selected], device)
            batch = visualize_batch(model, kind, rgb=rgb, thermal=thermal)
            for i, (_, cls, count) in enumerate(selected):
                fig = FIGURES[kind](sample_at(batch, i))
                path = os.path.join(out_dir, f"{CLASS_NAMES[cls]}_{count:02d}.png")
                fig.savefig(path, dpi=150, bbox_inches="tight")
                print(f"  ✓ Saved {os.path.basename(path)}")
                written.append(path)
                counts[cls] += 1
        print(f"\n✅ Saved {sum(counts)} {name} visualizations ({counts[0]} healthy, "
              f"{counts[1]} ulcer) to {out_dir}")
    print("\n" + bar)
    print("✅ GRAD-CAM VISUALIZATION COMPLETE")
    print(f"📁 Output directory: {output_dir}")
    print(bar)
    return written
