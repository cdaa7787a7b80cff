"""GPU input pipeline: the reference's torchvision transforms (train_multimodal_fusion.py:172-205)
run as two HIP launches per modality per batch (csrc/augment.hip), bit-exact with torchvision's
PIL backend for the same random parameters.

Division of labour (MI355X-first): the host decodes (PIL, exactly as the reference's DataLoader
workers do), draws the per-sample random parameters in torchvision's order, and packs one
pinned staging buffer per batch — descriptors, parameters, resize taps and the decoded bytes —
which crosses PCIe as ONE copy.  Resize, flips, rotation, colour jitter, affine, ToTensor and
Normalize then run on the GPU and the batch lands in HBM as the fp32 NCHW tensors the
reference's model receives.

Parameter draws follow torchvision's transforms (version pinned by the reference's
requirements, not installed here): RandomHorizontalFlip / RandomVerticalFlip
`torch.rand(1) < p`; RandomRotation `uniform_(-deg, deg)`; RandomApply `p < torch.rand(1)`
skips; ColorJitter `randperm(4)` then brightness, contrast, saturation factors
`uniform_(1 - 0.3, 1 + 0.3)`; RandomAffine angle, tx, ty (`int(round(uniform_(-0.1 W, 0.1 W)))`),
scale; RandomApply coin, then GaussianBlur sigma `uniform_(0.1, 0.5)`.  The pixel arithmetic
given those parameters is pinned against PIL itself (tests/test_augment_gpu.py); the draw order
is "parity unpinned" (torchvision absent).

The thermal-only script's train transform (train_thermal_only.py:103-112,
`thermal_only_train_transform`) ends in RandomApply([GaussianBlur(3, (0.1, 0.5))]).  torchvision
blurs a PIL image as a tensor (F.gaussian_blur: fp32 conv2d after a reflect pad, torch.round
back to uint8), not through PIL, so that arithmetic is restated from its source, parity
unpinned (include/dfu_hip.h, dfu_augment_blur; tests/test_blur_gpu.py pins it against an fp64
restatement up to rounding ties).

Test-time augmentation (notebooks/test_time_augmentation.py:145-167): `rgb_tta_transform` /
`thermal_tta_transform` put the rotation before the flips (TransformSpec.order) and use a bare
RandomAffine without a scale; `views=K` on the preprocessor and the loaders gives K views per
image from one decode, one copy and one resize (dfu_augment_views; tests/test_tta_gpu.py).

Aspect-preserving standardisation (scripts/standardize_images.py:58-76, the step that makes the
`*_standardized` trees notebooks/ablation_study.py reads): `standardized(spec)` sets
TransformSpec.standardize = T, and the first device stage is then the script's letterbox in
place of the Resize — each image resized to its own `letterbox_dims` (longest edge T, PIL
bilinear) and placed centred on a black T x T canvas (dfu_letterbox_batch), pinned against PIL's
own resize + paste (tests/test_standardize_gpu.py).  The random ops, `views=K` and the blur read
the canvas unchanged; the batch still crosses PCIe as one copy.  This equals the reference's disk
flow bit for bit only for losslessly stored trees (PNG, BMP, TIFF): the script re-encodes a .jpg
at quality 95 and training decodes that.  data/standardize.py is the offline tool that writes
those files.
"""
import ctypes
import math
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field, replace
from functools import lru_cache

import numpy as np
import torch

from dfu_hip import _lib as L
from dfu_hip._lib import check

AUG_PROB = 0.6  # train_multimodal_fusion.py:37
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
THERMAL_MEAN = (0.5, 0.5, 0.5)
THERMAL_STD = (0.5, 0.5, 0.5)

BRIGHTNESS, CONTRAST, SATURATION = (L.DFU_AUG_BRIGHTNESS, L.DFU_AUG_CONTRAST,
                                    L.DFU_AUG_SATURATION)  # enum dfu_aug_op

RESIZE_DESC = np.dtype(L.ResizeDesc)  # dfu_resize_desc
AUG_PARAMS = np.dtype(L.AugParams)    # dfu_aug_params


@dataclass(frozen=True)
class TransformSpec:
    """One of the reference's Compose pipelines (resize -> random ops -> normalize)."""
    size: tuple = (224, 224)                 # (H, W) of transforms.Resize
    hflip_p: float = 0.0
    vflip_p: float = 0.0
    rotation: float = 0.0                     # RandomRotation(degrees); 0 = absent
    jitter: tuple = None                      # ColorJitter(brightness, contrast, saturation)
    jitter_p: float = 0.0
    affine: tuple = None                      # RandomAffine(degrees, translate, scale);
                                              # scale None = no scale argument (no draw, 1.0)
    affine_p: float = 0.0                     # RandomApply's p; None = a bare RandomAffine
    mean: tuple = IMAGENET_MEAN
    std: tuple = IMAGENET_STD
    order: str = "flip_rotate"                # flips then rotation (the train scripts), or
                                              # "rotate_flip" (test_time_augmentation.py)
    blur: tuple = None                        # GaussianBlur sigma range (sigma_min, sigma_max),
                                              # after the affine
    blur_p: float = 0.0                       # RandomApply's p; None = a bare GaussianBlur
    blur_kernel: int = 3                      # GaussianBlur kernel_size: only 3 is implemented
    standardize: int = None                   # T: standardize_images.py's letterbox to T x T
                                              # first, then the Compose; size must be (T, T)

    def __post_init__(self):
        if self.blur_kernel != 3:
            raise NotImplementedError(f"GaussianBlur kernel_size {self.blur_kernel}: only 3")
        if self.standardize is not None:
            T = self.standardize
            if not isinstance(T, int) or T < 1:
                raise ValueError(f"standardize = {T!r}: a positive target edge")
            if tuple(self.size) != (T, T):
                # the reference's Resize((224, 224)) on a standardised 224 x 224 file is PIL's
                # copy; another size would be a second resample of the canvas
                raise NotImplementedError(f"standardize {T} with Resize{tuple(self.size)}: "
                                          f"only size == ({T}, {T})")

    @property
    def random(self):
        return bool(self.hflip_p or self.vflip_p or self.rotation or self.jitter or self.affine
                    or self.blur)


# train_multimodal_fusion.py:172-205
rgb_train_transform = TransformSpec(hflip_p=0.5, vflip_p=0.5, rotation=30,
                                    jitter=(0.3, 0.3, 0.3), jitter_p=AUG_PROB,
                                    affine=(20, (0.1, 0.1), (0.8, 1.2)), affine_p=AUG_PROB)
rgb_val_test_transform = TransformSpec()
thermal_train_transform = TransformSpec(hflip_p=0.5, vflip_p=0.5, rotation=30,
                                        affine=(20, (0.1, 0.1), (0.8, 1.2)), affine_p=AUG_PROB,
                                        mean=THERMAL_MEAN, std=THERMAL_STD)
thermal_val_test_transform = TransformSpec(mean=THERMAL_MEAN, std=THERMAL_STD)
# train_thermal_only.py:103-112: the thermal train transform, then
# RandomApply([GaussianBlur(kernel_size=3, sigma=(0.1, 0.5))], p=AUG_PROB)
thermal_only_train_transform = replace(thermal_train_transform, blur=(0.1, 0.5),
                                       blur_p=AUG_PROB)
# test_time_augmentation.py:145-167 get_light_augmentation_transforms: Resize, RandomRotation(15),
# the two flips, a bare RandomAffine(10, translate=(0.05, 0.05)), ToTensor, Normalize
rgb_tta_transform = TransformSpec(hflip_p=0.5, vflip_p=0.5, rotation=15,
                                  affine=(10, (0.05, 0.05), None), affine_p=None,
                                  order="rotate_flip")
thermal_tta_transform = TransformSpec(hflip_p=0.5, vflip_p=0.5, rotation=15,
                                      affine=(10, (0.05, 0.05), None), affine_p=None,
                                      mean=THERMAL_MEAN, std=THERMAL_STD, order="rotate_flip")
ORDERS = {"flip_rotate": L.DFU_AUG_ORDER_FLIP_ROTATE,
          "rotate_flip": L.DFU_AUG_ORDER_ROTATE_FLIP}  # enum dfu_aug_order


def standardized(spec, target=224):
    """`spec` on standardize_images.py's output: letterbox the raw image to target x target,
    then the spec as before (what the reference computes from its *_standardized trees)."""
    return replace(spec, standardize=target)


def letterbox_dims(w, h, target):
    """standardize_images.py:58-73 for a w x h image: (out_w, out_h, pad_x, pad_y), the
    script's own float expressions.  The double rounding is the script's: int(m * (target / m))
    is target - 1 for some longest edges m (55, 71, 83, ... at 224), and such an image keeps a
    one-pixel black strip on the right or bottom.
    ValueError where an output side is 0 (PIL's resize raises there and the script counts the
    image as an error).  NotImplementedError where the short output side is below 3: for very
    thin images PIL's resize gives the bytes of the vertical pass first, which the kernels
    (horizontal first) do not model; every such case met has out_w <= 2."""
    scale = target / max(w, h)
    out_w = int(w * scale)
    out_h = int(h * scale)
    if out_w == 0 or out_h == 0:
        raise ValueError(f"letterbox {w} x {h} -> {out_w} x {out_h}: height and width must be > 0")
    if min(out_w, out_h) < 3:
        raise NotImplementedError(f"letterbox {w} x {h} -> {out_w} x {out_h}: short side "
                                  f"below 3 (PIL's pass order for thin images)")
    return out_w, out_h, (target - out_w) // 2, (target - out_h) // 2


@dataclass
class AugParams:
    """Random parameters of one sample, as torchvision would have drawn them."""
    hflip: bool = False
    vflip: bool = False
    angle: float = 0.0                        # RandomRotation
    ops: list = field(default_factory=list)   # [(op, factor)] ColorJitter, in applied order
    affine: tuple = None                      # (angle, (tx, ty), scale, (shear_x, shear_y))
    blur: float = None                        # GaussianBlur sigma; None = not applied


def _uniform(a, b, g):
    return float(torch.empty(1).uniform_(a, b, generator=g).item())


def sample_params(spec, generator=None):
    """Draw one sample's parameters in the order torchvision's Compose consumes the torch RNG
    (generator None = the global RNG, as the reference's transforms use).  spec.order places
    the rotation angle after the flip coins ("flip_rotate") or before them ("rotate_flip")."""
    g = generator
    p = AugParams()
    H, W = spec.size
    if spec.order not in ORDERS:
        raise ValueError(f"TransformSpec.order {spec.order!r}")
    if spec.rotation and spec.order == "rotate_flip":
        p.angle = _uniform(-float(spec.rotation), float(spec.rotation), g)
    if spec.hflip_p:
        p.hflip = bool(torch.rand(1, generator=g) < spec.hflip_p)
    if spec.vflip_p:
        p.vflip = bool(torch.rand(1, generator=g) < spec.vflip_p)
    if spec.rotation and spec.order == "flip_rotate":
        p.angle = _uniform(-float(spec.rotation), float(spec.rotation), g)
    if spec.jitter is not None and not (spec.jitter_p < torch.rand(1, generator=g)):
        order = torch.randperm(4, generator=g).tolist()
        f = [_uniform(max(0.0, 1 - v), 1 + v, g) for v in spec.jitter]
        p.ops = [(k, f[k]) for k in order if k < 3]   # hue (3) is None in the reference
    if spec.affine is not None and (spec.affine_p is None
                                    or not (spec.affine_p < torch.rand(1, generator=g))):
        deg, (tr_x, tr_y), scale_range = spec.affine
        angle = _uniform(-float(deg), float(deg), g)
        max_dx, max_dy = float(tr_x * W), float(tr_y * H)
        tx = int(round(_uniform(-max_dx, max_dx, g)))
        ty = int(round(_uniform(-max_dy, max_dy, g)))
        scale = _uniform(*scale_range, g) if scale_range is not None else 1.0
        p.affine = (angle, (tx, ty), scale, (0.0, 0.0))
    if spec.blur is not None and (spec.blur_p is None
                                  or not (spec.blur_p < torch.rand(1, generator=g))):
        p.blur = _uniform(float(spec.blur[0]), float(spec.blur[1]), g)
    return p


def blur_weight_rows(sigmas):
    """torchvision _get_gaussian_kernel1d(3, sigma) for every sigma of a batch: the three fp32
    weights of GaussianBlur's separable kernel by the same torch ops (restated), fp32 [n][3],
    with a zero row (no blur) for None.  One set of torch calls on an [n, 3] tensor per batch,
    not one per sample (3 ms per batch of 64, EXPERIMENTS.md); each row has the bits the ops
    give for that sigma alone (tests/test_blur_cpu.py).  The 2-D weight of tap (j, i) is
    fp32(k[j] * k[i]), formed in the kernel."""
    rows = np.zeros((len(sigmas), 3), np.float32)
    idx = [i for i, s in enumerate(sigmas) if s is not None]
    if idx:
        sig = torch.tensor([sigmas[i] for i in idx], dtype=torch.float64).float()
        x = torch.linspace(-1, 1, steps=3)
        pdf = torch.exp(-0.5 * (x[None, :] / sig[:, None]).pow(2))
        rows[idx] = (pdf / pdf.sum(1, keepdim=True)).numpy()
    return rows


def blur_weights(sigma):
    """The three fp32 weights of one sigma."""
    return blur_weight_rows([sigma])[0]


# ------------------------------------------------------------------ inverse maps (host)
def rotate_matrix(angle, W, H):
    """PIL Image.rotate(angle, expand=False, center=None) inverse affine matrix, or None when
    PIL copies the image (angle % 360 == 0).  angle % 360 in {90, 180, 270} takes PIL's
    transpose fast paths, which this pipeline does not model (never drawn by +-30 degrees)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    if angle == 180 or (angle in (90, 270) and W == H):
        raise NotImplementedError("rotation by a multiple of 90 degrees")
    cx, cy = W / 2, H / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0,
         round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m2 = m[0] * -cx + m[1] * -cy + m[2]
    m5 = m[3] * -cx + m[4] * -cy + m[5]
    m[2], m[5] = m2 + cx, m5 + cy
    return m


def affine_matrix(angle, translate, scale, shear, W, H):
    """torchvision F.affine for PIL images: _get_inverse_affine_matrix about the centre
    (W * 0.5, H * 0.5)."""
    cx, cy = W * 0.5, H * 0.5
    tx, ty = translate
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [x / scale for x in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def fixed_map(m, W, H):
    """PIL Geometry.c affine_fixed: 16.16 coefficients with the pixel-centre terms folded in.
    Raises when PIL would take another path (ImagingScaleAffine for a pure scale, the float
    path when a coordinate leaves +-32768) — neither is reachable by the reference's ranges."""
    if m[1] == 0 and m[3] == 0:
        raise NotImplementedError("pure scaling affine (PIL ImagingScaleAffine)")
    for x, y in ((0, 0), (W, H), (0, H), (W, 0)):
        if abs(m[0] * x + m[1] * y + m[2]) >= 32768.0 or abs(m[3] * x + m[4] * y + m[5]) >= 32768.0:
            raise NotImplementedError("affine map outside PIL's fixed-point range")

    def fix(v):
        v = v * 65536.0 + 0.5
        return int(math.floor(v)) if v < 0 else int(v)
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def pack_params(params, spec):
    """AugParams list -> dfu_aug_params records."""
    H, W = spec.size
    rec = np.zeros(len(params), AUG_PARAMS)
    for i, p in enumerate(params):
        rec["hflip"][i], rec["vflip"][i] = int(p.hflip), int(p.vflip)
        m = rotate_matrix(p.angle, W, H) if p.angle else None
        if m is not None:
            rec["rotate"][i] = 1
            rec["rot"][i] = fixed_map(m, W, H)
        if p.affine is not None:
            rec["affine"][i] = 1
            rec["aff"][i] = fixed_map(affine_matrix(*p.affine, W, H), W, H)
        rec["n_ops"][i] = len(p.ops)
        for k, (op, f) in enumerate(p.ops):
            rec["op"][i][k], rec["factor"][i][k] = op, f
    return rec


# ------------------------------------------------------------------------- resize taps
@lru_cache(maxsize=4096)
def resize_taps(in_size, out_size):
    """(ksize, bounds int32 [out][2], weights int32 [out][ksize]) from the native host code."""
    lib = L.load()
    k = lib.dfu_resize_ksize(in_size, out_size)
    if k <= 0:
        raise ValueError(f"resize {in_size} -> {out_size}")
    bounds = np.empty((out_size, 2), np.int32)
    kk = np.empty((out_size, k), np.int32)
    check(lib.dfu_resize_coeffs(in_size, out_size, bounds.ctypes.data_as(ctypes.c_void_p),
                                kk.ctypes.data_as(ctypes.c_void_p)), "dfu_resize_coeffs")
    return k, bounds, kk


def _align(n, a=256):
    return (n + a - 1) // a * a


class GpuPreprocessor:
    """Applies one TransformSpec to a batch of decoded H x W x 3 uint8 images on the GPU."""

    def __init__(self, spec, device="cuda"):
        self.spec = spec
        self.device = torch.device(device)
        if spec.blur is not None and min(spec.size) < 2:
            raise ValueError(f"GaussianBlur reflects about the edge: size {spec.size} < 2 x 2")
        self._mean = (ctypes.c_float * 3)(*spec.mean)
        self._std = (ctypes.c_float * 3)(*spec.std)

    def __call__(self, images, params=None, views=None):
        return self.run(self.stage(images, params, views))

    def stage(self, images, params=None, views=None):
        """Host side of one batch: pack descriptors, parameters, resize taps and pixels into one
        pinned buffer and start its single H2D copy on the current stream.  views=K (test-time
        augmentation): K parameter records per image, sample-major (view v of image i at
        i * K + v); the images are still staged, copied and resized once."""
        spec = self.spec
        OH, OW = spec.size
        n = len(images)
        if views is None and spec.order != "flip_rotate":
            views = 1  # dfu_augment_normalize has the train scripts' order only
        if views is not None and views < 1:
            raise ValueError(f"views = {views}")
        if n == 0:
            return _Staged(None, 0, 0, 0, 0, 0, views)
        nv = n * (views or 1)
        if params is None:
            params = [AugParams() for _ in range(nv)]
        if len(params) != nv:
            raise ValueError("one AugParams per image" if views is None
                             else f"{views} AugParams per image, sample-major")
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError(f"expected H x W x 3 uint8 images, got {im.shape}")
        desc = np.zeros(n, RESIZE_DESC)
        # spec.standardize: each image's letterbox box, int32 [n][4] (dfu_letterbox_batch)
        T = spec.standardize
        boxes = np.zeros((n if T is not None else 0, 4), np.int32)
        taps, coef_len, src_len, tmp_len = [], 0, 0, 0
        for i, im in enumerate(imgs):
            h, w = im.shape[:2]
            ow, oh = OW, OH
            if T is not None:
                try:
                    ow, oh, pad_x, pad_y = letterbox_dims(w, h, T)
                except (ValueError, NotImplementedError) as e:
                    raise type(e)(f"image {i} of the batch: {e}") from None
                # the entry point cannot read device records: what it requires is checked here
                if not (0 < ow <= T and 0 < oh <= T and 0 <= pad_x <= T - ow
                        and 0 <= pad_y <= T - oh):
                    raise ValueError(f"image {i} of the batch: box {ow} x {oh} at "
                                     f"({pad_x}, {pad_y}) leaves the {T} x {T} canvas")
                boxes[i] = (ow, oh, pad_x, pad_y)
            kh, bh, wh = resize_taps(w, ow)
            kv, bv, wv = resize_taps(h, oh)
            desc[i] = (src_len, tmp_len, coef_len, w, h, kh, kv)
            taps.append((bh, wh, bv, wv))
            coef_len += bh.size + wh.size + bv.size + wv.size
            src_len += im.size
            tmp_len += h * ow * 3
        rec = pack_params(params, spec)
        # with views, each record's source image follows the records: view_src int32 [n * K]
        view_src = (np.repeat(np.arange(n, dtype=np.int32), views) if views is not None
                    else np.empty(0, np.int32))
        # with a blur, each record's 1-D weights: blur_k fp32 [nv][3], zeros = not blurred
        blur_k = (blur_weight_rows([p.blur for p in params]) if spec.blur is not None
                  else np.empty(0, np.float32))
        # one staging buffer: [descs, boxes | params, view_src | blur_k | taps | pixels], 256-byte
        # aligned sections (no boxes without spec.standardize, no blur_k section without spec.blur)
        o_par = _align(desc.nbytes + boxes.nbytes)
        o_blur = o_par + _align(rec.nbytes + view_src.nbytes)
        o_coef = o_blur + _align(blur_k.nbytes)
        o_src = o_coef + _align(coef_len * 4)
        total = o_src + src_len + 4  # the resize reads whole dwords of the last row
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        buf = stage.numpy()
        buf[:desc.nbytes] = desc.view(np.uint8)
        buf[desc.nbytes:desc.nbytes + boxes.nbytes] = boxes.reshape(-1).view(np.uint8)
        buf[o_par:o_par + rec.nbytes] = rec.view(np.uint8)
        buf[o_par + rec.nbytes:o_par + rec.nbytes + view_src.nbytes] = view_src.view(np.uint8)
        buf[o_blur:o_blur + blur_k.nbytes] = blur_k.reshape(-1).view(np.uint8)
        cv = buf[o_coef:o_coef + coef_len * 4].view(np.int32)
        at = 0
        for t in taps:
            for a in t:
                cv[at:at + a.size] = a.ravel()
                at += a.size
        at = o_src
        for im in imgs:
            buf[at:at + im.size] = im.ravel()
            at += im.size
        return _Staged(stage.to(self.device, non_blocking=True), n, o_par, o_coef, o_src,
                       tmp_len, views, o_par + rec.nbytes,
                       o_blur if spec.blur is not None else None,
                       desc.nbytes if T is not None else None)

    def resize(self, st, out=None):
        """First device stage of a staged batch: uint8 [n, H, W, 3], the resized images, or with
        spec.standardize the letterboxed canvases (what standardize_images.py saves).  `out`: a
        contiguous uint8 CUDA tensor of that many bytes to write into; every byte is written."""
        OH, OW = self.spec.size
        if out is None:
            out = torch.empty((st.n, OH, OW, 3), dtype=torch.uint8, device=self.device)
        if (out.dtype != torch.uint8 or out.numel() != st.n * OH * OW * 3
                or not out.is_contiguous() or out.device.type != "cuda"):
            raise ValueError("out: a contiguous uint8 CUDA tensor of n * H * W * 3 bytes")
        if st.n == 0:
            return out
        lib = L.load()
        base = st.dev.data_ptr()
        tmp = torch.empty(st.tmp_len, dtype=torch.uint8, device=self.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if st.o_box is not None:  # spec.standardize: the letterbox in place of the resize
            check(lib.dfu_letterbox_batch(ctypes.c_void_p(base + st.o_src), ctypes.c_void_p(base),
                                          ctypes.c_void_p(base + st.o_box),
                                          ctypes.c_void_p(base + st.o_coef), st.n, OH,
                                          ctypes.c_void_p(tmp.data_ptr()),
                                          ctypes.c_void_p(out.data_ptr()), stream),
                  "dfu_letterbox_batch")
        else:
            check(lib.dfu_resize_batch(ctypes.c_void_p(base + st.o_src), ctypes.c_void_p(base),
                                       ctypes.c_void_p(base + st.o_coef), st.n, OW, OH,
                                       ctypes.c_void_p(tmp.data_ptr()),
                                       ctypes.c_void_p(out.data_ptr()), stream),
                  "dfu_resize_batch")
        return out

    def run(self, st):
        """Device side: resize (or letterbox) + augment + normalise a staged batch (4 launches);
        a batch staged with views gives [n * K, 3, H, W], sample-major (dfu_augment_views).  A
        spec with a blur goes through dfu_augment_blur instead, with or without views."""
        OH, OW = self.spec.size
        if st.n == 0:
            return torch.empty((0, 3, OH, OW), dtype=torch.float32, device=self.device)
        lib = L.load()
        base = st.dev.data_ptr()
        resized = self.resize(st)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if self.spec.blur is not None:
            nv = st.n * (st.views or 1)
            out = torch.empty((nv, 3, OH, OW), dtype=torch.float32, device=self.device)
            means = torch.empty(nv, dtype=torch.int32, device=self.device)
            view_src = ctypes.c_void_p(base + st.o_view) if st.views is not None else None
            check(lib.dfu_augment_blur(ctypes.c_void_p(resized.data_ptr()), st.n,
                                       ctypes.c_void_p(base + st.o_par), view_src,
                                       ctypes.c_void_p(base + st.o_blur), nv,
                                       ORDERS[self.spec.order], OH, OW, self._mean, self._std,
                                       ctypes.c_void_p(means.data_ptr()),
                                       ctypes.c_void_p(out.data_ptr()), stream),
                  "dfu_augment_blur")
            return out
        if st.views is not None:
            nv = st.n * st.views
            out = torch.empty((nv, 3, OH, OW), dtype=torch.float32, device=self.device)
            means = torch.empty(nv, dtype=torch.int32, device=self.device)
            check(lib.dfu_augment_views(ctypes.c_void_p(resized.data_ptr()), st.n,
                                        ctypes.c_void_p(base + st.o_par),
                                        ctypes.c_void_p(base + st.o_view), nv,
                                        ORDERS[self.spec.order], OH, OW, self._mean, self._std,
                                        ctypes.c_void_p(means.data_ptr()),
                                        ctypes.c_void_p(out.data_ptr()), stream),
                  "dfu_augment_views")
            return out
        out = torch.empty((st.n, 3, OH, OW), dtype=torch.float32, device=self.device)
        means = torch.empty(st.n, dtype=torch.int32, device=self.device)
        check(lib.dfu_augment_normalize(ctypes.c_void_p(resized.data_ptr()),
                                        ctypes.c_void_p(base + st.o_par), st.n, OH, OW,
                                        self._mean, self._std, ctypes.c_void_p(means.data_ptr()),
                                        ctypes.c_void_p(out.data_ptr()), stream),
              "dfu_augment_normalize")
        return out


@dataclass
class _Staged:
    dev: torch.Tensor      # the batch's staging buffer in HBM
    n: int
    o_par: int
    o_coef: int
    o_src: int
    tmp_len: int
    views: int = None      # K parameter records per image (dfu_augment_views), None: one each
    o_view: int = 0        # view_src int32 [n * K]
    o_blur: int = None     # blur_k fp32 [n * K][3] (dfu_augment_blur), None: a spec without blur
    o_box: int = None      # boxes int32 [n][4] (dfu_letterbox_batch), None: a plain Resize


def decode_rgb(path):
    """MultimodalDataset.__getitem__'s decode: Image.open(path).convert('RGB') as H x W x 3."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def _check_views(views):
    if not isinstance(views, int) or views < 1:
        raise ValueError(f"views = {views!r}: a positive number of views per sample")
    return views


class GpuPairLoader:
    """DataLoader replacement for MultimodalDataset (train_multimodal_fusion.py:259-275): yields
    (rgb, thermal, label) batches already on the GPU, fp32 NCHW as the reference's loader
    produces them after pin_memory + .to(DEVICE).  Decode runs on `num_threads` host threads
    one batch ahead of the GPU; per sample the RGB parameters are drawn before the thermal
    ones, as __getitem__ applies the two transforms.  views=K > 1 (test-time augmentation,
    test_time_augmentation.py:347-361): [B * K, 3, H, W] inputs, view v of sample i in row
    i * K + v, and [B] labels; per sample and per view the RGB parameters before the thermal
    ones, the order of the script's nested loops."""

    def __init__(self, dataset, batch_size, sampler=None, shuffle=False, train=False,
                 rgb_spec=None, thermal_spec=None, device="cuda", num_threads=4, generator=None,
                 drop_last=False, views=1):
        self.dataset = dataset
        self.batch_size = batch_size
        self.sampler = sampler
        self.shuffle = shuffle
        self.generator = generator
        self.drop_last = drop_last
        self.views = _check_views(views)
        rgb_spec = rgb_spec or (rgb_train_transform if train else rgb_val_test_transform)
        thermal_spec = thermal_spec or (thermal_train_transform if train
                                        else thermal_val_test_transform)
        self.rgb = GpuPreprocessor(rgb_spec, device)
        self.thermal = GpuPreprocessor(thermal_spec, device)
        self.device = torch.device(device)
        self.num_threads = num_threads

    def _batches(self):
        if self.sampler is not None:
            order = list(self.sampler)
        elif self.shuffle:
            order = torch.randperm(len(self.dataset), generator=self.generator).tolist()
        else:
            order = list(range(len(self.dataset)))
        bs = self.batch_size
        for s in range(0, len(order), bs):
            b = order[s:s + bs]
            if len(b) < bs and self.drop_last:
                return
            yield b

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _decode(self, pool, idx):
        pairs = [self.dataset.pairs[i] for i in idx]
        rgb = pool.map(decode_rgb, [p[0] for p in pairs])
        th = pool.map(decode_rgb, [p[1] for p in pairs])
        return list(rgb), list(th), [p[2] for p in pairs]

    def __iter__(self):
        # one thread orchestrates the next batch's decode on the pool (a pool task waiting on
        # its own pool could starve it)
        with ThreadPoolExecutor(self.num_threads) as pool, ThreadPoolExecutor(1) as ahead:
            pending = None
            for idx in self._batches():
                nxt = ahead.submit(self._decode, pool, idx)
                if pending is not None:
                    yield self._finish(*pending.result())
                pending = nxt
            if pending is not None:
                yield self._finish(*pending.result())

    def _finish(self, rgb, th, labels):
        rp, tp = [], []
        for _ in range(len(labels) * self.views):  # sample-major: every view of a sample in turn
            rp.append(sample_params(self.rgb.spec, self.generator) if self.rgb.spec.random
                      else AugParams())
            tp.append(sample_params(self.thermal.spec, self.generator) if self.thermal.spec.random
                      else AugParams())
        y = torch.tensor(labels, dtype=torch.long).to(self.device, non_blocking=True)
        k = self.views if self.views > 1 else None
        return self.rgb(rgb, rp, k), self.thermal(th, tp, k), y


class GpuImageLoader:
    """DataLoader replacement for the single-modality datasets (data.single_modality:
    RGBDataset, train_rgb_only.py:181-197; ThermalDataset): yields (images, labels) already on
    the GPU, fp32 NCHW, through the same decode-ahead threads and HIP transform kernels as
    GpuPairLoader.  `spec` defaults to the RGB train / val-test transform of
    train_rgb_only.py:102-118 (the fusion script's RGB transforms, identical).  The thermal-only
    script's loaders (train_thermal_only.py:103-118) are GpuImageLoader(ds, bs, train=True,
    spec=thermal_only_train_transform), whose train transform ends in a GaussianBlur, and
    spec=thermal_val_test_transform.  views=K > 1: [B * K, 3, H, W] images, sample-major, and
    [B] labels, as GpuPairLoader."""

    def __init__(self, dataset, batch_size, sampler=None, shuffle=False, train=False,
                 spec=None, device="cuda", num_threads=4, generator=None, drop_last=False,
                 views=1):
        self.dataset = dataset
        self.batch_size = batch_size
        self.sampler = sampler
        self.shuffle = shuffle
        self.generator = generator
        self.drop_last = drop_last
        self.views = _check_views(views)
        spec = spec or (rgb_train_transform if train else rgb_val_test_transform)
        self.pre = GpuPreprocessor(spec, device)
        self.device = torch.device(device)
        self.num_threads = num_threads

    _batches = GpuPairLoader._batches
    __len__ = GpuPairLoader.__len__

    def _decode(self, pool, idx):
        imgs = pool.map(decode_rgb, [self.dataset.image_paths[i] for i in idx])
        return list(imgs), [self.dataset.labels[i] for i in idx]

    def __iter__(self):
        with ThreadPoolExecutor(self.num_threads) as pool, ThreadPoolExecutor(1) as ahead:
            pending = None
            for idx in self._batches():
                nxt = ahead.submit(self._decode, pool, idx)
                if pending is not None:
                    yield self._finish(*pending.result())
                pending = nxt
            if pending is not None:
                yield self._finish(*pending.result())

    def _finish(self, imgs, labels):
        params = [sample_params(self.pre.spec, self.generator) if self.pre.spec.random
                  else AugParams() for _ in range(len(labels) * self.views)]
        y = torch.tensor(labels, dtype=torch.long).to(self.device, non_blocking=True)
        return self.pre(imgs, params, self.views if self.views > 1 else None), y
