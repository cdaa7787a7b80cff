"""The reference's offline standardisation (scripts/standardize_images.py) with the resample on
the GPU: every image of a tree resized so that its longest edge is `target_size` (PIL bilinear,
aspect kept) and pasted centred on a black target_size x target_size canvas, saved under the same
relative path.  This produces the `rgb_standardized/` and `thermal_standardized/` trees that
notebooks/ablation_study.py reads.

The host decodes and encodes with PIL, as the script does; the letterbox of a batch is
dfu_letterbox_batch (csrc/augment.hip) through GpuPreprocessor, bit-exact with the script's
`resize` + `paste` (tests/test_standardize_gpu.py), so the saved files are the script's byte for
byte.  Training straight from raw images with `gpu_transforms.standardized(spec)` skips the files;
it equals the disk flow bit for bit only for losslessly stored trees (PNG, BMP, TIFF): the script
re-encodes a .jpg at quality 95 and training then decodes that.

Neither function prompts, prints or draws progress bars (the script's main() does all three).
"""
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from data import gpu_transforms as GT
from data.multimodal import IMAGE_EXTS


def image_files(root):
    """Every image under `root`, sorted.  Suffixes are matched with suffix.lower(), as this
    project's datasets do: the script globs `*.ext` and `*.EXT` only, so a mixed-case suffix
    (`a.Jpg`) is picked up here and missed there."""
    return sorted(p for p in Path(root).rglob("*")
                  if p.is_file() and p.suffix.lower() in IMAGE_EXTS)


def _decode(path):
    try:
        return GT.decode_rgb(path)  # convert("RGB"): the script's, a copy for an RGB image
    except Exception:
        return None


def standardize_tree(input_dir, output_dir, target_size=224, batch_size=64, device="cuda",
                     num_threads=4):
    """standardize_images.py:13-100 standardize_images.  Returns (success_count, error_count):
    an image that fails to open, decode, letterbox (letterbox_dims' refusals) or save is counted
    as an error and skipped, and the rest go on, as the script's try / except does.
    FileNotFoundError when input_dir does not exist (the script prints and returns False)."""
    from PIL import Image
    input_dir, output_dir = Path(input_dir), Path(output_dir)
    if not input_dir.is_dir():
        raise FileNotFoundError(f"input directory not found: {input_dir}")
    output_dir.mkdir(parents=True, exist_ok=True)
    T = target_size
    pre = GT.GpuPreprocessor(GT.TransformSpec(size=(T, T), standardize=T), device)
    paths = image_files(input_dir)
    success = errors = 0
    with ThreadPoolExecutor(num_threads) as pool:
        for s in range(0, len(paths), batch_size):
            batch, imgs = [], []
            for p, im in zip(paths[s:s + batch_size], pool.map(_decode, paths[s:s + batch_size])):
                try:
                    if im is None:
                        raise ValueError("decode")
                    GT.letterbox_dims(im.shape[1], im.shape[0], T)
                except (ValueError, NotImplementedError):
                    errors += 1
                    continue
                batch.append(p)
                imgs.append(im)
            if not imgs:
                continue
            canvases = pre.resize(pre.stage(imgs)).cpu().numpy()
            for p, c in zip(batch, canvases):
                out = output_dir / p.relative_to(input_dir)
                try:
                    out.parent.mkdir(parents=True, exist_ok=True)
                    Image.fromarray(np.ascontiguousarray(c)).save(out, quality=95)
                    success += 1
                except Exception:
                    errors += 1
    return success, errors


def verify_standardization(directory, target_size=224):
    """standardize_images.py:102-156 verify_standardization: (all_correct, size_distribution).
    size_distribution counts the images by (width, height); all_correct is True when there is
    at least one image and every image opens and is target_size x target_size.  Reads the sizes
    only (no decode, no GPU)."""
    from PIL import Image
    sizes, all_correct = {}, True
    paths = image_files(directory)
    for p in paths:
        try:
            with Image.open(p) as im:
                size = im.size
        except Exception:
            all_correct = False
            continue
        sizes[size] = sizes.get(size, 0) + 1
        if size != (target_size, target_size):
            all_correct = False
    return all_correct and bool(paths), sizes
