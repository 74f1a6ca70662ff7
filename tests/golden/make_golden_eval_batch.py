"""Produces tests/golden/eval_batch_pil.npz: the fixture of the batched eval transform (include/gg_eval.h, tests/test_eval_transform_cpu.py,
tests/test_gpu_eval_transform.py).  Pillow itself makes every expected crop -- ``Image.resize((Wr, Hr), filter)`` of the whole image, then ``Image.crop`` -- for
fourteen (source size, pipeline, size, crop_pct, crop mode) geometries; the resized size and the crop origin are the published formulas of the three upstream
transforms (timm ``transforms_imagenet_eval``, transformers ``CLIPImageProcessor``, torchvision ``Resize`` + ``CenterCrop``), restated below.

    python tests/golden/make_golden_eval_batch.py          (needs Pillow; written with 12.2.0)

Sources follow make_golden_r5.py::synth: smooth structure + noise + hard edges, so bicubic overshoot clips at 0 and 255."""
import math
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (source H, W, pipeline, size, crop_pct, crop mode)
CASES = [
    (37, 53, "timm", 32, 0.875, "center"),
    (61, 29, "timm", 32, 1.0, "center"),
    (32, 32, "timm", 32, 1.0, "center"),            # neither axis resamples
    (32, 48, "timm", 32, 1.0, "center"),            # a copy with a column offset
    (17, 23, "clip", 32, 1.0, "center"),            # up-scale
    (301, 97, "torchvision", 16, 1.0, "center"),    # 6x reduction, bilinear, large ksize
    (45, 70, "timm", 32, 0.9, "squash"),
    (33, 64, "clip", 32, 1.0, "center"),
    (64, 35, "torchvision", 32, 1.0, "center"),
    (32, 32, "timm", 32, 0.875, "center"),
    (40, 32, "clip", 32, 1.0, "center"),            # a copy with a row offset
    (97, 301, "timm", 16, 0.875, "center"),
    (35, 50, "timm", 32, 0.9, "squash"),            # only the horizontal pass runs
    (50, 35, "timm", 32, 0.9, "squash"),            # only the vertical pass runs
]


def synth(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.zeros((h, w, 3))
    for c in range(3):
        a[..., c] = 127 + 90 * np.sin(x / (7.0 + 3 * c) + c) * np.cos(y / (11.0 - 2 * c)) + 35 * g.standard_normal((h, w))
        a[(y.astype(int) // 23 + x.astype(int) // 31 + c) % 5 == 0, c] = 255 * ((c + seed) % 2)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def geometry(h, w, pipeline, size, crop_pct, mode):
    """(PIL filter, (Hr, Wr), (top, left)): shortest edge -> s, long edge int(s * long / short); torchvision / timm centre crop int(round((H - c) / 2.0)),
    transformers (H - c) // 2."""
    flt = Image.BILINEAR if pipeline == "torchvision" else Image.BICUBIC
    s = int(math.floor(size / crop_pct)) if pipeline == "timm" else size
    if pipeline == "timm" and mode == "squash":
        hr, wr = s, s
    elif w <= h:
        wr, hr = s, int(s * h / w)
    else:
        hr, wr = s, int(s * w / h)
    if pipeline == "clip":
        top, left = (hr - size) // 2, (wr - size) // 2
    else:
        top, left = int(round((hr - size) / 2.0)), int(round((wr - size) / 2.0))
    return flt, (hr, wr), (top, left)


def main():
    out = {"pipeline": np.array([c[2] for c in CASES]), "size": np.array([c[3] for c in CASES], np.int32), "crop_pct": np.array([c[4] for c in CASES], np.float64),
           "crop_mode": np.array([c[5] for c in CASES]), "geom": np.zeros((len(CASES), 4), np.int32), "filter": np.zeros(len(CASES), np.int32),
           "pillow_version": np.array(Image.__version__)}
    for i, (h, w, pipeline, size, crop_pct, mode) in enumerate(CASES):
        src = synth(h, w, 100 + i)
        flt, (hr, wr), (top, left) = geometry(h, w, pipeline, size, crop_pct, mode)
        assert hr >= size and wr >= size, (i, hr, wr)
        im = Image.fromarray(src, "RGB").resize((wr, hr), flt).crop((left, top, left + size, top + size))
        crop = np.asarray(im, np.uint8)
        assert crop.shape == (size, size, 3)
        out[f"src{i}"], out[f"crop{i}"] = src, crop
        out["geom"][i], out["filter"][i] = (hr, wr, top, left), int(flt)
    clipped = sum(int((out[f"crop{i}"] == 0).sum() + (out[f"crop{i}"] == 255).sum()) for i in range(len(CASES)))
    assert clipped > 0
    np.savez_compressed(os.path.join(HERE, "eval_batch_pil.npz"), **out)
    print("wrote eval_batch_pil.npz:", len(CASES), "cases,", clipped, "bytes at 0 / 255")


if __name__ == "__main__":
    main()
