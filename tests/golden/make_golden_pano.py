"""Produces tests/golden/pano_pil.npz: the fixture of the panorama fine-tune's input path (include/gg_pano.h, tests/test_pano_cpu.py, tests/test_gpu_pano.py).
Pillow and torch themselves make every expected value, on the CPU: per case a seeded source image, ``Image.resize((Wr, Hr), BILINEAR)`` of it with torchvision's
``Resize(rs)`` size rule (the short edge to rs, the long edge to int(rs * long / short); rs = 0: no resize), then ToTensor (``u8 / 255`` in float32, CHW),
``F.interpolate(size=target, mode="bilinear", align_corners=False)`` and ``(x - mean) / std`` -- with and without the normalisation.

    python tests/golden/make_golden_pano.py          (needs Pillow and torch; written with Pillow 12.2.0)"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# (source H, W, required_size, target (Ht, Wt))
CASES = [
    (17, 33, 8, (12, 12)),
    (33, 17, 8, (5, 9)),
    (70, 3, 3, (6, 6)),               # the short edge is already rs: nothing resamples; a thin image
    (9, 9, 12, (12, 12)),             # an up-scale, then the identity
    (64, 48, 16, (16, 21)),           # resizes to 21 x 16: the transposed target, both axes interpolate
    (64, 48, 16, (21, 16)),           # the interpolation is the identity on a non-square image
    (40, 40, 40, (16, 16)),
    (1, 1, 1, (2, 3)),
    (61, 47, 0, (23, 29)),            # no resize stage
]


def synth(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.zeros((h, w, 3))
    for c in range(3):
        a[..., c] = 127 + 90 * np.sin(x / (7.0 + 3 * c) + c) * np.cos(y / (11.0 - 2 * c)) + 35 * g.standard_normal((h, w))
        a[(y.astype(int) // 23 + x.astype(int) // 31 + c) % 5 == 0, c] = 255 * ((c + seed) % 2)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def resized_size(h, w, rs):
    if rs == 0:
        return h, w
    if w <= h:
        return int(rs * h / w), rs
    return rs, int(rs * w / h)


def main():
    out = {"cases": np.array([(h, w, rs, t[0], t[1]) for h, w, rs, t in CASES], np.int32), "mean": np.array(MEAN, np.float32), "std": np.array(STD, np.float32),
           "pillow_version": np.array(Image.__version__), "torch_version": np.array(torch.__version__)}
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    for i, (h, w, rs, target) in enumerate(CASES):
        src = synth(h, w, 300 + i)
        hr, wr = resized_size(h, w, rs)
        im = Image.fromarray(src, "RGB")
        if rs:
            im = im.resize((wr, hr), Image.BILINEAR)
        u8 = np.asarray(im, np.uint8)
        assert u8.shape == (hr, wr, 3)
        x = torch.from_numpy(u8.copy()).permute(2, 0, 1).contiguous().float().div(255.0).unsqueeze(0)      # ToTensor
        y = F.interpolate(x, size=target, mode="bilinear", align_corners=False)
        out[f"src{i}"], out[f"u8_{i}"] = src, u8
        out[f"plain{i}"], out[f"norm{i}"] = y[0].numpy().copy(), ((y - mean) / std)[0].numpy().copy()
    np.savez_compressed(os.path.join(HERE, "pano_pil.npz"), **out)
    print("wrote pano_pil.npz:", len(CASES), "cases,", os.path.getsize(os.path.join(HERE, "pano_pil.npz")), "bytes")


if __name__ == "__main__":
    main()
