"""Records what gg_preprocess_pil computes on the build it is run on: SHA-256 digests of dst_u8 and of the bytes of dst for seeded uint8 images, one record per case.
Run ONCE on the commit BEFORE the per-image path was folded into the batch passes (on an MI355X); tests/test_gpu_eval_transform.py
(test_per_image_bits_unchanged_from_the_parent_build) holds every later build to that file.  The file holds data only: the geometry, the seed and the digests.

The cases are the smallest shapes at which the fold can go wrong: the six geometries of the guard-band case (tests/test_gpu_guards.py::test_preprocess_pil: down, up,
no-op, both filters, odd crop offsets, mul_rescale 0 / 1, with and without normalize), 17 x 9 -> 33 x 20 with both filters, a horizontal-only and a vertical-only
resize, and one strip of 5 x 24 000 -> 5 x 2048 whose row span (72 000 bytes) is beyond what a workgroup of the batch passes stages in LDS.
    python tools/make_preprocess_pil_parent_golden.py [--out tests/golden/preprocess_pil_parent.json]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
#        name                  Hs  Ws     flt Hr  Wr    top left Hc  Wc    mul norm
CASES = [("guard_down_bicubic", 50, 60, 3, 28, 34, 2, 5, 24, 24, 0, 1),
         ("guard_up_bilinear", 17, 9, 2, 33, 20, 0, 0, 33, 20, 1, 1),
         ("guard_noop", 8, 8, 2, 8, 8, 0, 0, 8, 8, 0, 0),
         ("guard_tiny_bilinear", 5, 7, 2, 3, 4, 1, 1, 2, 3, 0, 1),
         ("guard_odd_bicubic", 64, 31, 3, 16, 8, 3, 1, 10, 7, 1, 0),
         ("guard_half_bicubic", 40, 90, 3, 20, 45, 0, 11, 20, 23, 0, 1),
         ("up_17x9_bilinear", 17, 9, 2, 33, 20, 0, 0, 33, 20, 0, 1),
         ("up_17x9_bicubic", 17, 9, 3, 33, 20, 0, 0, 33, 20, 0, 1),
         ("horizontal_only", 20, 40, 3, 20, 16, 0, 0, 20, 16, 0, 1),
         ("vertical_only", 40, 20, 3, 16, 20, 0, 0, 16, 20, 0, 1),
         ("strip_beyond_lds", 5, 24000, 3, 5, 2048, 0, 0, 5, 2048, 0, 1)]


def source(seed, Hs, Ws):
    return np.random.default_rng(seed).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)


def digests(ops, c):
    """(sha256 of dst_u8, sha256 of dst's bytes) of one per-image call for case record c"""
    img = torch.from_numpy(source(c["seed"], c["Hs"], c["Ws"])).cuda()
    norm = bool(c["normalize"])
    pv, u8 = ops.preprocess_pil(img, c["filter"], (c["Hr"], c["Wr"]), (c["top"], c["left"]), (c["Hc"], c["Wc"]), MEAN if norm else None, STD if norm else None,
                                mul_rescale=bool(c["mul_rescale"]), want_u8=True)
    torch.cuda.synchronize()
    return hashlib.sha256(u8.cpu().numpy().tobytes()).hexdigest(), hashlib.sha256(pv.cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "preprocess_pil_parent.json"))
    a = ap.parse_args()
    from geoguessr_ai_amd import _lib as L, ops
    L.require_gpu()
    keys = ("name", "Hs", "Ws", "filter", "Hr", "Wr", "top", "left", "Hc", "Wc", "mul_rescale", "normalize")
    cases = []
    for i, row in enumerate(CASES):
        c = dict(zip(keys, row), seed=1000 + i)
        c["u8_sha256"], c["f32_sha256"] = digests(ops, c)
        cases.append(c)
        print(json.dumps(c))
    rec = dict(tool="make_preprocess_pil_parent_golden", device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:12], mean=MEAN, std=STD, cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
