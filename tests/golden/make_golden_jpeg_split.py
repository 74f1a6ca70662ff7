"""Writes tests/golden/jpeg_split_pil.npz: baseline JPEG files large enough to be cut into many sub-segments (include/gg_jscan.h), most of them without restart
markers, each with the RGB that Pillow decoded from it -- Pillow's own results are the fixture, as in tests/golden/jpeg_pil.npz.

    python tests/golden/make_golden_jpeg_split.py

Arrays: file_<i> (uint8 file bytes), rgb_<i> (uint8 H x W x 3, Image.open(...).convert("RGB")), desc (one string per case).  While it writes them the generator runs
the restatement of the scheme (tests/jscan_ref.py) at split_bytes = 512 on every file and asserts that at most 10 % of its sub-segments take the slow path: a
property of these inputs that the GPU test then holds the device to.  Made with Pillow 12.2 (libjpeg-turbo)."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import jpeg_ref as J                                              # noqa: E402
from tests import jscan_ref as S                                             # noqa: E402


def content(kind, w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "noise":
        a = np.stack([xx * 0.8, yy, 255 - xx * 0.5 - yy * 0.3], 2) + rng.integers(-48, 48, (h, w, 3))
    elif kind == "texture":                                   # structure plus noise: what a photograph's blocks look like to the coder
        a = np.stack([127 + 100 * np.sin(xx / 9.0) * np.cos(yy / 6.0), 40 + 1.1 * xx + 0.7 * yy, 200 - 0.9 * xx + 0.4 * yy], 2) + rng.normal(0, 14, (h, w, 3))
    elif kind == "gradient":                                  # smooth: long runs of blocks that are a DC difference and an end-of-block
        a = np.stack([40 + 1.0 * xx, 30 + 1.2 * yy, 220 - 0.5 * xx - 0.5 * yy], 2)
    else:                                                     # saturated checkerboard: large coefficients, many FF 00 in the stream
        c = ((xx.astype(int) // 3 + yy.astype(int) // 2) & 1) * 255.0
        a = np.stack([c, 255.0 - c, c], 2)
    return np.clip(a, 0, 255).astype(np.uint8)


CASES = [                                                     # (W, H, sampling, content, quality, save options)
    (160, 160, "4:2:0", "noise", 90, {}),
    (200, 136, "4:2:2", "noise", 50, {}),
    (200, 136, "4:4:4", "texture", 95, {}),
    (160, 160, "grey", "noise", 90, {}),
    (200, 136, "4:2:0", "texture", 90, {"optimize": True}),
    (200, 136, "4:4:4", "checker", 95, {}),
    (200, 136, "4:4:4", "gradient", 95, {}),
    (160, 160, "4:2:2", "texture", 95, {}),
    (160, 160, "4:2:0", "noise", 90, {"restart_marker_rows": 4}),
    (200, 136, "4:2:2", "texture", 95, {"restart_marker_rows": 4}),
]


def slow_share(data, split):
    """(sub-segments, of which on the slow path) of a whole file, by the restatement"""
    p = J.parse(data)
    total, ri = p["mcux"] * p["mcuy"], p["ri"]
    nc = p["ncomp"]
    blocks = [p["hs"] * p["vs"], 1, 1] if nc == 3 else [1, 0, 0]
    nsub = slow = 0
    for i, (b, e) in enumerate(p["segments"]):
        mcu0 = i * ri if ri else 0
        r = S.run(bytes(data[b:e]), min(ri, total - mcu0) if ri else total, nc, blocks, p["dc"], p["ac"], split)
        assert r["status"] == 0
        nsub += r["nsub"]; slow += r["slow"]
    return nsub, slow


def main():
    rng = np.random.default_rng(20261019)
    out, desc = {}, []
    for i, (w, h, mode, kind, q, kw) in enumerate(CASES):
        im, buf = Image.fromarray(content(kind, w, h, rng)), io.BytesIO()
        if mode == "grey":
            im.convert("L").save(buf, "JPEG", quality=q, **kw)
        else:
            im.save(buf, "JPEG", quality=q, subsampling=mode, **kw)
        data = buf.getvalue()
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert rgb.shape == (h, w, 3)
        nsub, slow = slow_share(data, 512)
        assert nsub >= (2 if kind == "gradient" else 4) and 10 * slow <= nsub, (i, nsub, slow)   # the gradient is small whatever the settings: blocks of a few bits
        out[f"file_{i}"], out[f"rgb_{i}"] = np.frombuffer(data, np.uint8), rgb
        desc.append(f"{w}x{h} {mode} {kind} q{q} {' '.join(sorted(kw))}".strip())
        print(f"{desc[-1]}: {len(data)} bytes, {data.count(bytes([255, 0]))} x FF 00, {nsub} sub-segments at 512 bytes, {slow} slow")
    out["desc"] = np.array(desc)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_split_pil.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print(f"{path}: {len(CASES)} files, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
