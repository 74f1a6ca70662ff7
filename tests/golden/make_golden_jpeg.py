"""Writes tests/golden/jpeg_pil.npz: baseline JPEG files that Pillow encoded together with the RGB that Pillow decoded from them (so Pillow's own results are the
fixture of the device decoder, include/gg_jpeg.h), and one hand-assembled header per refusal of the host-side plan (headers only: no image data follows them).

    python tests/golden/make_golden_jpeg.py

Arrays: file_<i> (uint8 file bytes), rgb_<i> (uint8 H x W x 3, Image.open(...).convert("RGB")), desc (one string per case); refuse_<i> (uint8 header bytes),
refuse_name (the refusal's name, gg_jpeg_refusal_name), refuse_desc.  Made with Pillow 12.2 (libjpeg-turbo)."""
import io
import os
import struct

import numpy as np
from PIL import Image

SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (40, 48), (33, 50), (3, 70), (47, 9), (64, 48)]          # (W, H)
MODES = ["4:4:4", "4:2:2", "4:2:0", "grey"]


def content(kind, w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        a = np.stack([127 + 120 * np.sin(xx / 7.0 + 0.3) * np.cos(yy / 5.0), 40 + 3.1 * xx + 1.7 * yy, 200 - 2.3 * xx + 0.9 * yy], 2)
    elif kind == "noise":
        a = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
    else:                                                     # saturated checkerboard: reaches the range-limit clamp
        c = ((xx.astype(int) // 3 + yy.astype(int) // 2) & 1) * 255.0
        a = np.stack([c, 255.0 - c, c], 2)
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, mode, quality, **kw):
    im = Image.fromarray(a)
    buf = io.BytesIO()
    if mode == "grey":
        im.convert("L").save(buf, "JPEG", quality=quality, **kw)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=mode, **kw)
    data = buf.getvalue()
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return np.frombuffer(data, np.uint8), rgb


def seg(marker, payload=b""):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def refusal_headers():
    SOI, JFIF = b"\xff\xd8", seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    dqt = seg(0xDB, bytes([0]) + bytes([16] * 64)) + seg(0xDB, bytes([1]) + bytes([17] * 64))
    counts = bytes([0, 2, 2] + [0] * 13)
    dht = b"".join(seg(0xC4, bytes([tc << 4 | th]) + counts + bytes([0, 1, 2, 3])) for tc in (0, 1) for th in (0, 1))

    def sof(marker=0xC0, prec=8, h=16, w=16, comps=((1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1))):
        return seg(marker, struct.pack(">BHHB", prec, h, w, len(comps)) + b"".join(bytes(c) for c in comps))

    def sos(ids=(1, 2, 3)):
        return seg(0xDA, bytes([len(ids)]) + b"".join(bytes([i, 0x00 if n == 0 else 0x11]) for n, i in enumerate(ids)) + bytes([0, 63, 0]))

    adobe0 = seg(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0))
    rgb_ids = ((ord("R"), 0x11, 0), (ord("G"), 0x11, 0), (ord("B"), 0x11, 0))
    cases = [
        ("not a JPEG (no SOI)", "a PNG signature", b"\x89PNG\r\n\x1a\n" + bytes(16)),
        ("progressive (SOF2)", "SOF2", SOI + JFIF + dqt + sof(0xC2)),
        ("unsupported SOF (lossless or hierarchical)", "SOF3", SOI + JFIF + dqt + sof(0xC3)),
        ("arithmetic coding", "SOF9", SOI + JFIF + dqt + sof(0xC9)),
        ("sample precision is not 8 bits", "SOF1 with 12-bit samples", SOI + JFIF + dqt + sof(0xC1, prec=12)),
        ("component count is not 1 or 3", "2 components", SOI + JFIF + dqt + sof(comps=((1, 0x11, 0), (2, 0x11, 1)))),
        ("component count is not 1 or 3", "4 components", SOI + adobe0 + dqt + sof(comps=((1, 0x11, 0), (2, 0x11, 0), (3, 0x11, 0), (4, 0x11, 0)))),
        ("three components that are not Y'CbCr", "Adobe APP14 with transform 0", SOI + adobe0 + dqt + sof(comps=((1, 0x11, 0), (2, 0x11, 0), (3, 0x11, 0))) + dht + sos()),
        ("three components that are not Y'CbCr", "ids R G B without JFIF or Adobe", SOI + dqt + sof(comps=rgb_ids) + dht + sos(tuple(c[0] for c in rgb_ids))),
        ("unsupported sampling factors", "4:4:0 (luma 1x2)", SOI + JFIF + dqt + sof(comps=((1, 0x12, 0), (2, 0x11, 1), (3, 0x11, 1)))),
        ("unsupported sampling factors", "4:1:1 (luma 4x1)", SOI + JFIF + dqt + sof(comps=((1, 0x41, 0), (2, 0x11, 1), (3, 0x11, 1)))),
        ("unsupported sampling factors", "chroma 2x1", SOI + JFIF + dqt + sof(comps=((1, 0x22, 0), (2, 0x21, 1), (3, 0x11, 1)))),
        ("more than one scan or a non-interleaved scan", "a scan of one of three components", SOI + JFIF + dqt + sof() + dht + sos((1,))),
        ("more than one scan or a non-interleaved scan", "a second SOS after the first scan", SOI + JFIF + dqt + sof() + dht + sos() + sos()),
        ("missing or invalid DQT / DHT", "no DQT for the chroma components", SOI + JFIF + seg(0xDB, bytes([0]) + bytes([16] * 64)) + sof() + dht + sos()),
        ("missing or invalid DQT / DHT", "no DHT at all", SOI + JFIF + dqt + sof() + sos()),
        ("missing or invalid DQT / DHT", "a DHT with three codes of length 1", SOI + JFIF + dqt + sof() + seg(0xC4, bytes([0x00, 3] + [0] * 15 + [0, 1, 2])) + dht[21 + 4:] + sos()),
        ("restart markers disagree with DRI", "DRI 1 and no restart marker", SOI + JFIF + dqt + sof(w=32) + dht + seg(0xDD, b"\0\x01") + sos() + b"\x12\x34\xff\xd9"),
        ("restart markers disagree with DRI", "a restart marker without DRI", SOI + JFIF + dqt + sof() + dht + sos() + b"\x12\xff\xd0\x34\xff\xd9"),
        ("restart markers disagree with DRI", "RST1 first", SOI + JFIF + dqt + sof(h=8, w=32) + dht + seg(0xDD, b"\0\x01") + sos() + b"\x12\xff\xd1\x34\xff\xd9"),
        ("header runs past the end of the file", "an APP0 longer than the file", SOI + JFIF[:9]),
        ("header runs past the end of the file", "the file ends before SOS", SOI + JFIF + dqt + sof() + dht),
        ("height or width 0 or above 16384", "height 0", SOI + JFIF + dqt + sof(h=0)),
        ("height or width 0 or above 16384", "width 20000", SOI + JFIF + dqt + sof(w=20000)),
    ]
    return cases


def main():
    rng = np.random.default_rng(20261019)
    cases = []
    kinds, quals = ["smooth", "noise", "checker"], [30, 75, 95, 100]
    n = 0
    for (w, h) in SIZES:                                      # every size in every sampling, content and quality rotating
        for mode in MODES:
            cases.append((w, h, mode, kinds[n % 3], quals[n % 4], {})); n += 1
    for mode in MODES:
        cases.append((40, 48, mode, "noise", 75, {"optimize": True}))
        cases.append((33, 50, mode, "smooth", 95, {"restart_marker_blocks": 3}))
        cases.append((17, 23, mode, "noise", 30, {"restart_marker_blocks": 3, "optimize": True}))
        cases.append((64, 48, mode, "noise", 75, {"restart_marker_rows": 1}))
        cases.append((16, 16, mode, "checker", 100, {}))
        cases.append((47, 9, mode, "checker", 30, {}))
        for q in quals:
            cases.append((40, 48, mode, "smooth", q, {}))
    cases.append((33, 50, "4:2:0", "smooth", 75, {"comment": b"a comment segment", "exif": b"Exif\0\0MM\0*\0\0\0\x08\0\0\0\0\0\0"}))
    out, desc = {}, []
    for i, (w, h, mode, kind, q, kw) in enumerate(cases):
        data, rgb = encode(content(kind, w, h, rng), mode, q, **kw)
        assert rgb.shape == (h, w, 3)
        out[f"file_{i}"], out[f"rgb_{i}"] = data, rgb
        desc.append(f"{w}x{h} {mode} {kind} q{q} {' '.join(sorted(kw))}".strip())
    out["desc"] = np.array(desc)
    ref = refusal_headers()
    for i, (_, _, data) in enumerate(ref):
        out[f"refuse_{i}"] = np.frombuffer(data, np.uint8)
    out["refuse_name"] = np.array([r[0] for r in ref])
    out["refuse_desc"] = np.array([r[1] for r in ref])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_pil.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(cases)} files, {len(ref)} refusal headers, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
