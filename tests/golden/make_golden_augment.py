"""Produces tests/golden/augment_pil.npz by running PILLOW ITSELF (12.2; never on the GPU box): the pieces of timm's training transform
(``create_transform(is_training=True, auto_augment='rand-m9-mstd0.5-inc1')``) as timm 1.0.21's transforms.py / auto_augment.py call them --

    img.crop(box).resize((S, S), filter)          RandomResizedCropAndInterpolation (torchvision F.resized_crop)
    img.transpose(FLIP_LEFT_RIGHT)                RandomHorizontalFlip
    ImageOps.autocontrast / equalize / invert / posterize / solarize, img.point(lut) (solarize_add)
    ImageEnhance.Color / Contrast / Brightness / Sharpness (...).enhance(f)
    img.transform(size, AFFINE, m, resample, fillcolor) (shear, translate), img.rotate(angle, resample, fillcolor)

on three seeded sources, two boxes each.  A case is (source, box, filter, flip, op slot) -> the uint8 (S, S, 3) image; op -1 is the resize alone.

    python tests/golden/make_golden_augment.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import augment_ref as R  # noqa: E402  (op ids and Pillow's rotate matrix, which the golden then pins)

S = 32
FILL = (124, 116, 104)


def sources():
    g = np.random.default_rng(20240)
    noise = g.integers(0, 256, (50, 50, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:61, 0:83]
    grad = np.stack([(yy * 4 + xx) % 256, (xx * 3) % 256, (255 - yy * 2 - xx) % 256], -1).astype(np.uint8)
    # a constant channel, a two-level channel whose rare level has fewer than 255 pixels (Equalize: step == 0), and noise
    flat = np.empty((96, 64, 3), np.uint8)
    flat[..., 0] = 77
    flat[..., 1] = 200
    flat[24:30, 20:40, 1] = 10
    flat[..., 2] = g.integers(0, 256, (96, 64), dtype=np.uint8)
    return [noise, grad, flat]


# (top, left, h, w): per source one box with an axis equal to S and one narrower than S (upsampling) or wider (reduction)
BOXES = [[(5, 7, 32, 20), (2, 3, 45, 40)], [(10, 20, 40, 50), (0, 0, 61, 83)], [(20, 16, 32, 32), (8, 4, 80, 24)]]


def op_slots():
    """(op, iarg, factor, pillow call) twice per op: both signs or two magnitudes; a factor above and below 1; Posterize of 8 bits; both resample codes."""
    out = []
    add = lambda op, fn, iarg=0, factor=1.0, m=None, resample=3: out.append((op, iarg, factor, m, resample, fn))
    add(R.AUTO_CONTRAST, lambda im: ImageOps.autocontrast(im))
    add(R.AUTO_CONTRAST, lambda im: ImageOps.autocontrast(ImageOps.autocontrast(im)))      # second variant: marked below as a two-layer case
    add(R.EQUALIZE, lambda im: ImageOps.equalize(im))
    add(R.EQUALIZE, lambda im: ImageOps.equalize(ImageOps.equalize(im)))
    add(R.INVERT, lambda im: ImageOps.invert(im))
    add(R.INVERT, lambda im: ImageOps.invert(ImageOps.invert(im)))
    for bits in (2, 8):
        add(R.POSTERIZE, lambda im, b=bits: ImageOps.posterize(im, b), iarg=bits)
    for t in (26, 200):
        add(R.SOLARIZE, lambda im, t=t: ImageOps.solarize(im, t), iarg=t)
    for a in (99, 30):
        def sol_add(im, a=a):
            lut = [min(255, i + a) if i < 128 else i for i in range(256)]
            return im.point(lut + lut + lut)
        add(R.SOLARIZE_ADD, sol_add, iarg=a)
    for op, cls in ((R.COLOR, ImageEnhance.Color), (R.CONTRAST, ImageEnhance.Contrast), (R.BRIGHTNESS, ImageEnhance.Brightness), (R.SHARPNESS, ImageEnhance.Sharpness)):
        for f in (1.81, 0.37):
            add(op, lambda im, c=cls, f=f: c(im).enhance(f), factor=f)
    for ang, rs in ((27.0, 3), (-13.5, 2)):
        add(R.ROTATE, lambda im, a=ang, rs=rs: im.rotate(a, resample=rs, fillcolor=FILL), m=R.rotate_matrix(ang, S, S), resample=rs)
    for v, rs in ((0.27, 2), (-0.19, 3)):
        add(R.SHEAR_X, lambda im, v=v, rs=rs: im.transform(im.size, Image.AFFINE, (1, v, 0, 0, 1, 0), resample=rs, fillcolor=FILL), m=[1, v, 0, 0, 1, 0], resample=rs)
        add(R.SHEAR_Y, lambda im, v=v, rs=rs: im.transform(im.size, Image.AFFINE, (1, 0, 0, v, 1, 0), resample=rs, fillcolor=FILL), m=[1, 0, 0, v, 1, 0], resample=rs)
    for pct, rs in ((0.405, 3), (-0.13, 2)):
        px = pct * S
        add(R.TRANSLATE_X, lambda im, p=px, rs=rs: im.transform(im.size, Image.AFFINE, (1, 0, p, 0, 1, 0), resample=rs, fillcolor=FILL), m=[1, 0, px, 0, 1, 0], resample=rs)
        add(R.TRANSLATE_Y, lambda im, p=px, rs=rs: im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, p), resample=rs, fillcolor=FILL), m=[1, 0, 0, 0, 1, px], resample=rs)
    return out


def main():
    srcs = sources()
    rows, outs = [], []

    def base(si, box, flt, flip):
        t, l, h, w = box
        im = Image.fromarray(srcs[si]).crop((l, t, l + w, t + h)).resize((S, S), flt)
        return im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im

    def row(si, box, flt, flip, op=-1, layers=0, iarg=0, factor=1.0, m=None, resample=3):
        rows.append(dict(src=si, box=box, filter=flt, flip=flip, op=op, layers=layers, iarg=iarg, factor=factor, m=m or [1, 0, 0, 0, 1, 0], resample=resample))

    for si in range(3):
        for bi, box in enumerate(BOXES[si]):
            for flt in (2, 3):
                flip = (si + bi + flt) % 2
                row(si, box, flt, flip)
                outs.append(np.asarray(base(si, box, flt, flip)))
    slots = op_slots()
    for si in range(3):
        im = base(si, BOXES[si][0], 3, 0)
        seen = set()
        for op, iarg, factor, m, resample, fn in slots:
            # the parameter-free ops' second variant is the op applied twice (two layers of the same slot)
            layers = 2 if op in (R.AUTO_CONTRAST, R.EQUALIZE, R.INVERT) and op in seen else 1
            seen.add(op)
            row(si, BOXES[si][0], 3, 0, op, layers, iarg, factor, m, resample)
            outs.append(np.asarray(fn(im)))
    n = len(rows)
    np.savez_compressed(
        os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment_pil.npz"),
        S=np.int32(S), fill=np.array(FILL, np.uint8), pillow=np.array(Image.__version__),
        src0=srcs[0], src1=srcs[1], src2=srcs[2],
        case_src=np.array([r["src"] for r in rows], np.int32), case_box=np.array([r["box"] for r in rows], np.int32),
        case_filter=np.array([r["filter"] for r in rows], np.int32), case_flip=np.array([r["flip"] for r in rows], np.int32),
        case_op=np.array([r["op"] for r in rows], np.int32), case_layers=np.array([r["layers"] for r in rows], np.int32),
        case_iarg=np.array([r["iarg"] for r in rows], np.int32), case_factor=np.array([r["factor"] for r in rows], np.float32),
        case_m=np.array([r["m"] for r in rows], np.float64), case_resample=np.array([r["resample"] for r in rows], np.int32),
        out=np.stack(outs).astype(np.uint8))
    print(f"wrote augment_pil.npz: {n} cases (Pillow {Image.__version__})")


if __name__ == "__main__":
    main()
