"""Pure-numpy restatement (TEST INFRASTRUCTURE ONLY) of the Pillow operations behind timm's training transform -- crop + resize, flip, and the fifteen RandAugment
ops of the increasing set -- and of one record's whole pipeline, as include/gg_aug.h states them.  Pillow 12.2 is the authority: tests/golden/augment_pil.npz holds
Pillow's own outputs (tests/golden/make_golden_augment.py) and tests/test_augment_cpu.py holds every function here against it byte for byte.  The resize is
oracle.preprocess_ref.pil_resize.  No import of the package: a record is read by field name, so any structured array with the fields of GgAugRecord serves."""
import numpy as np

from oracle.preprocess_ref import pil_resize

(AUTO_CONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X, SHEAR_Y, TRANSLATE_X,
 TRANSLATE_Y) = range(15)
OP_NAMES = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness", "Sharpness", "ShearX",
            "ShearY", "TranslateX", "TranslateY"]
AFFINE_OPS = (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y)
f32 = np.float32


# ------------------------------------------------------------------------------------------------- lookup-table ops (ImageOps)
def _hist(img):
    return [np.bincount(img[..., c].ravel(), minlength=256).astype(np.int64) for c in range(3)]


def lut_autocontrast(h):
    """ImageOps.autocontrast(cutoff=0) of one channel's histogram."""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], np.uint8)


def lut_equalize(h):
    """ImageOps.equalize of one channel's histogram (entries past the last occupied bin, which no pixel reads, are clamped to a byte)."""
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if step == 0:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, np.uint8)


def lut_static(op, iarg):
    i = np.arange(256, dtype=np.int64)
    if op == INVERT:
        return (255 - i).astype(np.uint8)
    if op == POSTERIZE:                                  # timm: bits >= 8 returns the image itself
        return i.astype(np.uint8) if iarg >= 8 else (i & ~(2 ** (8 - iarg) - 1) & 255).astype(np.uint8)
    if op == SOLARIZE:
        return np.where(i < iarg, i, 255 - i).astype(np.uint8)
    if op == SOLARIZE_ADD:
        return np.where(i < 128, np.minimum(255, i + iarg), i).astype(np.uint8)
    raise ValueError(op)


def apply_lut_op(img, op, iarg=0):
    out = np.empty_like(img)
    hs = _hist(img) if op in (AUTO_CONTRAST, EQUALIZE) else None
    for c in range(3):
        lut = lut_autocontrast(hs[c]) if op == AUTO_CONTRAST else lut_equalize(hs[c]) if op == EQUALIZE else lut_static(op, iarg)
        out[..., c] = lut[img[..., c]]
    return out


# ------------------------------------------------------------------------------------------------- blend ops (ImageEnhance)
def grey(img):
    """Image.convert("L") of an RGB image."""
    a = img.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(deg, img, f) on 8-bit pixels: float32 arithmetic, truncated; clamped first when f is outside [0, 1]."""
    f = f32(f)
    d, x = deg.astype(f32), img.astype(f32)
    t = (d + (f * (x - d)).astype(f32)).astype(f32)
    if not (0.0 <= float(f) <= 1.0):
        t = np.clip(t, f32(0), f32(255))
    return t.astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH: 3x3 (1,1,1,1,5,1,1,1,1) / 13 in float32, the accumulator starting at 0.5f and taking the nine products in row-major order; the outermost
    rows and columns are copied."""
    k = [f32(v) / f32(13) for v in (1, 1, 1, 1, 5, 1, 1, 1, 1)]
    a = img.astype(f32)
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    ss = np.full((H - 2, W - 2, 3), f32(0.5), f32)
    for j, (dy, dx) in enumerate([(dy, dx) for dy in (0, 1, 2) for dx in (0, 1, 2)]):
        ss = (ss + (a[dy:dy + H - 2, dx:dx + W - 2] * k[j]).astype(f32)).astype(f32)
    out[1:-1, 1:-1] = np.clip(ss, f32(0), f32(255)).astype(np.uint8)
    return out


def apply_enhance(img, op, f):
    if op == BRIGHTNESS:
        deg = np.zeros_like(img)
    elif op == COLOR:
        deg = np.repeat(grey(img)[..., None], 3, axis=2)
    elif op == CONTRAST:
        g = grey(img)
        deg = np.full_like(img, int(int(g.astype(np.int64).sum()) / g.size + 0.5))
    elif op == SHARPNESS:
        deg = smooth(img)
    else:
        raise ValueError(op)
    return blend(deg, img, f)


# ------------------------------------------------------------------------------------------------- affine ops (Image.transform(AFFINE))
def rotate_matrix(angle, w, h):
    """The matrix Image.rotate(angle) hands to Image.transform (no expand, centre of the image)."""
    import math
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, m, resample, fill):
    """Image.transform(size, AFFINE, m, resample, fillcolor=fill) of an (H, W, 3) uint8 image, in double like Geometry.c."""
    H, W = img.shape[:2]
    a = img.astype(np.float64)
    xs = np.arange(W, dtype=np.float64)[None, :] + 0.5
    ys = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xin = m[0] * xs + m[1] * ys + m[2]
    yin = m[3] * xs + m[4] * ys + m[5]
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    cx = lambda v: np.clip(v, 0, W - 1)
    if resample == 2:
        def row(r):
            return a[r, cx(x)] + (a[r, cx(x + 1)] - a[r, cx(x)]) * dx
        v1 = row(np.clip(y, 0, H - 1))
        v2 = np.where(((y + 1 >= 0) & (y + 1 < H))[..., None], row(np.clip(y + 1, 0, H - 1)), v1)
        v = v1 + (v2 - v1) * dy
    elif resample == 3:
        def row(r):
            return _cubic(a[r, cx(x - 1)], a[r, cx(x)], a[r, cx(x + 1)], a[r, cx(x + 2)], dx)
        v1 = row(np.clip(y - 1, 0, H - 1))
        v2 = np.where(((y >= 0) & (y < H))[..., None], row(np.clip(y, 0, H - 1)), v1)
        v3 = np.where(((y + 1 >= 0) & (y + 1 < H))[..., None], row(np.clip(y + 1, 0, H - 1)), v2)
        v4 = np.where(((y + 2 >= 0) & (y + 2 < H))[..., None], row(np.clip(y + 2, 0, H - 1)), v3)
        v = _cubic(v1, v2, v3, v4, dy)
    else:
        raise ValueError(resample)
    out = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, np.trunc(v))).astype(np.uint8)      # truncated: there is no + 0.5
    return np.where(inside[..., None], out, np.asarray(fill, np.uint8)[None, None, :])


# ------------------------------------------------------------------------------------------------- one op slot, one record
def apply_op(img, op, iarg=0, factor=1.0, m=None, resample=3, fill=(0, 0, 0)):
    op = int(op)
    if op in (AUTO_CONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD):
        return apply_lut_op(img, op, int(iarg))
    if op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        return apply_enhance(img, op, factor)
    if op in AFFINE_OPS:
        return affine(img, [float(v) for v in m], int(resample), fill)
    raise ValueError(op)


def crop_resize_flip(src, top, left, h, w, S, flt, flip):
    out = pil_resize(src[top:top + h, left:left + w], S, S, flt)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def apply_record(src, rec, S, flt):
    """The uint8 (S, S, 3) image one record makes of one (H, W, 3) source: img.crop(box).resize((S, S), flt), the flip, then the record's op slots in order."""
    img = crop_resize_flip(src, int(rec["top"]), int(rec["left"]), int(rec["h"]), int(rec["w"]), S, flt, bool(rec["flip"]))
    for l in range(int(rec["num_layers"])):
        o = rec["ops"][l]
        if int(o["applied"]):
            img = apply_op(img, o["op"], o["iarg"], o["factor"], o["m"], o["resample"], tuple(int(v) for v in o["fill"]))
    return img


def normalise(u8_bhwc, mean, std):
    """ToTensor + Normalize in float32: ((float)u8 / 255.0f - mean) / std, (B, 3, S, S)."""
    x = np.asarray(u8_bhwc).astype(f32).transpose(0, 3, 1, 2) / f32(255)
    return ((x - np.asarray(mean, f32).reshape(1, 3, 1, 1)) / np.asarray(std, f32).reshape(1, 3, 1, 1)).astype(f32)
