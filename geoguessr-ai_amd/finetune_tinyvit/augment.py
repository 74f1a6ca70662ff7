"""The training transform of the reference's ``ImageCSVDataset`` (``finetune_tinyvit/train_tinyvit_timm.py:47-54``) on the device:

    timm.data.create_transform(input_size=img_size, is_training=True, auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic', mean=..., std=...)

i.e. RandomResizedCropAndInterpolation(scale (0.08, 1), ratio (3/4, 4/3)) -> RandomHorizontalFlip(0.5) -> RandAugment -> ToTensor -> Normalize, for a whole batch of
raw uint8 images per call (``gg_aug_batch``, include/gg_aug.h), bit-identical to Pillow on the uint8 side.

timm is not a dependency of this package.  THE SPECIFICATION IS timm 1.0.21's ``timm/data/auto_augment.py`` AND ``timm/data/transforms.py``, RESTATED HERE FROM
THEIR PUBLIC SOURCE: the config string (``rand-mM-mstdS-incI-nN-pP-mmaxX``), the increasing op set, the level -> argument table (timm's ``LEVEL_TO_ARG``: ``level_to_arg`` below), the
per-op probability, the magnitude noise, the fill colour, and ``RandomResizedCropAndInterpolation.get_params``.

The host draws the randomness (``sample_params``), the device does the pixels.  The draws come from a ``numpy.random.Generator``: THIS IS NOT timm's RANDOM STREAM
(timm mixes Python's ``random`` and ``numpy.random``) -- the distribution is timm's, the draws are not, so a seed here does not reproduce a timm run image for image.
One deviation in distribution: with ``interpolation='random'`` timm draws the resize filter per image, here it is drawn once per batch (``gg_aug_batch`` takes one
filter per call); the per-op resample code of the affine ops is drawn per op as in timm."""
from __future__ import annotations

import ctypes as C
import math
import re
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .._lib import GgError
from ..training.preprocess import PIL_BICUBIC, PIL_BILINEAR, TINYVIT_MEAN, TINYVIT_STD, _rgb_hwc

(AUTO_CONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X, SHEAR_Y, TRANSLATE_X,
 TRANSLATE_Y) = range(15)                 # GG_AUG_* of include/gg_aug.h
MAX_LAYERS = _lib.AUG_MAX_LAYERS
LEVEL_DENOM = 10.0                        # timm _LEVEL_DENOM

# timm _RAND_INCREASING_TRANSFORMS, in its order (the "Increasing" / "Rel" variants are the same pixel op with another level -> argument rule)
RAND_INCREASING_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd", "ColorIncreasing",
                       "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
OP_IDS = dict(zip(RAND_INCREASING_OPS, range(15)))

# the numpy mirrors of GgAugOp / GgAugRecord (aligned like the C structs: 72 and 312 bytes)
OP_DTYPE = np.dtype([("op", "<i4"), ("applied", "<i4"), ("iarg", "<i4"), ("factor", "<f4"), ("m", "<f8", (6,)), ("resample", "<i4"), ("fill", "u1", (3,)), ("reserved", "u1")])
RECORD_DTYPE = np.dtype([("top", "<i4"), ("left", "<i4"), ("h", "<i4"), ("w", "<i4"), ("flip", "<i4"), ("num_layers", "<i4"), ("ops", OP_DTYPE, (MAX_LAYERS,))])
assert OP_DTYPE.itemsize == C.sizeof(_lib.AugOp) and RECORD_DTYPE.itemsize == C.sizeof(_lib.AugRecord)


def parse_config(config: str) -> Dict[str, float]:
    """``rand_augment_transform``'s reading of the config string: sections split by '-', the first is ``rand``; ``m`` magnitude (default 10), ``mstd`` its std
    (above 100: uniform magnitudes), ``mmax`` the clamp (default 10), ``inc`` the increasing op set, ``n`` layers (default 2), ``p`` the per-op probability (0.5)."""
    parts = config.split("-")
    if parts[0] != "rand":
        raise ValueError(f"parse_config: only RandAugment ('rand-...') configs are built, got {config!r}")
    out = dict(magnitude=10.0, magnitude_std=0.0, magnitude_max=10.0, increasing=False, num_layers=2, prob=0.5)
    for c in parts[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue                      # timm skips sections without a number
        key, val = cs[0], cs[1]
        if key == "mstd":
            out["magnitude_std"] = float("inf") if float(val) > 100 else float(val)
        elif key == "mmax":
            out["magnitude_max"] = float(int(val))
        elif key == "inc":
            out["increasing"] = bool(int(val))
        elif key == "m":
            out["magnitude"] = float(int(val))
        elif key == "n":
            out["num_layers"] = int(val)
        elif key == "p":
            out["prob"] = float(val)
        else:
            raise ValueError(f"parse_config: unknown RandAugment config section {c!r}")
    if not out["increasing"]:
        raise ValueError("parse_config: only the increasing op set (inc1, the reference's) is built")
    if not 0 <= out["num_layers"] <= MAX_LAYERS:
        raise ValueError(f"parse_config: n={out['num_layers']} layers, the record holds 0..{MAX_LAYERS}")
    return out


def fill_colour(mean: Sequence[float]):
    """timm ``img_mean``: ``tuple(min(255, round(255 * x)) for x in mean)`` -- (124, 116, 104) for the ImageNet mean."""
    return tuple(min(255, round(255 * float(x))) for x in mean)


def rotate_matrix(angle: float, w: int, h: int):
    """The six doubles ``PIL.Image.rotate(angle)`` hands to ``Image.transform(AFFINE)`` (no expand, centre of the image)."""
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def level_to_arg(name: str, level: float, sign: float = 1.0, size: int = 224) -> dict:
    """timm ``LEVEL_TO_ARG`` for the increasing set, as the fields of an op slot.  ``sign``: +1 / -1, what ``_randomly_negate`` drew; ``size``: the image the op runs
    on is ``size`` x ``size`` (it follows the resize)."""
    frac = level / LEVEL_DENOM
    if name in ("AutoContrast", "Equalize", "Invert"):
        return {}
    if name == "Rotate":
        return {"m": rotate_matrix(sign * frac * 30.0, size, size)}
    if name == "PosterizeIncreasing":
        return {"iarg": 4 - int(frac * 4)}
    if name == "SolarizeIncreasing":
        return {"iarg": 256 - int(frac * 256)}
    if name == "SolarizeAdd":
        return {"iarg": min(128, int(frac * 110))}
    if name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
        return {"factor": max(0.1, 1.0 + sign * frac * 0.9)}
    if name in ("ShearX", "ShearY"):
        v = sign * frac * 0.3
        return {"m": [1.0, v, 0.0, 0.0, 1.0, 0.0] if name == "ShearX" else [1.0, 0.0, 0.0, v, 1.0, 0.0]}
    if name in ("TranslateXRel", "TranslateYRel"):
        px = sign * frac * 0.45 * size
        return {"m": [1.0, 0.0, px, 0.0, 1.0, 0.0] if name == "TranslateXRel" else [1.0, 0.0, 0.0, 0.0, 1.0, px]}
    raise ValueError(f"level_to_arg: unknown op {name!r}")


_SIGNED = {"Rotate", "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"}


def crop_box(h: int, w: int, rng: np.random.Generator, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """``RandomResizedCropAndInterpolation.get_params``: (top, left, h, w, accepted)."""
    area = h * w
    for _ in range(10):
        target = rng.uniform(scale[0], scale[1]) * area
        aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        cw = int(round(math.sqrt(target * aspect)))
        ch = int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            top = int(rng.integers(0, h - ch + 1))
            left = int(rng.integers(0, w - cw + 1))
            return top, left, ch, cw, True
    in_ratio = w / h
    if in_ratio < min(ratio):
        cw = w
        ch = int(round(cw / min(ratio)))
    elif in_ratio > max(ratio):
        ch = h
        cw = int(round(ch * max(ratio)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw, False


def sample_params(sizes: Sequence[Sequence[int]], img_size: int = 224, config: str = "rand-m9-mstd0.5-inc1", generator: Optional[np.random.Generator] = None,
                  mean: Sequence[float] = TINYVIT_MEAN, interpolation: str = "bicubic", flip_prob: float = 0.5) -> np.ndarray:
    """One record (``RECORD_DTYPE`` = GgAugRecord) per (height, width) of ``sizes``: the crop box, the flip flag and ``n`` op slots drawn with timm's distribution
    from ``generator`` (NOT timm's random stream: see the module docstring)."""
    rng = generator if generator is not None else np.random.default_rng()
    cfg = parse_config(config)
    fill = fill_colour(mean)
    fixed = {"bilinear": PIL_BILINEAR, "bicubic": PIL_BICUBIC}.get(interpolation)
    if fixed is None and interpolation != "random":
        raise ValueError(f"sample_params: interpolation must be bilinear, bicubic or random, got {interpolation!r}")
    rec = np.zeros(len(sizes), RECORD_DTYPE)
    rec["ops"]["m"][...] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    rec["ops"]["resample"] = PIL_BICUBIC
    rec["ops"]["factor"] = 1.0
    for b, (h, w) in enumerate(sizes):
        r = rec[b]
        r["top"], r["left"], r["h"], r["w"], _ = crop_box(int(h), int(w), rng)
        r["flip"] = int(rng.random() < flip_prob)
        r["num_layers"] = cfg["num_layers"]
        names = rng.integers(0, len(RAND_INCREASING_OPS), cfg["num_layers"])          # uniform, with replacement
        for l, oi in enumerate(names):
            name, o = RAND_INCREASING_OPS[int(oi)], r["ops"][l]
            o["op"] = OP_IDS[name]
            o["applied"] = int(not (cfg["prob"] < 1.0 and rng.random() > cfg["prob"]))
            mag = cfg["magnitude"]
            if cfg["magnitude_std"] == float("inf"):
                mag = rng.uniform(0.0, mag)
            elif cfg["magnitude_std"] > 0:
                mag = rng.normal(mag, cfg["magnitude_std"])
            level = max(0.0, min(mag, cfg["magnitude_max"]))
            sign = (-1.0 if rng.random() > 0.5 else 1.0) if name in _SIGNED else 1.0
            for k, v in level_to_arg(name, level, sign, img_size).items():
                o[k] = v
            o["resample"] = fixed if fixed is not None else int(rng.choice((PIL_BILINEAR, PIL_BICUBIC)))
            o["fill"] = fill
    return rec


def _as_hwc_list(images):
    """What ``images_to_pixel_values`` takes -> a list of (H, W, 3) uint8 tensors (host or device)."""
    if not torch.is_tensor(images):
        seq = list(images) if isinstance(images, (list, tuple)) else [images]
        return [_rgb_hwc(im) for im in seq]
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.uint8:
        raise GgError(f"DeviceTrainTransform: expected raw RGB images, a (N,3,H,W) uint8 tensor, got {tuple(images.shape)} {images.dtype}")
    return [im.permute(1, 2, 0) for im in images]


class DeviceTrainTransform:
    """``create_transform(is_training=True, auto_augment=..., interpolation=...)`` for batches, on the device.  ``__call__(images, params=None)``: PIL images, (H, W, 3)
    uint8 arrays, a list of those or an (N,3,H,W) uint8 tensor -> (N,3,S,S) float32 ``pixel_values`` on ``device`` (with ``return_u8=True`` also the (N,S,S,3) uint8
    batch after the last op).  ``params``: a record table to replay (``sample_params``' layout); otherwise one is drawn from the transform's own generator and kept in
    ``.last_params``.  The workspace is the transform's own and is reused from call to call (it grows when a batch needs more).  ``images`` may also be a list in
    which every item is a JPEG file as bytes (decoded on the device by a ``training.jpeg.DeviceJpegDecoder`` the transform owns) or that decoder's ``PackedImages``.
    ``jpeg_split_bytes`` is that decoder's ``split_bytes`` (0, the default: one lane per restart segment; positive: many lanes inside a scan, the same pixels),
    ``jpeg_progressive`` its ``progressive`` (off, the default: a progressive file is refused by name; on: decoded next to baseline files)."""

    def __init__(self, img_size: int = 224, mean: Sequence[float] = TINYVIT_MEAN, std: Sequence[float] = TINYVIT_STD, auto_augment: str = "rand-m9-mstd0.5-inc1",
                 interpolation: str = "bicubic", seed: int = 0, device="cuda", jpeg_split_bytes: int = 0,
                 jpeg_progressive: bool = False):
        if interpolation not in ("bilinear", "bicubic", "random"):
            raise ValueError(f"DeviceTrainTransform: interpolation must be bilinear, bicubic or random, got {interpolation!r}")
        parse_config(auto_augment)
        self.img_size, self.mean, self.std, self.auto_augment, self.interpolation = int(img_size), tuple(mean), tuple(std), auto_augment, interpolation
        self.device = torch.device(device)
        self.generator = np.random.default_rng(seed)
        self.last_params: Optional[np.ndarray] = None
        self._workspace: Optional[torch.Tensor] = None
        self._decoder = None                              # training.jpeg.DeviceJpegDecoder, made when file bytes first arrive
        self.jpeg_split_bytes = int(jpeg_split_bytes)
        self.jpeg_progressive = bool(jpeg_progressive)

    def _filter(self) -> int:
        if self.interpolation == "random":
            return int(self.generator.choice((PIL_BILINEAR, PIL_BICUBIC)))
        return PIL_BILINEAR if self.interpolation == "bilinear" else PIL_BICUBIC

    def __call__(self, images, params: Optional[np.ndarray] = None, return_u8: bool = False):
        _lib.require_gpu()
        from ..training.jpeg import DeviceJpegDecoder, PackedImages, is_file_bytes, is_file_bytes_list
        if is_file_bytes(images):
            images = [images]
        if is_file_bytes_list(images):                    # JPEG files as bytes: decoded on the device, consumed where the decoded batch lies
            if self._decoder is None:
                self._decoder = DeviceJpegDecoder(self.device, self.jpeg_split_bytes, self.jpeg_progressive)
            images = self._decoder.decode(images)
        decoded = images if isinstance(images, PackedImages) else None
        hwc = [] if decoded is not None else _as_hwc_list(images)
        sizes = [(int(h), int(w)) for h, w in decoded.sizes] if decoded is not None else [(int(im.shape[0]), int(im.shape[1])) for im in hwc]
        if params is None:
            params = sample_params(sizes, self.img_size, self.auto_augment, self.generator, self.mean, self.interpolation)
        params = np.ascontiguousarray(params, RECORD_DTYPE)
        if len(params) != len(sizes):
            raise GgError(f"DeviceTrainTransform: {len(params)} records for {len(sizes)} images")
        self.last_params = params.copy()
        if decoded is not None:
            packed, offsets = decoded.packed, np.ascontiguousarray(decoded.offsets, np.int64)
        else:
            nbytes = [3 * h * w for h, w in sizes]
            offsets = np.concatenate([[0], np.cumsum([(n + 255) // 256 * 256 for n in nbytes])]).astype(np.int64)
            packed = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=self.device)
            for im, off, n in zip(hwc, offsets, nbytes):
                packed[int(off):int(off) + n].copy_(im.reshape(-1), non_blocking=True)
        B, S = len(sizes), self.img_size
        dst = torch.empty(B, 3, S, S, dtype=torch.float32, device=self.device)
        dst_u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device=self.device) if return_u8 else None
        heights, widths = np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32)
        a = _lib.AugArgs()
        a.src, a.src_bytes = packed.data_ptr(), packed.numel()
        a.offsets, a.heights, a.widths = offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data
        a.B, a.S, a.filter = B, S, self._filter()
        a.mean, a.std = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        a.records = None                                  # the bound over every record table for these image sizes
        need = _lib.lib().gg_aug_workspace_bytes(C.byref(a))
        if need < 0:
            raise GgError(f"gg_aug_workspace_bytes: {_lib.lib().gg_last_error().decode(errors='replace')}")
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != self.device:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        a.records = params.ctypes.data
        a.dst, a.dst_u8 = dst.data_ptr(), dst_u8.data_ptr() if dst_u8 is not None else None
        a.workspace, a.workspace_bytes = self._workspace.data_ptr(), self._workspace.numel()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gg_aug_batch(C.byref(a), _lib.stream()), "gg_aug_batch")
        return (dst, dst_u8) if return_u8 else dst


def _hand_split_bytes(transform, jpeg_split_bytes: int, jpeg_progressive: bool = False) -> None:
    if jpeg_split_bytes and getattr(transform, "jpeg_split_bytes", 0) != int(jpeg_split_bytes):
        transform.jpeg_split_bytes, transform._decoder = int(jpeg_split_bytes), None
    if jpeg_progressive and not getattr(transform, "jpeg_progressive", False):
        transform.jpeg_progressive, transform._decoder = True, None


class augmented:
    """``{"images", "labels"}`` batches -> ``{"pixel_values", "labels"}`` batches, lazily, one ``transform`` call per batch: ``train(model, augmented(raw_batches,
    tfm), val_batches, ...)`` is the reference's loop with its training transform.  Iterating is a generator over ``batches``; like a DataLoader the object can be
    walked once per epoch (when ``batches`` can), and every walk draws new records.  ``jpeg_split_bytes`` other than 0 is handed to the transform (its decoder of
    file bytes is made anew with it); 0 leaves the transform as it is.  ``jpeg_progressive=True`` is handed on the same way; off leaves the transform as it is."""

    def __init__(self, batches: Iterable, transform: DeviceTrainTransform, jpeg_split_bytes: int = 0, jpeg_progressive: bool = False):
        self.batches, self.transform = batches, transform
        _hand_split_bytes(transform, jpeg_split_bytes, jpeg_progressive)

    def __iter__(self):
        for batch in self.batches:
            labels = batch["labels"]
            if not torch.is_tensor(labels):
                labels = torch.as_tensor(labels, dtype=torch.int64)
            yield {"pixel_values": self.transform(batch["images"]), "labels": labels.to(self.transform.device)}


class eval_transformed:
    """The twin of ``augmented`` for the validation side -- the reference's ``collate_val``: ``{"images", "labels"}`` batches -> ``{"pixel_values", "labels"}``
    batches, lazily, one ``transform`` call (``training.preprocess.DeviceEvalTransform``: one ``gg_eval_batch``) per batch, so
    ``evaluate(model, eval_transformed(raw_val, tfm))`` and ``extract_embeddings(model, eval_transformed(...))`` run on raw images.  Nothing is drawn: every walk
    yields the same batches.  ``jpeg_split_bytes``, ``jpeg_progressive``: as in ``augmented``."""

    def __init__(self, batches: Iterable, transform, jpeg_split_bytes: int = 0, jpeg_progressive: bool = False):
        self.batches, self.transform = batches, transform
        _hand_split_bytes(transform, jpeg_split_bytes, jpeg_progressive)

    def __iter__(self):
        for batch in self.batches:
            labels = batch["labels"]
            if not torch.is_tensor(labels):
                labels = torch.as_tensor(labels, dtype=torch.int64)
            yield {"pixel_values": self.transform(batch["images"]), "labels": labels.to(self.transform.device)}
