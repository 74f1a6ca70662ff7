"""The panorama fine-tune's input path (include/gg_pano.h) restated in numpy, used only as a checker (tests/test_pano_cpu.py pins it on
tests/golden/pano_pil.npz, which Pillow and torch made; tests/test_gpu_pano.py leans on it for images the fixture does not hold): torchvision's ``Resize`` size
rule, Pillow's 8-bit BILINEAR resize (oracle/preprocess_ref.py::pil_resize), ToTensor, ATen's bilinear interpolation in float32 with the source index as ONE
fused multiply-add, the normalisation, and the constant a missing view becomes."""
import numpy as np

from oracle import preprocess_ref as P

F32 = np.float32


def resized_size(h, w, rs):
    """(Hr, Wr): the short edge to rs, the long edge to int(rs * long / short); rs == 0: the image as it is."""
    if rs == 0:
        return h, w
    if w <= h:
        return int(rs * h / w), rs
    return rs, int(rs * w / h)


def resize_u8(img_hwc, rs):
    hr, wr = resized_size(img_hwc.shape[0], img_hwc.shape[1], rs)
    if (hr, wr) == img_hwc.shape[:2]:
        return img_hwc.copy()
    return P.pil_resize(img_hwc, wr, hr, 2)


def _taps(n_in, n_out):
    scale = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32) + F32(0.5)
    src = np.maximum((np.float64(scale) * d.astype(np.float64) - 0.5).astype(F32), F32(0))        # fmaf(scale, d + 0.5, -0.5): the product is exact in double
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    return i0, i1, (F32(1) - l1).astype(F32), l1


def interpolate(x_chw, target):
    """F.interpolate(x[None], size=target, mode="bilinear", align_corners=False)[0] for (3, H, W) float32."""
    x = np.asarray(x_chw, F32)
    if tuple(x.shape[1:]) == tuple(target):
        return x.copy()
    y0, y1, ly0, ly1 = _taps(x.shape[1], target[0])
    x0, x1, lx0, lx1 = _taps(x.shape[2], target[1])
    top = (lx0 * x[:, y0][:, :, x0] + lx1 * x[:, y0][:, :, x1]).astype(F32)
    bot = (lx0 * x[:, y1][:, :, x0] + lx1 * x[:, y1][:, :, x1]).astype(F32)
    return (ly0[:, None] * top + ly1[:, None] * bot).astype(F32)


def normalise(x_chw, mean, std):
    if mean is None or std is None:
        return np.asarray(x_chw, F32)
    return ((x_chw - np.asarray(mean, F32).reshape(3, 1, 1)) / np.asarray(std, F32).reshape(3, 1, 1)).astype(F32)


def view(img_hwc, rs, target, mean=None, std=None):
    """One view: (the resized uint8 image, the (3, Ht, Wt) float32 result); img_hwc None: a missing view (no uint8 image)."""
    if img_hwc is None:
        return None, normalise(np.zeros((3,) + tuple(target), F32), mean, std)
    u8 = resize_u8(np.asarray(img_hwc, np.uint8), rs)
    x = u8.transpose(2, 0, 1).astype(F32) / F32(255)
    return u8, normalise(interpolate(x, target), mean, std)
