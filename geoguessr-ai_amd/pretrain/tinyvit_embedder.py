"""Drop-in for the reference's ``pretrain/tinyvit_embedder.py`` (``TinyViTEmbedding``, :8-124): frozen TinyViT with
``num_classes=0`` run under ``no_grad``; panorama kwargs ``image_2..4`` stack on dim 1.  Float tensors are pixel_values (:70-72); PIL images /
uint8 arrays or tensors go through timm's eval transform on the device (:51-53,67-69: Pillow bicubic resize of the shortest edge to floor(size / crop_pct) --
of both edges in "squash" mode --, centre crop, /255, ImageNet mean / std: ``training.preprocess.images_to_pixel_values``, bit-identical to Pillow on the
uint8 image)."""
from __future__ import annotations

import torch
from torch import Tensor

from ..models.tinyvit import VARIANTS, TinyViTAdapter, check_attention16


class TinyViTEmbedding(torch.nn.Module):
    def __init__(self, model_name: str = "tiny_vit_21m_512.dist_in22k_ft_in1k", device: str = "cuda", load_checkpoint: bool = False,
                 panorama: bool = False, img_size: int = None, batch_transform: bool = False, jpeg_split_bytes: int = 0, attention16: bool = False,
                 jpeg_progressive: bool = False):
        """``img_size`` (not in the reference): run the checkpoint at another input side (a multiple of 32; ``TinyViTAdapter``'s override) -- the preprocessing
        resizes to that side, with the crop settings of the checkpoint's own variant.  ``batch_transform`` (not in the reference): raw images -- a list of any
        sizes, or the four panorama views together -- go through ONE ``gg_eval_batch`` call (``training.preprocess.DeviceEvalTransform``) instead of one
        ``gg_preprocess_pil`` call per image; same arithmetic.  ``jpeg_split_bytes`` (with ``batch_transform`` only): the ``split_bytes`` of the decoder that
        takes JPEG files given as bytes (``DeviceEvalTransform``'s keyword; 0 is one lane per restart segment); ``jpeg_progressive`` (with ``batch_transform`` only): that decoder's
        ``progressive`` (progressive files are decoded next to baseline ones; off by default).  ``attention16`` (not in the reference; bf16
        only, opt-in): the attention of windows beyond 256 tokens on the 16-bit MFMA (``TinyViTAdapter``'s keyword); the fp32 modes refuse it by name."""
        super().__init__()
        check_attention16(attention16, None, "TinyViTEmbedding")
        self.device, self.panorama, self.model_name = device, panorama, model_name
        self.batch_transform, self._transform = bool(batch_transform), None
        if jpeg_split_bytes and not batch_transform:
            raise ValueError("TinyViTEmbedding: jpeg_split_bytes needs batch_transform=True")
        self.jpeg_split_bytes = int(jpeg_split_bytes)
        if jpeg_progressive and not batch_transform:
            raise ValueError("TinyViTEmbedding: jpeg_progressive needs batch_transform=True")
        self.jpeg_progressive = bool(jpeg_progressive)
        arch = "tiny_vit_21m_224" if load_checkpoint else model_name
        self.tinyvit_model = TinyViTAdapter(arch, pretrained=not load_checkpoint, **({} if img_size is None else dict(img_size=int(img_size))),
                                            **({"attention16": True} if attention16 else {}))
        if load_checkpoint:
            self.tinyvit_model.backbone.load_state_dict(torch.load(model_name, map_location="cpu"))
            print("Loaded embedder from checkpoint:", model_name)
        self.tinyvit_model = self.tinyvit_model.to(device if isinstance(device, str) else f"cuda:{device}")
        self.eval()

    def _eval_transform(self):
        """The batch transform with this checkpoint's crop settings (``batch_transform=True``); it keeps its workspace from call to call."""
        if self._transform is None:
            from ..training.preprocess import TINYVIT_MEAN, TINYVIT_STD, DeviceEvalTransform
            bb = self.tinyvit_model.backbone
            native = VARIANTS[bb.model_name]["img_size"]
            self._transform = DeviceEvalTransform(bb.img_size, TINYVIT_MEAN, TINYVIT_STD, "timm", 0.95 if native == 224 else 1.0,
                                                  "squash" if native == 512 else "center", bb.flat_params.device, jpeg_split_bytes=self.jpeg_split_bytes,
                                                  jpeg_progressive=self.jpeg_progressive)
        return self._transform

    def _get_embedding(self, image) -> Tensor:
        if isinstance(image, Tensor) and image.is_floating_point():
            pixel_values = image
        elif self.batch_transform:
            pixel_values = self._eval_transform()(image)
        else:
            from ..training.preprocess import TINYVIT_MEAN, TINYVIT_STD, images_to_pixel_values
            bb = self.tinyvit_model.backbone
            # timm's published default_cfgs (timm/models/tiny_vit.py; timm itself is not in the image): crop_pct 0.95 for the 224 variants, 1.0 for the 384 one,
            # 1.0 with crop_mode "squash" for the 512 one; bicubic everywhere
            # (keyed on the variant's own size: an ``img_size=`` override changes the target side, not the checkpoint's transform)
            native = VARIANTS[bb.model_name]["img_size"]
            crop = 0.95 if native == 224 else 1.0
            pixel_values = images_to_pixel_values(image, bb.img_size, TINYVIT_MEAN, TINYVIT_STD, bb.flat_params.device, crop_pct=crop, pipeline="timm",
                                                  crop_mode="squash" if native == 512 else "center")
        with torch.no_grad():
            return self.tinyvit_model(pixel_values=pixel_values).pooler_output

    def forward(self, image, **kwargs) -> Tensor:
        if "image_2" not in kwargs:
            return self._get_embedding(image)
        views = [image] + [kwargs[c] for c in ("image_2", "image_3", "image_4")]
        if self.batch_transform:
            views = _transform_views(views, self._eval_transform())
        return torch.stack([self._get_embedding(v) for v in views], dim=1)


def _host_raw_list(v):
    """A view's raw host images as a list of (H, W, 3) uint8 tensors, or None when the view keeps its own path (float tensors are pixel_values already; a device
    tensor is transformed where it lives)."""
    from ..training.preprocess import _rgb_hwc
    if isinstance(v, Tensor):
        if v.is_floating_point() or v.is_cuda or v.dtype != torch.uint8 or v.dim() not in (3, 4):
            return None
        return [im.permute(1, 2, 0).contiguous() for im in (v if v.dim() == 4 else v.unsqueeze(0))]
    return [_rgb_hwc(im) for im in (v if isinstance(v, (list, tuple)) else [v])]


def _transform_views(views, transform):
    """The panorama views' raw host images through ONE transform call: they are joined into one list, transformed together and handed back as per-view
    ``pixel_values``."""
    from ..training.jpeg import is_file_bytes_list
    if all(is_file_bytes_list(v) for v in views):         # JPEG files as bytes: one device decode and one transform call for all the views
        pv, out, at = transform([f for v in views for f in v]), [], 0
        for v in views:
            out.append(pv[at:at + len(v)]); at += len(v)
        return out
    lists = [_host_raw_list(v) for v in views]
    flat = [im.numpy() for l in lists if l is not None for im in l]
    if not flat:
        return views
    pv, out, at = transform(flat), [], 0
    for v, l in zip(views, lists):
        out.append(v if l is None else pv[at:at + len(l)])
        at += 0 if l is None else len(l)
    return out
