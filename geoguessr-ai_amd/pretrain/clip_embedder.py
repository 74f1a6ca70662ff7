"""Drop-in for the reference's ``pretrain/clip_embedder.py`` (``CLIPEmbedding``, :10-101) plus the HIP vision tower it wraps
(``CLIPVisionTower``: transformers ``CLIPVisionModel`` semantics and state-dict keys, ``csrc/clip.hip``).

* ``CLIPEmbedding``: frozen, inference only -- ``forward`` returns ``last_hidden_state.mean(dim=1)`` (:63-65); panorama kwargs
  ``image, image_2..4`` stack on dim 1 (:94-101).  Float tensors are pixel_values; PIL images / uint8 arrays or tensors go through the
  processor's tensor side on the device (``clip_preprocess``).
* ``CLIPVisionTower``: the base model of ``SuperGuessr`` for CLIP runs (models/super_guessr.py:134-150: ``config._name_or_path`` contains
  "clip-vit", ``config.hidden_size``, ``vision_model.encoder.layers``).  It trains: the whole forward and backward are one C call each
  (``gg_clip_forward`` / ``gg_clip_backward``), parameters are views into one flat fp32 buffer like the TinyViT backbone's, so
  ``optim.AdamW`` and the RCCL gradient exchange treat both encoders alike.  ``gradient_checkpointing_enable()`` (HF's call) turns on
  activation recompute (``GgClipCfg.recompute``): the workspace keeps each trained layer's input instead of its eight activations.

Arithmetic: ``precision="fp32"`` (default; the reference runs the tower in fp32), ``"fp32_split"`` (f32 storage, every GEMM and the attention as
f32-accurate split-bf16 products: ``GgClipCfg.act_dtype`` 3), ``"bf16"``, ``"fp16"`` (inference only: the precision BASELINE
config c4 names), or ``"fp8"`` (inference only: fp16's storage and schedule with the four Linears of every encoder layer as W8A8 e4m3 products,
``GgClipCfg.act_dtype`` 8, include/gg_fp8.h; resolved by ``tower_precision_code``); the default is ``$GG_PRECISION``.  ``attention16=True`` (bf16, fp16 and fp8; opt-in,
not in the reference): the inference forward of a tower beyond 256 tokens (ViT-L/14-336: 577) runs its attention with both products on the 16-bit MFMA
(``gg_attention_flash16_fwd``, include/gg_attn16.h) instead of the f32-MFMA online-softmax kernel; training forwards are unaffected.  ``attention16_train=True`` (bf16 only; opt-in, not in the reference, independent of
``attention16``): the TRAINING step of such a tower -- the training forward, the recompute replay and the attention backward -- runs on the 16-bit MFMA
(``gg_attention_flash16_fwd`` / ``gg_attention_flash16_bwd``, include/gg_attn16b.h).  ``interpolate_pos_encoding=True`` (transformers' keyword; opt-in, as a
tower default or per call): pixel_values of another size than ``image_size`` run on the position table resampled to their grid (include/gg_clip_interp.h).  No hub download: weights come from a
state dict (HF names, with or without the leading ``vision_model.``)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Optional

import torch
from torch import Tensor, nn

from .. import _lib as L
from ..models.flat import EncoderNode, EncoderRuntime

CLIP_CONFIGS = {
    "openai/clip-vit-base-patch32": dict(hidden_size=768, intermediate_size=3072, num_layers=12, num_heads=12, image_size=224, patch_size=32),
    "openai/clip-vit-large-patch14-336": dict(hidden_size=1024, intermediate_size=4096, num_layers=24, num_heads=16, image_size=336, patch_size=14),
}
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # CLIPProcessor's image_mean / image_std (openai/clip-vit-*)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_NAMES = {0: "bf16", 1: "fp32", 2: "fp16", 3: "fp32_split", 8: "fp8"}      # GgClipCfg.act_dtype -> the name ``.precision`` reports


def _precision_code(precision: Optional[str]) -> int:
    from ..models.tinyvit import PRECISIONS, default_precision
    p = precision or default_precision()
    if p in ("fp16", "f16", "float16", "half"):
        return 2                      # CLIP only, inference only (BASELINE config c4: "MFMA fp16")
    if p not in PRECISIONS:
        raise ValueError(f"precision='{p}' (known: bf16, fp16, fp32, fp32_split)")
    return PRECISIONS[p]


FP8_CODE = 8                          # GG_CLIP_ACT_FP8 (include/gg_fp8.h)


def tower_precision_code(precision: Optional[str]) -> int:
    """``_precision_code`` plus the one name only the VISION tower takes: ``"fp8"`` / ``"e4m3"`` (inference only: W8A8 e4m3 Linears on fp16 storage).  The name is
    an explicit argument only: ``$GG_PRECISION`` and ``_precision_code`` (shared with the text tower's callers) keep refusing it."""
    if precision in ("fp8", "e4m3"):
        return FP8_CODE
    try:
        return _precision_code(precision)
    except ValueError as e:
        raise ValueError(f"{e}; CLIPVisionTower / CLIPEmbedding also take fp8") from None


def check_attention16(attention16: bool, code: int, who: str) -> None:
    """``attention16=True`` is a switch of the 16-bit modes: refused by name for ``fp32`` and ``fp32_split`` (their attention is f32-accurate by contract)."""
    if attention16 and code in (1, 3):
        raise L.GgError(f"{who}: attention16=True is a switch of the bf16, fp16 and fp8 modes; precision='{PRECISION_NAMES[code]}' keeps its f32-accurate attention "
                        "(leave attention16 off)")


def check_attention16_train(attention16_train: bool, code: int, who: str) -> None:
    """``attention16_train=True`` is a switch of the bf16 training step: refused by name for ``fp32`` and ``fp32_split`` (their attention is f32-accurate by
    contract) and for ``fp16`` and ``fp8`` (inference-only modes: they have no training step)."""
    if attention16_train and code in (1, 3):
        raise L.GgError(f"{who}: attention16_train=True is a switch of the bf16 mode; precision='{PRECISION_NAMES[code]}' keeps its f32-accurate attention "
                        "(leave attention16_train off)")
    if attention16_train and code != 0:
        raise L.GgError(f"{who}: attention16_train=True is a switch of the bf16 mode; precision='{PRECISION_NAMES[code]}' is inference-only (attention16 is the "
                        "switch of its forward)")


class _VisionModel(EncoderRuntime):
    """``vision_model`` of the HF module tree: owner of the flat storage and of the HIP workspace.  Its children (``embeddings``, ``pre_layrnorm``,
    ``encoder.layers.N....``, ``post_layernorm``) are rebuilt from the tensor names, so ``encoder.layers[i].parameters()`` is what
    ``SuperGuessr._freeze_params`` expects."""
    _name, _switch = "CLIP", "gradient_checkpointing"
    _mask_changed = "requires_grad changed between the CLIP forward and its backward; run the forward again"
    _toggled_gen = None               # generation of a training forward that a gradient_checkpointing toggle made the runtime forget
    attention16 = False               # CLIPVisionTower(attention16=True): this tower's forwards run with gg_clip_set_attention16(1)
    attention16_train = False         # CLIPVisionTower(attention16_train=True): its training forwards and backwards run with gg_clip_set_attention16_train(1)
    _hw = (0, 0)                      # GgClipCfg.input_h / input_w of the call at hand ((0, 0): the native size); the weight cache holds the position table resampled for it
    _wc_hw = (0, 0)                   # ... and the size the weight cache was last rebuilt for

    def __init__(self, cfg: L.ClipCfg, seed: int):
        super().__init__()
        self.cfg = cfg
        self.precision = PRECISION_NAMES[cfg.act_dtype]
        self.split = cfg.act_dtype == 3
        lib = L.lib()
        n = lib.gg_clip_num_tensors(C.byref(cfg))
        if n < 0:
            raise L.GgError(lib.gg_last_error().decode())
        self.table = []
        name = C.create_string_buffer(256)
        off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int()
        shape = (C.c_int64 * 4)()
        for i in range(n):
            L.check(lib.gg_clip_tensor_info(C.byref(cfg), i, name, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape), "gg_clip_tensor_info")
            self.table.append(dict(name=name.value.decode(), offset=off.value, numel=numel.value, shape=tuple(shape[j] for j in range(ndim.value)),
                                   kind=0, index=i))
        self.param_floats = lib.gg_clip_param_floats(C.byref(cfg))
        self.buffer_floats, self.num_counters = 0, 0
        g = torch.Generator().manual_seed(seed)

        def init(name, shape):
            if name.endswith(("norm.weight", "norm1.weight", "norm2.weight")):
                return torch.ones(shape)
            if name.endswith(".bias"):
                return torch.zeros(shape)
            return torch.randn(shape, generator=g) * 0.02
        self._register_table(init)

    def _cfg_at(self, hw) -> L.ClipCfg:
        """``self.cfg`` with ``input_h`` / ``input_w`` of a call ((0, 0): the native size -- the struct as it is)."""
        c = L.ClipCfg.from_buffer_copy(self.cfg)
        c.input_h, c.input_w = hw
        return c

    def _call_size(self, x: Tensor, interpolate: bool):
        """(input_h, input_w) of ``GgClipCfg`` for these pixel_values: (0, 0) at the native size; a foreign size needs ``interpolate_pos_encoding``."""
        S, P = self.cfg.image_size, self.cfg.patch_size
        native = x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == S and x.shape[3] == S
        if native:
            return (0, 0)
        if not interpolate or x.dim() != 4 or x.shape[1] != 3:
            raise L.GgError(f"CLIPVisionTower expects (B,3,{S},{S}) pixel_values, got {tuple(x.shape)}")
        H, W = int(x.shape[2]), int(x.shape[3])
        if H < P or W < P or H % P or W % P:
            raise L.GgError(f"CLIPVisionTower(interpolate_pos_encoding=True): input size {H} x {W} is not a multiple of the patch size {P}")
        return (H, W)

    def _set_call_size(self, hw):
        """The weight cache carries the position table of ONE call size in its last region.  A cache too small for this size's table is let go (``_ensure_weights``
        allocates and rebuilds it whole); otherwise ``_sync_table`` rebuilds the table alone."""
        self._hw = hw
        if hw != self._wc_hw and self._wcache is not None and self._wcache.numel() < self._wcache_bytes():
            self._wcache = None

    def _sync_table(self):
        """After ``_ensure_weights``: the cache is current for the parameters; if its table is another call size's, resample the table alone
        (``gg_clip_pos_interp_fwd`` into the cache's last region, whose offset is the native cache's size: include/gg.h, ``GgClipCfg.input_h``)."""
        if self._hw == self._wc_hw:
            return
        if self._hw != (0, 0):
            from .. import ops
            P, D = self.cfg.patch_size, self.cfg.hidden_size
            gh, gw = self._hw[0] // P, self._hw[1] // P
            off = L.lib().gg_clip_wcache_bytes(C.byref(self.cfg))
            region = self._wcache[off:off + (gh * gw + 1) * D * 4].view(torch.float32).view(gh * gw + 1, D)
            ops.clip_pos_interp(self._params["embeddings.position_embedding.weight"].data, (gh, gw), out=region)
        self._wc_hw = self._hw

    def _wcache_bytes(self) -> int:
        n = L.lib().gg_clip_wcache_bytes(C.byref(self._cfg_at(self._hw)))
        if n < 0:
            raise L.GgError(L.lib().gg_last_error().decode())
        return n

    def _refresh(self, only):             # (no masked refresh: the whole cache is rebuilt, in the fp32_split mode the bf16 planes with it)
        L.check(L.lib().gg_clip_refresh_weights(C.byref(self._cfg_at(self._hw)), L.ptr(self._flat), L.ptr(self._wcache), L.stream()), "gg_clip_refresh_weights")
        self._wc_hw = self._hw

    def _workspace_bytes(self, batch: int, training: bool, mask) -> int:
        return L.lib().gg_clip_workspace_bytes(C.byref(self._cfg_at(self._hw)), batch, int(training), mask)

    def set_recompute(self, enable: bool) -> bool:
        changed = super().set_recompute(enable)
        if changed and self._last is not None:
            self._last, self._toggled_gen = None, self._gen
        return changed

    def _pending(self, gen, batch=None):
        if self._last is None and self._toggled_gen == self._gen:
            raise L.GgError(f"gradient checkpointing was toggled since the training forward (now recompute={self.cfg.recompute}): its workspace was "
                            "released, the other layout keeps other tensors; run the forward again")
        return super()._pending(gen, batch)

    def forward_hip(self, x: Tensor, training: bool, return_last_hidden: bool, interpolate_pos_encoding: bool = False):
        """``interpolate_pos_encoding``: a (B,3,H,W) input of another size than ``image_size`` (H, W multiples of the patch size) runs on the position table
        resampled to its grid (``GgClipCfg.input_h`` / ``input_w``); without it such an input is refused.  The workspaces (one per ``training`` flag) grow to
        the largest call; the record of a training forward carries its size, and its backward runs at that size."""
        L.require_gpu()
        if not self._flat.is_cuda:
            raise L.GgError("CLIPVisionTower parameters are on the CPU; call .to('cuda') -- there is no CPU fallback")
        hw = self._call_size(x, interpolate_pos_encoding)
        cfg = self._cfg_at(hw)
        S, P = self.cfg.image_size, self.cfg.patch_size
        x = x.to(device=self._flat.device, dtype=torch.float32).contiguous()
        B = x.shape[0]
        self._set_call_size(hw)
        mask, ws = self._prepare(B, training)
        self._sync_table()
        D, T = self.cfg.hidden_size, ((hw[0] // P) * (hw[1] // P) if hw != (0, 0) else (S // P) ** 2) + 1
        out = torch.empty((B, D), dtype=torch.float32, device=x.device)
        last = torch.empty((B, T, D), dtype=torch.float32, device=x.device) if return_last_hidden else None
        lib = L.lib()
        prev = lib.gg_clip_set_attention16(1) if self.attention16 else None      # process-wide switch, read when the forward is enqueued: set for this call only
        prev_t = lib.gg_clip_set_attention16_train(1) if self.attention16_train and training else None      # the same, the training step's switch
        try:
            rc = lib.gg_clip_forward(C.byref(cfg), B, int(training), L.ptr(self._flat), L.ptr(self._wcache), L.ptr(x), L.ptr(ws), L.ptr(out),
                                     L.ptr(last), mask, L.stream())
        finally:
            if prev is not None:
                lib.gg_clip_set_attention16(prev)
            if prev_t is not None:
                lib.gg_clip_set_attention16_train(prev_t)
        L.check(rc, "gg_clip_forward")
        if training:
            self._record_forward(B, mask, payload=hw)
        return out, last

    def backward_hip(self, d_out: Optional[Tensor], d_last: Optional[Tensor], gen: int):
        B, hw, ws = self._pending(gen)
        mask = self._same_mask()
        cfg = self._cfg_at(hw)      # the size of ITS forward (the backward reads no position table: an eval forward at another size in between changes nothing)
        fg = self.attach_grads()
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        d_out, d_last = f(d_out), f(d_last)
        lib = L.lib()
        prev_t = lib.gg_clip_set_attention16_train(1) if self.attention16_train else None      # read when the backward is enqueued (its recompute replay included)
        try:
            rc = lib.gg_clip_backward(C.byref(cfg), B, L.ptr(self._flat), L.ptr(self._wcache), L.ptr(ws), L.ptr(d_out), L.ptr(d_last), L.ptr(fg), mask,
                                      L.stream())
        finally:
            if prev_t is not None:
                lib.gg_clip_set_attention16_train(prev_t)
        L.check(rc, "gg_clip_backward")
        if self._grad_ready_hook is not None:          # (no stage callback in the CLIP backward: the buckets leave after it)
            self._grad_ready_hook(0, self.param_floats)


class CLIPVisionTower(nn.Module):
    supports_gradient_checkpointing = True          # (transformers PreTrainedModel's class attribute)

    def __init__(self, model_name: str = "openai/clip-vit-base-patch32", seed: int = 0, precision: Optional[str] = None,
                 gradient_checkpointing: bool = False, attention16: bool = False, attention16_train: bool = False, interpolate_pos_encoding: bool = False,
                 **cfg_overrides):
        """``interpolate_pos_encoding`` (transformers' ``CLIPVisionModel.forward`` keyword, here also a tower default for callers that pass ``pixel_values`` alone,
        as ``SuperGuessr`` does): pixel_values of another size than ``image_size`` -- any (H, W) of patch multiples, square or not -- run on the pretrained
        position table resampled to their grid (bicubic, the class row kept; include/gg_clip_interp.h), gradients flowing back into the table.  Off: such
        input is refused, as before.  ``image_size`` keeps naming the size the weights were trained at.

        ``attention16_train=True`` (bf16 only; opt-in, independent of ``attention16``): this tower's training steps run with
        ``gg_clip_set_attention16_train(1)`` -- with more than 256 tokens the training forward, the recompute replay and the attention backward go through
        ``gg_attention_flash16_fwd`` / ``gg_attention_flash16_bwd`` (include/gg_attn16b.h); inference forwards are unaffected."""
        super().__init__()
        kw = dict(CLIP_CONFIGS.get(model_name, CLIP_CONFIGS["openai/clip-vit-base-patch32"]))
        kw.update(cfg_overrides)
        check_attention16(attention16, tower_precision_code(precision), "CLIPVisionTower")
        check_attention16_train(attention16_train, tower_precision_code(precision), "CLIPVisionTower")
        c = L.ClipCfg()
        c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads = kw["hidden_size"], kw["intermediate_size"], kw["num_layers"], kw["num_heads"]
        c.image_size, c.patch_size, c.ln_eps = kw["image_size"], kw["patch_size"], 1e-5
        c.act_dtype = tower_precision_code(precision)
        c.recompute = int(bool(gradient_checkpointing))
        self.cfg = c
        self.precision = PRECISION_NAMES[c.act_dtype]
        self.config = SimpleNamespace(hidden_size=kw["hidden_size"], _name_or_path=model_name, **{k: v for k, v in kw.items() if k != "hidden_size"})
        self.vision_model = _VisionModel(c, seed)
        self.attention16 = self.vision_model.attention16 = bool(attention16)
        self.attention16_train = self.vision_model.attention16_train = bool(attention16_train)
        self.interpolate_pos_encoding = bool(interpolate_pos_encoding)
        self.num_tokens = (c.image_size // c.patch_size) ** 2 + 1      # (at the native size)

    # ---- activation recompute -----------------------------------------------------------------------------------------------------------
    @property
    def is_gradient_checkpointing(self) -> bool:
        return bool(self.cfg.recompute)

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        """transformers' switch (``model.gradient_checkpointing_enable()``): activation recompute of the training step (``GgClipCfg.recompute``,
        include/gg.h).  The workspace keeps the input of every encoder layer from the first trainable one up; the backward re-forms a layer's
        other tensors (LayerNorm outputs, qkv, attention output, the MLP activations) right before its backward.  ``pooled_mean``,
        ``last_hidden_state`` and every gradient are bit-identical to the step without recompute.  ``gradient_checkpointing_kwargs`` (HF's
        ``use_reentrant``) has no counterpart here and is ignored.  Inference ignores the setting."""
        self.vision_model.set_recompute(True)

    def gradient_checkpointing_disable(self):
        self.vision_model.set_recompute(False)

    # ---- weights ----------------------------------------------------------------------------------------------------------------------
    @property
    def backbone(self):          # same attribute name as TinyViTAdapter's flat-storage owner (SuperGuessr reads .backbone.precision)
        return self.vision_model

    def named_views(self) -> Dict[str, Tensor]:
        return {n: p.data for n, p in self.vision_model.named_parameters()}

    def load_hf_state_dict(self, sd: Dict[str, Tensor]):
        """HF ``CLIPVisionModel`` keys; a leading ``vision_model.`` (transformers 4.x nesting) is stripped.  Unknown keys (``position_ids``) are ignored."""
        views = self.named_views()
        with torch.no_grad():
            for k, v in sd.items():
                k = k[len("vision_model."):] if k.startswith("vision_model.") else k
                if k in views:
                    views[k].copy_(torch.as_tensor(v).to(views[k].device, torch.float32))
        self.vision_model.mark_params_dirty()

    def forward_hip(self, x: Tensor, training: bool, return_last_hidden: bool, interpolate_pos_encoding: bool = False):          # (the HIP calls are the vision model's)
        return self.vision_model.forward_hip(x, training, return_last_hidden, interpolate_pos_encoding)

    def backward_hip(self, d_out: Optional[Tensor], d_last: Optional[Tensor], gen: int):
        self.vision_model.backward_hip(d_out, d_last, gen)

    def forward(self, pixel_values: Tensor = None, return_last_hidden: bool = True, interpolate_pos_encoding: Optional[bool] = None):
        """``interpolate_pos_encoding``: ``None`` = the tower's default (the constructor's keyword)."""
        vm = self.vision_model
        interp = self.interpolate_pos_encoding if interpolate_pos_encoding is None else bool(interpolate_pos_encoding)
        need = vm.wants_grad()      # (no dropout / BatchNorm: train and eval compute the same)
        if need and self.precision in ("fp16", "fp8"):
            raise L.GgError(f"CLIPVisionTower(precision='{self.precision}') is inference-only: run under torch.no_grad() / freeze it, or train in fp32 / bf16")
        if not need:
            out, last = vm.forward_hip(pixel_values, False, return_last_hidden, interp)
        else:
            out, last = _ClipFn.apply(vm, pixel_values, vm._anchor(), return_last_hidden, interp)
        return SimpleNamespace(last_hidden_state=last, pooled_mean=out, pooler_output=out)


class _ClipFn(EncoderNode):
    """Whole-tower autograd node (the counterpart of the TinyViT backbone's; ``EncoderRuntime._anchor``)."""

    @staticmethod
    def forward(ctx, vm: _VisionModel, x: Tensor, anchor: Tensor, want_last: bool, interpolate: bool = False):
        out, last = vm.forward_hip(x, True, want_last, interpolate)
        vm._enter_node(ctx)
        ctx.set_materialize_grads(False)          # an unused last_hidden_state must not cost a (B,T,D) zero gradient
        return out, last


def clip_preprocess(images, size: int, device) -> Tensor:
    """``CLIPProcessor(images=image, return_tensors="pt")["pixel_values"]`` (pretrain/clip_embedder.py:55-57) on the device: see
    ``training.preprocess.images_to_pixel_values`` (Pillow bicubic resize of the shortest edge to ``size``, centre crop, * 1/255, CLIP mean / std; the uint8
    image is bit-identical to the processor's, pinned by transformers' own output in tests/golden/preprocess_pil.npz)."""
    from ..training.preprocess import images_to_pixel_values
    return images_to_pixel_values(images, size, CLIP_MEAN, CLIP_STD, device, pipeline="clip")


class CLIPEmbedding(nn.Module):
    def __init__(self, model_name: str = "openai/clip-vit-base-patch32", device: str = "cuda", load_checkpoint: bool = False,
                 panorama: bool = False, state_dict: Optional[Dict[str, Tensor]] = None, precision: Optional[str] = None, batch_transform: bool = False,
                 jpeg_split_bytes: int = 0, attention16: bool = False, jpeg_progressive: bool = False, image_size: Optional[int] = None, **cfg_overrides):
        """``image_size`` (not in the reference): raw images are resized and cropped to this size instead of the tower's own (``DeviceEvalTransform`` /
        ``clip_preprocess`` at that size; a multiple of the patch size) and the tower runs them on its resampled position table
        (``CLIPVisionTower(interpolate_pos_encoding=True)``); the weights keep the size they were trained at.  ``None``: the tower's size.

        ``batch_transform`` (not in the reference): raw images -- a list of any sizes, or the four panorama views together -- go through ONE ``gg_eval_batch``
        call (``training.preprocess.DeviceEvalTransform``) instead of one ``gg_preprocess_pil`` call per image; same arithmetic.  ``jpeg_split_bytes`` (with
        ``batch_transform`` only): the ``split_bytes`` of the decoder that takes JPEG files given as bytes (``DeviceEvalTransform``'s keyword); ``jpeg_progressive`` (with
        ``batch_transform`` only): that decoder's ``progressive`` (progressive files are decoded next to baseline ones; off by default).  ``attention16``:
        ``CLIPVisionTower``'s keyword (opt-in 16-bit-MFMA attention beyond 256 tokens; refused for fp32 / fp32_split)."""
        super().__init__()
        check_attention16(attention16, tower_precision_code(precision), "CLIPEmbedding")
        self.device = device
        self.batch_transform, self._transform = bool(batch_transform), None
        if jpeg_split_bytes and not batch_transform:
            raise ValueError("CLIPEmbedding: jpeg_split_bytes needs batch_transform=True")
        self.jpeg_split_bytes = int(jpeg_split_bytes)
        if jpeg_progressive and not batch_transform:
            raise ValueError("CLIPEmbedding: jpeg_progressive needs batch_transform=True")
        self.jpeg_progressive = bool(jpeg_progressive)
        self.panorama = panorama
        self.clip_model = CLIPVisionTower(model_name if not load_checkpoint else "openai/clip-vit-base-patch32", precision=precision, attention16=attention16,
                                          interpolate_pos_encoding=image_size is not None, **cfg_overrides)
        self.image_size = int(image_size) if image_size is not None else self.clip_model.cfg.image_size      # the size raw images are brought to
        if self.image_size <= 0 or self.image_size % self.clip_model.cfg.patch_size:
            raise ValueError(f"CLIPEmbedding: image_size={image_size} is not a multiple of the patch size {self.clip_model.cfg.patch_size}")
        if load_checkpoint:
            state_dict = torch.load(model_name, map_location="cpu")
            print("Loaded embedder from checkpoint:", model_name)
        if state_dict is not None:
            self.clip_model.load_hf_state_dict({(k.partition(".")[2] if "base_model" in k else k): v for k, v in state_dict.items()})
        self.clip_model = self.clip_model.to(device if isinstance(device, str) else f"cuda:{device}")
        for p in self.clip_model.parameters():          # the embedder is frozen (pretrain/clip_embedder.py:51: torch.no_grad())
            p.requires_grad = False
        self.eval()

    def _eval_transform(self):
        """The processor's tensor side as a batch transform (``batch_transform=True``); it keeps its workspace from call to call."""
        if self._transform is None:
            from ..training.preprocess import DeviceEvalTransform
            self._transform = DeviceEvalTransform(self.image_size, CLIP_MEAN, CLIP_STD, "clip", device=next(self.clip_model.parameters()).device,
                                                  jpeg_split_bytes=self.jpeg_split_bytes, jpeg_progressive=self.jpeg_progressive)
        return self._transform

    def _get_embedding(self, image) -> Tensor:
        """A float tensor is taken as ``pixel_values`` (pretrain/clip_embedder.py:58-59); anything else -- PIL image, uint8 array / tensor, list of
        images -- goes through the processor's tensor side on the device (:55-57)."""
        dev = next(self.clip_model.parameters()).device
        if torch.is_tensor(image) and image.is_floating_point():
            pixel_values = image
        elif self.batch_transform:
            pixel_values = self._eval_transform()(image)
        else:
            pixel_values = clip_preprocess(image, self.image_size, dev)
        with torch.no_grad():
            return self.clip_model(pixel_values=pixel_values, return_last_hidden=False).pooled_mean

    def forward(self, image, **kwargs) -> Tensor:
        if "image_2" not in kwargs:
            return self._get_embedding(image)
        views = [image] + [kwargs[c] for c in ("image_2", "image_3", "image_4")]
        if self.batch_transform:
            from .tinyvit_embedder import _transform_views
            views = _transform_views(views, self._eval_transform())
        return torch.stack([self._get_embedding(v) for v in views], dim=1)
