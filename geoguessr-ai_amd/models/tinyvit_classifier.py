"""Drop-in for ``timm.create_model("tiny_vit_*", num_classes=C)`` as the reference's ``finetune_tinyvit/`` stage uses it
(``train_tinyvit_timm.py:122-124``: the country classifier; ``extract_embeddings.py:52-82``: the feature export): same ``forward(x) -> logits``,
``forward_features(x) -> (B, C3, H, W)``, same state-dict keys (the backbone's timm names plus ``head.fc.weight`` / ``head.fc.bias``).

The encoder is the HIP runtime of ``TinyVitBackbone`` (one flat parameter buffer, one C call per forward / backward); ``head.fc`` is a Linear on the GEMMs of
the active precision (``gg_gemm_nt_f32`` in the fp32 and fp32_split modes -- at a few rows it is far below the split GEMMs' routing threshold --, the bf16
MFMA ``gg_gemm_nt`` in the bf16 mode), its weight gradient ``gg_gemm_tn*``, its bias gradient ``gg_colsum*``.  Loss and metrics are the fused
``gg_cls_head`` kernel (``csrc/cls_head.hip``).  The reference's fp16 autocast + GradScaler have no counterpart: the precision modes are fp32 / fp32_split / bf16,
unscaled.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Optional

import torch
import torch.nn as nn
from torch.nn.modules.module import _IncompatibleKeys

from .. import _lib as L
from .. import ops
from .tinyvit import TinyVitBackbone, check_attention16, check_attention16_train

BF16, F32 = torch.bfloat16, torch.float32


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


class _FcFn(torch.autograd.Function):
    """``head.fc``: logits = emb . W^T + b.  The logits live in a (B, pad8(C)) f32 buffer (the GEMMs' leading dimensions) and are returned as its
    (B, C) column slice; the gradient comes back in the same layout and is padded with zero columns before the three gradient launches."""

    @staticmethod
    def forward(ctx, emb: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, bf16: bool):
        L.require_gpu()
        x = emb.to(F32).contiguous()
        B, D = x.shape
        Cn, Cp = weight.shape[0], _pad8(weight.shape[0])
        w = weight.detach().contiguous()
        logits = torch.empty((B, Cp), dtype=F32, device=x.device)
        wt = None
        if bf16:      # bf16 MFMA operands, f32 accumulation and f32 logits (the SuperGuessr head's bf16 form)
            xa = torch.empty((B, D), dtype=BF16, device=x.device)
            L.check(L.lib().gg_cast_f32_to_bf16(L.ptr(x), L.ptr(xa), B * D, L.stream()), "gg_cast_f32_to_bf16")
            wn = torch.empty((Cn, D), dtype=BF16, device=x.device)
            wt = torch.zeros((D, Cp), dtype=BF16, device=x.device)
            L.check(L.lib().gg_cast_transpose_f32(L.ptr(w, F32, "head.fc.weight"), Cn, D, L.ptr(wn), D, L.ptr(wt), Cp, L.stream()), "gg_cast_transpose_f32")
            ops.gemm_nt(xa, wn, bias=bias.detach(), out_f32=True, out=logits, N=Cn, ldc=Cp)
        else:
            xa = x
            ops.gemm_nt(x, w, bias=bias.detach(), out=logits, N=Cn, ldc=Cp)
        ctx.save_for_backward(xa, w if wt is None else wt)
        ctx.dims, ctx.bf16 = (B, D, Cn, Cp), bf16
        return logits[:, :Cn]

    @staticmethod
    def backward(ctx, g):
        xa, w = ctx.saved_tensors
        B, D, Cn, Cp = ctx.dims
        dev = xa.device
        gp = torch.zeros((B, Cp), dtype=F32, device=dev)
        gp[:, :Cn].copy_(g)
        if ctx.bf16:
            g16 = torch.empty((B, Cp), dtype=BF16, device=dev)
            L.check(L.lib().gg_cast_f32_to_bf16(L.ptr(gp), L.ptr(g16), B * Cp, L.stream()), "gg_cast_f32_to_bf16")
            gp, wt = g16, w                                                              # (D, Cp) bf16, pad columns zero
        else:
            wt = torch.zeros((D, Cp), dtype=F32, device=dev)
            L.check(L.lib().gg_transpose_f32(L.ptr(w, F32, "head.fc.weight"), Cn, D, L.ptr(wt), Cp, L.stream()), "gg_transpose_f32")
        demb = dW = db = None
        if ctx.needs_input_grad[0]:
            demb = ops.gemm_nt(gp, wt, K=Cp, out_f32=True)                                  # (B, D) f32 = dlogits . W
        if ctx.needs_input_grad[1]:
            dW = ops.gemm_tn(gp, xa)[:Cn]                                                  # (C, D) f32 = dlogits^T . emb (the pad rows are zero)
        if ctx.needs_input_grad[2]:
            db = ops.colsum_bf16(gp)[:Cn]
        return demb, dW, db, None


class _ClsLossFn(torch.autograd.Function):
    """Mean cross-entropy + rank of the label (``gg_cls_head``).  The forward leaves no gradient behind; the backward runs the kernel once more for
    d(mean loss)/d(logits) with the incoming gradient multiplied in on the device (no host read of a device scalar, no elementwise pass afterwards)."""

    @staticmethod
    def forward(ctx, logits: torch.Tensor, labels: torch.Tensor):
        r = ops.cls_head(logits, labels, want_preds=False)
        ctx.save_for_backward(logits, labels)
        ctx.mark_non_differentiable(r["rank"])
        return r["loss"].view(()), r["rank"]

    @staticmethod
    def backward(ctx, g_loss, _g_rank):
        logits, labels = ctx.saved_tensors
        up = g_loss.to(F32).reshape(1).contiguous()
        r = ops.cls_head(logits, labels, upstream=up, want_loss=False, want_dlogits=True, want_rank=False, want_preds=False)
        return r["dlogits"][:, :logits.shape[1]], None


class _Fc(nn.Module):
    """Parameter holder with nn.Linear's state-dict keys, initialised as timm's NormMlpClassifierHead does through TinyVit._init_weights:
    trunc_normal(std .02), zero bias."""

    def __init__(self, in_features: int, out_features: int, generator: Optional[torch.Generator] = None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        w = torch.empty(out_features, in_features)
        nn.init.trunc_normal_(w, std=0.02, generator=generator)
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(out_features))


class _Head(nn.Module):
    def __init__(self, fc: _Fc):
        super().__init__()
        self.fc = fc


class TinyViTClassifier(nn.Module):
    """``overrides`` as ``TinyViTAdapter``: ``precision`` ("fp32" | "fp32_split" | "bf16"; default ``$GG_PRECISION`` or fp32), ``seed``, ``drop_path_rate``,
    ``grad_checkpointing``, ``img_size``, ``attention16`` (bf16 only: the inference forward's windows beyond 256 tokens on the 16-bit MFMA), ``attention16_train`` (bf16 only: the training step's), ``deterministic_bias_grad`` (every precision: the ``attention_biases`` gradients in a fixed order of adds, include/gg_attn_dbias.h) ...  ``pretrained=True`` cannot download: ``$GG_PRETRAINED_DIR/<model_name>.pt`` (a timm state dict, any head size)
    is loaded with ``strict=False`` when it exists, otherwise a warning is issued and the timm initialisation stands."""

    def __init__(self, model_name: str = "tiny_vit_5m_224", num_classes: int = 1000, pretrained: bool = False, **overrides):
        super().__init__()
        if int(num_classes) < 1:
            raise ValueError(f"num_classes={num_classes}: the classifier needs at least one class (TinyViTAdapter is the num_classes=0 form)")
        if overrides.get("features_only"):
            raise ValueError("features_only belongs to TinyViTAdapter; the classifier exports features through forward_features / pooled_features")
        check_attention16(overrides.get("attention16", False), overrides.get("precision"), "TinyViTClassifier")
        check_attention16_train(overrides.get("attention16_train", False), overrides.get("precision"), "TinyViTClassifier")
        self.backbone = TinyVitBackbone(model_name, **overrides)
        self.num_classes, self.num_features = int(num_classes), self.backbone.num_features
        seed = overrides.get("seed")
        g = torch.Generator().manual_seed((torch.initial_seed() if seed is None else seed) + 1)
        self.head = _Head(_Fc(self.num_features, self.num_classes, g))
        self._backbone_eval = False
        if pretrained:
            d = os.environ.get("GG_PRETRAINED_DIR")
            path = os.path.join(d, model_name + ".pt") if d else None
            if path and os.path.exists(path):
                self.load_state_dict(torch.load(path, map_location="cpu"), strict=False)
            else:
                warnings.warn(f"pretrained weights for {model_name} not available offline (set GG_PRETRAINED_DIR); using the timm initialisation")

    precision = property(lambda self: self.backbone.precision)

    # ---- timm's state-dict contract: the backbone's keys carry no prefix, the classifier's Linear is head.fc ------------------------------
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = self.backbone.state_dict(destination=destination, prefix=prefix, keep_vars=keep_vars)
        return self.head.state_dict(destination=sd, prefix=prefix + "head.", keep_vars=keep_vars)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """A timm checkpoint of any head size: with ``strict=False`` a ``head.fc`` of another shape is skipped (torch itself raises on a shape mismatch
        whatever ``strict`` says; the reference's loaders filter by shape first, inference.py) and reported among the missing keys."""
        fc_keys = ("head.fc.weight", "head.fc.bias")
        own = {"head.fc.weight": self.head.fc.weight, "head.fc.bias": self.head.fc.bias}
        body = {k: v for k, v in state_dict.items() if k not in fc_keys}
        missing, unexpected = [], []
        for k in fc_keys:
            v = state_dict.get(k)
            if v is None or tuple(v.shape) != tuple(own[k].shape):
                if strict:
                    raise RuntimeError(f"TinyViTClassifier.load_state_dict: {k} is {'missing' if v is None else f'{tuple(v.shape)}, expected {tuple(own[k].shape)}'}")
                missing.append(k)
            else:
                with torch.no_grad():
                    own[k].copy_(v)
        r = self.backbone.load_state_dict(body, strict=strict)
        return _IncompatibleKeys(list(r.missing_keys) + missing, list(r.unexpected_keys) + unexpected)

    # ---- freeze policies ------------------------------------------------------------------------------------------------------------------
    def freeze_all_but_last_stage(self):
        """The reference's TinyViT policy (models/tinyvit.py:100-111): stages 0-2 frozen; patch_embed, the last stage and the head train."""
        for m in list(self.backbone._modules["stages"])[:-1]:
            for p in m.parameters():
                p.requires_grad = False
        return self

    def freeze_backbone(self, eval_mode: bool = True):
        """Linear probing: only ``head.fc`` trains; ``eval_mode`` keeps the encoder on its running BatchNorm statistics through ``train()``."""
        for p in self.backbone.parameters():
            p.requires_grad = False
        self._backbone_eval = bool(eval_mode)
        if eval_mode:
            self.backbone.train(False)
        return self

    def unfreeze_all(self):
        for p in self.parameters():
            p.requires_grad = True
        self._backbone_eval = False
        self.backbone.train(self.training)
        return self

    def train(self, mode: bool = True):
        super().train(mode)
        if self._backbone_eval:
            self.backbone.train(False)
        return self

    def set_grad_checkpointing(self, enable: bool = True):
        self.backbone.set_grad_checkpointing(enable)
        return self

    # ---- forward --------------------------------------------------------------------------------------------------------------------------
    def _check_device(self):
        if not self.head.fc.weight.is_cuda:
            raise L.GgError("TinyViTClassifier parameters are on the CPU; call .to('cuda') -- there is no CPU fallback")

    def forward_head(self, embedding: torch.Tensor) -> torch.Tensor:
        """timm's ``forward_head`` after pool + norm: (B, num_features) -> logits (B, C)."""
        self._check_device()
        return _FcFn.apply(embedding, self.head.fc.weight, self.head.fc.bias, self.backbone.precision == "bf16")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_device()
        return self.forward_head(self.backbone(x))

    def loss_and_metrics(self, logits: torch.Tensor, labels: torch.Tensor):
        """-> (mean cross-entropy, rank int32 (B,)): top-1 hit <=> rank < 1, top-k hit <=> rank < k.  A label outside [0, C) makes the loss NaN."""
        if logits.dim() != 2 or logits.stride(1) != 1 or logits.dtype != F32:
            logits = logits.to(F32).contiguous()
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous().view(-1)
        if labels.numel() != logits.shape[0]:
            raise L.GgError(f"loss_and_metrics: {labels.numel()} labels for {logits.shape[0]} rows of logits")
        return _ClsLossFn.apply(logits, labels)

    # ---- feature export (inference only: the reference calls both under no_grad on an eval() model) -----------------------------------------
    def _export_input(self, x: torch.Tensor, what: str) -> torch.Tensor:
        self._check_device()
        if self.backbone.training:
            raise L.GgError(f"{what} is the feature export of an eval() model (running BatchNorm statistics, no autograd); call .eval() first")
        return x

    @torch.no_grad()
    def pooled_features(self, x: torch.Tensor) -> torch.Tensor:
        """(B, num_features) f32: the spatial mean of the last stage's map WITHOUT head.norm -- what ``extract_embeddings.forward_to_emb`` computes from
        ``forward_features`` and what a ``features_only`` TinyViTAdapter yields; same parameters, weight cache and workspace as ``forward``."""
        return self.backbone.forward_hip(self._export_input(x, "pooled_features"), False, None, features_only=True)

    @torch.no_grad()
    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        """timm's contract: the last stage's feature map (B, C3, H, W) f32 (a copy: the workspace region is reused by the next forward)."""
        bb = self.backbone
        bb.forward_hip(self._export_input(x, "forward_features"), False, None, features_only=True)
        B = x.shape[0]
        off, nbytes, res, ch = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        L.check(L.lib().gg_tinyvit_last_map_info(C.byref(bb.cfg), B, C.byref(off), C.byref(nbytes), C.byref(res), C.byref(ch)), "gg_tinyvit_last_map_info")
        raw = bb._ws[False][off.value:off.value + nbytes.value]
        if bb.precision == "bf16":
            fmap = torch.empty((B, res.value, res.value, ch.value), dtype=F32, device=raw.device)
            L.check(L.lib().gg_cast_bf16_to_f32(L.ptr(raw), L.ptr(fmap), fmap.numel(), L.stream()), "gg_cast_bf16_to_f32")
        else:
            fmap = raw.view(F32).view(B, res.value, res.value, ch.value).clone()
        return fmap.permute(0, 3, 1, 2)
