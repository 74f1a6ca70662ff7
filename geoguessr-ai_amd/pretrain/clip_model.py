"""Drop-in for ``transformers.CLIPModel`` as the reference's contrastive pre-training stage uses it (``pretrain_idun.py:205-300``: everything frozen but
``visual_projection`` and ``logit_scale``, (image, caption) batches with ``return_loss=True``) and as ``tests/test_clip.py`` uses it for zero-shot prompts.

* ``vision_model``: the flat-storage owner of the existing ``CLIPVisionTower`` (``csrc/clip.hip``), trainable under every mask ``gg_clip_backward`` supports,
  gradient checkpointing included.  ``pooler_output = post_layernorm(last_hidden_state[:, 0])`` is formed here from ``gg_layernorm_fwd`` / ``_bwd``.
* ``text_model``: the text tower (``gg_clip_text_forward``: causal attention, final_layer_norm, the row at the EOS position).  By default it is forward only:
  a text tensor that still has ``requires_grad=True`` when a loss is back-propagated raises ``GgError`` naming it.  ``CLIPModel(..., train_text=True)`` /
  ``set_text_training(True)`` opt in to training it (``include/gg_clip_text_train.h``): when grad mode is on and some text tensor requires grad, the forward is
  ``gg_clip_text_forward_train`` (same bits, the layers from the first trained one up keep their activations) behind a whole-tower autograd node whose backward,
  ``gg_clip_text_backward`` (causal attention backward, token-embedding scatter-add, position sum), accumulates into the tower's flat gradient buffer under any
  trainable mask; ``optim.AdamW(model)`` finds the tower through ``trainable_ranges``.  With the switch off, or every text tensor frozen, the five-region
  inference forward runs as before.  No activation recompute for the text tower; the data-parallel exchange of text gradients (``comm.py``) is out of scope.
* ``visual_projection`` / ``text_projection``: bias-free ``nn.Linear``-shaped weights; the projections and their weight gradients are library GEMMs.
* ``logit_scale``: ln(1 / 0.07).  The contrastive head (normalisation, both logit matrices, the symmetric cross-entropy and its whole backward) is one C call,
  ``gg_clip_contrastive``.

``attention_mask`` is accepted and not read: under the causal mask right-padding cannot reach a row at or before the pooled (EOS) position, transformers'
``text_embeds`` with and without it differ by exactly 0 on right-padded input.  No tokenizer, no ``CLIPProcessor``, no HF ``Trainer``; no fp16.
State-dict keys are transformers' (``text_model.*``, ``vision_model.*``, ``visual_projection.weight``, ``text_projection.weight``, ``logit_scale``)."""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Dict, Optional

import torch
from torch import Tensor, nn

from .. import _lib as L
from .. import ops
from ..models.flat import EncoderNode, EncoderRuntime
from .clip_embedder import CLIP_CONFIGS, PRECISION_NAMES, CLIPVisionTower, _precision_code

CLIP_TEXT_CONFIGS = {
    "openai/clip-vit-base-patch32": dict(hidden_size=512, intermediate_size=2048, num_layers=12, num_heads=8, projection_dim=512),
    "openai/clip-vit-large-patch14-336": dict(hidden_size=768, intermediate_size=3072, num_layers=12, num_heads=12, projection_dim=768),
}
TEXT_DEFAULTS = dict(vocab_size=49408, max_positions=77, eos_token_id=2)      # the shipped openai configs (eos_token_id 2: transformers takes the argmax)
LOGIT_SCALE_INIT = math.log(1.0 / 0.07)


def eos_positions(input_ids: Tensor, eos_token_id: int) -> Tensor:
    """transformers' pooling rule (CLIPTextTransformer.forward): ``eos_token_id == 2`` -- the configs shipped before the id was fixed -- takes the argmax of the
    ids (the EOS token has the highest id of the openai vocabulary); otherwise the first position equal to ``eos_token_id``.  int32 (B,)."""
    if eos_token_id == 2:
        return input_ids.to(torch.int32).argmax(dim=-1).to(torch.int32)
    return (input_ids == eos_token_id).to(torch.int32).argmax(dim=-1).to(torch.int32)


def _is_norm_weight(n: str) -> bool:
    return n.endswith(("norm.weight", "norm1.weight", "norm2.weight"))


class _TextModel(EncoderRuntime):
    """``text_model`` of the HF module tree: flat storage, weight cache, the inference workspace and (``train_text``) the training workspace of the text tower."""
    _name, _switch = "CLIP text tower", "text training"
    _mask_changed = "requires_grad changed between the CLIP text forward and its backward for {changed} ...; run the forward again"
    _toggled_gen = None               # generation of a training forward that a set_training toggle made the runtime forget

    def __init__(self, cfg: L.ClipTextCfg, seed: int, eos_token_id: int):
        super().__init__()
        self.cfg = cfg
        self.cfg.recompute = 0            # (a plain attribute, not a field of GgClipTextCfg: the step lifecycle reads it; the text tower has no checkpointing)
        self.train_text = False
        self.eos_token_id = eos_token_id
        self.precision = PRECISION_NAMES[cfg.act_dtype]
        lib = L.lib()
        n = lib.gg_clip_text_num_tensors(C.byref(cfg))
        if n < 0:
            raise L.GgError(lib.gg_last_error().decode())
        self.table = []
        name = C.create_string_buffer(256)
        off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int()
        shape = (C.c_int64 * 4)()
        for i in range(n):
            L.check(lib.gg_clip_text_tensor_info(C.byref(cfg), i, name, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape), "gg_clip_text_tensor_info")
            self.table.append(dict(name=name.value.decode(), offset=off.value, numel=numel.value, shape=tuple(shape[j] for j in range(ndim.value)),
                                   kind=0, index=i))
        self.param_floats = lib.gg_clip_text_param_floats(C.byref(cfg))
        self.buffer_floats, self.num_counters = 0, 0
        g = torch.Generator().manual_seed(seed)

        def init(name, shape):
            if _is_norm_weight(name):
                return torch.ones(shape)
            if name.endswith(".bias"):
                return torch.zeros(shape)
            return torch.randn(shape, generator=g) * 0.02
        self._register_table(init)

    def set_recompute(self, enable: bool) -> bool:      # (nothing to checkpoint: the training forward keeps every tensor its backward reads)
        return False

    def set_training(self, enable: bool) -> bool:
        """The opt-in switch of text-tower training.  True if it changed: the training workspace is released and a pending training forward is forgotten
        (its backward is refused)."""
        changed = bool(enable) != self.train_text
        if changed:
            self.train_text = bool(enable)
            self._ws.pop(True, None)
            if self._last is not None:
                self._last, self._toggled_gen = None, self._gen
        return changed

    def _pending(self, gen, batch=None):
        if self._last is None and self._toggled_gen == self._gen:
            raise L.GgError(f"text training was toggled since the training forward (now train_text={self.train_text}): its workspace was released; "
                            "run the forward again")
        return super()._pending(gen, batch)

    def wants_training(self) -> bool:
        return self.train_text and self.wants_grad()

    def _wcache_bytes(self) -> int:
        return L.lib().gg_clip_text_wcache_bytes(C.byref(self.cfg))

    def _refresh(self, only):
        L.check(L.lib().gg_clip_text_refresh_weights(C.byref(self.cfg), L.ptr(self._flat), L.ptr(self._wcache), L.stream()), "gg_clip_text_refresh_weights")

    def _text_workspace(self, B: int, T: int) -> Tensor:      # one inference workspace, sized by batch and token count
        need = L.lib().gg_clip_text_workspace_bytes(C.byref(self.cfg), B, T)
        if need < 0:
            raise L.GgError(L.lib().gg_last_error().decode())
        ws = self._ws.get(False)
        if ws is None or ws.numel() < need or ws.device != self._flat.device:
            ws = self._ws[False] = None
            ws = self._ws[False] = torch.empty(need, dtype=torch.uint8, device=self._flat.device)
        return ws

    def _train_workspace(self, B: int, T: int, mask: bytes) -> Tensor:      # its own buffer: an inference forward in between leaves the kept activations alone
        need = L.lib().gg_clip_text_train_workspace_bytes(C.byref(self.cfg), B, T, mask)
        if need < 0:
            raise L.GgError(L.lib().gg_last_error().decode())
        ws = self._ws.get(True)
        if ws is None or ws.numel() < need or ws.device != self._flat.device:
            ws = self._ws[True] = None
            ws = self._ws[True] = torch.empty(need, dtype=torch.uint8, device=self._flat.device)
        return ws

    def forward_hip(self, input_ids: Tensor, eos_pos: Optional[Tensor] = None, return_last_hidden: bool = False, training: bool = False):
        L.require_gpu()
        if not self._flat.is_cuda:
            raise L.GgError("CLIP text tower parameters are on the CPU; call .to('cuda') -- there is no CPU fallback")
        if not torch.is_tensor(input_ids) or not input_ids.is_cuda:
            raise L.GgError("input_ids must live on the GPU; there is no CPU fallback")
        if input_ids.dim() != 2 or input_ids.is_floating_point():
            raise L.GgError(f"input_ids must be an integer (batch, tokens) tensor, got {tuple(input_ids.shape)} {input_ids.dtype}")
        B, T = input_ids.shape
        if T > self.cfg.max_positions:
            raise L.GgError(f"{T} tokens per sequence, the position table holds {self.cfg.max_positions}")
        if eos_pos is None:
            eos_pos = eos_positions(input_ids, self.eos_token_id)
        elif not eos_pos.is_cuda:
            raise L.GgError("eos_pos must live on the GPU; there is no CPU fallback")
        eos_pos = eos_pos.to(torch.int32).contiguous()
        if eos_pos.shape != (B,):
            raise L.GgError(f"eos_pos must have shape ({B},), got {tuple(eos_pos.shape)}")
        # one host check for both index tensors (the kernels clamp, but a clamped id is a wrong answer, not an error message)
        lo, hi, elo, ehi = torch.stack([input_ids.min(), input_ids.max(), eos_pos.min().to(input_ids.dtype), eos_pos.max().to(input_ids.dtype)]).tolist()
        if lo < 0 or hi >= self.cfg.vocab_size:
            raise L.GgError(f"input_ids outside [0, {self.cfg.vocab_size}): min {lo}, max {hi}")
        if elo < 0 or ehi >= T:
            raise L.GgError(f"eos_pos outside the sequence [0, {T}): min {elo}, max {ehi}")
        ids = input_ids.to(torch.int32).contiguous()
        self._ensure_weights()
        D = self.cfg.hidden_size
        pooled = torch.empty((B, D), dtype=torch.float32, device=ids.device)
        last = torch.empty((B, T, D), dtype=torch.float32, device=ids.device) if return_last_hidden else None
        if training:
            mask = self.trainable_mask()
            ws = self._train_workspace(B, T, mask)
            L.check(L.lib().gg_clip_text_forward_train(C.byref(self.cfg), B, T, L.ptr(self._flat), L.ptr(self._wcache), L.ptr(ids), L.ptr(eos_pos), L.ptr(ws),
                                                       L.ptr(last), L.ptr(pooled), mask, L.stream()), "gg_clip_text_forward_train")
            self._record_forward(B, mask, (ids, eos_pos, T))
            return pooled, last
        ws = self._text_workspace(B, T)
        L.check(L.lib().gg_clip_text_forward(C.byref(self.cfg), B, T, L.ptr(self._flat), L.ptr(self._wcache), L.ptr(ids), L.ptr(eos_pos), L.ptr(ws),
                                             L.ptr(last), L.ptr(pooled), L.stream()), "gg_clip_text_forward")
        return pooled, last

    def backward_hip(self, d_pooled: Optional[Tensor], d_last: Optional[Tensor], gen: int):
        B, (ids, eos_pos, T), ws = self._pending(gen)
        mask = self._same_mask()
        fg = self.attach_grads()
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        d_pooled, d_last = f(d_pooled), f(d_last)
        L.check(L.lib().gg_clip_text_backward(C.byref(self.cfg), B, T, L.ptr(self._flat), L.ptr(self._wcache), L.ptr(ids), L.ptr(eos_pos), L.ptr(ws),
                                              L.ptr(d_pooled), L.ptr(d_last), L.ptr(fg), mask, L.stream()), "gg_clip_text_backward")

    def forward(self, input_ids: Tensor = None, attention_mask=None, **_):
        if self.wants_training():
            pooled, last = _TextFn.apply(self, input_ids, self._anchor(), True)
        else:
            pooled, last = self.forward_hip(input_ids, None, True)
        return SimpleNamespace(last_hidden_state=last, pooler_output=pooled)


class _TextFn(EncoderNode):
    """Whole-tower autograd node of the text tower (the counterpart of the vision tower's ``_ClipFn``; ``EncoderRuntime._anchor``)."""

    @staticmethod
    def forward(ctx, tm: _TextModel, input_ids: Tensor, anchor: Tensor, want_last: bool):
        pooled, last = tm.forward_hip(input_ids, None, want_last, training=True)
        tm._enter_node(ctx)
        ctx.set_materialize_grads(False)          # an unused last_hidden_state must not cost a (B,T,D) zero gradient
        return pooled, last


def _row0(x: Tensor) -> Tensor:
    B, T, D = x.shape
    out = torch.empty((B, D), dtype=torch.float32, device=x.device)
    L.check(L.lib().gg_row_gather_f32(L.ptr(x, torch.float32), None, L.ptr(out), B, T, D, L.stream()), "gg_row_gather_f32")
    return out


class _PoolerFn(torch.autograd.Function):
    """``post_layernorm(last_hidden_state[:, 0])`` of the vision tower.  d gamma / d beta are accumulated straight into the tower's flat gradient views (when
    trainable), dx returns as the gradient of last_hidden_state (zero but for row 0), which the tower's own backward consumes."""

    @staticmethod
    def forward(ctx, vm, last_hidden: Tensor):
        x0 = _row0(last_hidden.contiguous())
        y, mean, rstd = ops.layernorm_fwd(x0, vm._params["post_layernorm.weight"].data, vm._params["post_layernorm.bias"].data, eps=vm.cfg.ln_eps)
        ctx.vm, ctx.shape = vm, tuple(last_hidden.shape)
        ctx.save_for_backward(x0, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        vm = ctx.vm
        x0, mean, rstd = ctx.saved_tensors
        B, T, D = ctx.shape
        g, b = vm._params["post_layernorm.weight"], vm._params["post_layernorm.bias"]
        dy = dy.to(torch.float32).contiguous()
        dx0 = torch.empty_like(x0)
        dg = db = scratch = None
        if g.requires_grad or b.requires_grad:
            vm.attach_grads()
            dump = torch.zeros((D,), dtype=torch.float32, device=x0.device)      # a frozen half of the pair sums into a row nobody reads
            dg = g.grad if g.requires_grad else dump
            db = b.grad if b.requires_grad else dump
            scratch = torch.empty((L.lib().gg_layernorm_bwd_scratch_floats(B, D),), dtype=torch.float32, device=x0.device)
        L.check(L.lib().gg_layernorm_bwd(L.ptr(dy), L.ptr(x0), 1, L.ptr(mean), L.ptr(rstd), L.ptr(g.data), B, D, None, L.ptr(dx0), L.ptr(scratch),
                                         L.ptr(dg), L.ptr(db), 1, L.stream()), "gg_layernorm_bwd")
        d_last = torch.empty((B, T, D), dtype=torch.float32, device=x0.device)
        L.check(L.lib().gg_row_scatter_f32(L.ptr(dx0), None, L.ptr(d_last), B, T, D, L.stream()), "gg_row_scatter_f32")
        return None, d_last


def contrastive(img: Tensor, txt: Tensor, logit_scale: Tensor, want_loss: bool, d_loss_scale: float = 1.0, want_grads: bool = True):
    """``gg_clip_contrastive`` on (Bi, P) / (Bt, P) f32 projection outputs.  Returns a namespace: image_embeds, text_embeds, logits_per_text, logits_per_image and,
    with ``want_loss``, loss, d_logit_scale, d_img, d_txt (the gradients of ``d_loss_scale * loss``)."""
    L.require_gpu()
    for n, t in (("img", img), ("txt", txt), ("logit_scale", logit_scale)):
        if not t.is_cuda:
            raise L.GgError(f"{n} must live on the GPU (got device {t.device}); there is no CPU fallback")
    if img.dim() != 2 or txt.dim() != 2 or img.shape[1] != txt.shape[1] or img.stride(1) != 1 or txt.stride(1) != 1:
        raise L.GgError(f"contrastive: img (Bi, P) and txt (Bt, P) with unit column stride, got {tuple(img.shape)} / {tuple(txt.shape)}")
    Bi, P = img.shape
    Bt = txt.shape[0]
    dev = img.device
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    r = SimpleNamespace(image_embeds=new(Bi, P), text_embeds=new(Bt, P), logits_per_text=new(Bt, Bi), logits_per_image=new(Bi, Bt), loss=None,
                        d_logit_scale=None, d_img=None, d_txt=None)
    nscr = L.lib().gg_clip_contrastive_scratch_floats(Bi, Bt, P)
    if nscr < 0:
        raise L.GgError(L.lib().gg_last_error().decode())
    scratch = new(nscr)
    a = L.ContrastiveArgs()
    a.img, a.ldi, a.txt, a.ldt, a.Bi, a.Bt, a.P = ops._pr(img, torch.float32, "img"), img.stride(0), ops._pr(txt, torch.float32, "txt"), txt.stride(0), Bi, Bt, P
    a.logit_scale = L.ptr(logit_scale.detach().reshape(1), torch.float32, "logit_scale")
    a.img_n, a.txt_n, a.logits_per_text, a.logits_per_image = L.ptr(r.image_embeds), L.ptr(r.text_embeds), L.ptr(r.logits_per_text), L.ptr(r.logits_per_image)
    a.want_loss, a.d_loss_scale, a.scratch = int(want_loss), float(d_loss_scale), L.ptr(scratch)
    if want_loss:
        r.loss = new()
        a.loss = L.ptr(r.loss)
        if want_grads:
            r.d_logit_scale, r.d_img, r.d_txt = new(), new(Bi, P), new(Bt, P)
            a.d_logit_scale, a.d_img, a.d_txt = L.ptr(r.d_logit_scale), L.ptr(r.d_img), L.ptr(r.d_txt)
    L.check(L.lib().gg_clip_contrastive(C.byref(a), L.stream()), "gg_clip_contrastive")
    return r


def _transpose(w: Tensor) -> Tensor:
    R, Cc = w.shape
    out = torch.empty((Cc, R), dtype=torch.float32, device=w.device)
    L.check(L.lib().gg_transpose_f32(L.ptr(w, torch.float32), R, Cc, L.ptr(out), R, L.stream()), "gg_transpose_f32")
    return out


class _HeadFn(torch.autograd.Function):
    """Both projections, the contrastive head and (``return_loss``) its backward down to the pooled tower outputs, the two projection weights and logit_scale.
    The gradients of the loss are formed in the forward call (one pass over the B x B logits); backward scales them by the incoming gradient."""

    @staticmethod
    def forward(ctx, model, pooled_img: Tensor, pooled_txt: Tensor, w_img: Tensor, w_txt: Tensor, logit_scale: Tensor, want_loss: bool, grads: bool):
        img = ops.gemm_nt(pooled_img.contiguous(), w_img.detach())
        txt = ops.gemm_nt(pooled_txt.contiguous(), w_txt.detach())
        grads = bool(want_loss and grads)          # (decided by the caller: grad mode is off inside an autograd Function's forward)
        r = contrastive(img, txt, logit_scale, want_loss, 1.0, want_grads=grads)
        ctx.model, ctx.grads = model, grads
        ctx.set_materialize_grads(False)
        if grads:
            ctx.save_for_backward(pooled_img, pooled_txt, w_img, w_txt, r.d_img, r.d_txt, r.d_logit_scale)
        loss = r.loss if want_loss else torch.zeros((), device=img.device)
        ctx.mark_non_differentiable(r.logits_per_image, r.logits_per_text, r.text_embeds, r.image_embeds)
        return loss, r.logits_per_image, r.logits_per_text, r.text_embeds, r.image_embeds

    @staticmethod
    def backward(ctx, d_loss, *_):
        if d_loss is None or not ctx.grads:
            return (None,) * 8
        model = ctx.model
        need = ctx.needs_input_grad          # (model, pooled_img, pooled_txt, w_img, w_txt, logit_scale, want_loss, grads)
        hot = [n for n, p in model.text_model.named_parameters() if p.requires_grad]
        if hot and not model.text_model.train_text:
            raise L.GgError(f"text_model.{hot[0]} has requires_grad=True ({len(hot)} text tensors in all): the text tower is forward-only by default; freeze it, "
                            "e.g. with freeze_backbone_keep_head, or opt in to training it with CLIPModel(..., train_text=True) / set_text_training(True)")
        if hot and not need[2]:
            raise L.GgError(f"text_model.{hot[0]} has requires_grad=True, but this loss came from the text tower's inference forward (text training or "
                            "requires_grad was switched on since the forward); run the forward again")
        pooled_img, pooled_txt, w_img, w_txt, d_img, d_txt, d_ls = ctx.saved_tensors
        g = d_loss.to(torch.float32)
        d_pool = d_pool_txt = d_wi = d_wt = d_l = None
        if need[3]:
            d_wi = ops.gemm_tn(d_img, pooled_img.contiguous()) * g
        if need[4]:
            d_wt = ops.gemm_tn(d_txt, pooled_txt.contiguous()) * g
        if need[5]:
            d_l = (d_ls * g).reshape(ctx.model.logit_scale.shape)
        if need[1]:
            d_pool = ops.gemm_nt(d_img, _transpose(w_img.detach().contiguous())) * g
        if need[2]:
            d_pool_txt = ops.gemm_nt(d_txt, _transpose(w_txt.detach().contiguous())) * g
        return None, d_pool, d_pool_txt, d_wi, d_wt, d_l, None, None


class CLIPModel(nn.Module):
    supports_gradient_checkpointing = True

    def __init__(self, model_name: str = "openai/clip-vit-base-patch32", seed: int = 0, precision: Optional[str] = None, config: Optional[dict] = None,
                 train_text: bool = False):
        """``train_text``: opt in to training the text tower (see ``set_text_training``).  ``config`` (tests): ``dict(text=dict(hidden_size, intermediate_size, num_layers, num_heads[, vocab_size, max_positions, eos_token_id]),
        vision=dict(hidden_size, intermediate_size, num_layers, num_heads, image_size, patch_size), projection_dim=P)``."""
        super().__init__()
        if config is None:
            if model_name not in CLIP_TEXT_CONFIGS:
                raise ValueError(f"unknown CLIP model '{model_name}' (known: {', '.join(CLIP_TEXT_CONFIGS)}); pass config=")
            tk = dict(TEXT_DEFAULTS, **CLIP_TEXT_CONFIGS[model_name])
            vk = dict(CLIP_CONFIGS[model_name])
            P = tk.pop("projection_dim")
        else:
            tk = dict(TEXT_DEFAULTS, **config["text"])
            vk = dict(config["vision"])
            P = config["projection_dim"]
        code = _precision_code(precision)
        if code == 2:
            raise L.GgError("CLIPModel has no fp16 mode (precision: fp32, fp32_split or bf16)")
        tower = CLIPVisionTower(model_name, seed=seed, precision=precision, **vk)
        object.__setattr__(self, "vision_tower", tower)          # (not a registered child: its flat-storage owner is, under transformers' name)
        self.vision_model = tower.vision_model
        c = L.ClipTextCfg()
        c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads = tk["hidden_size"], tk["intermediate_size"], tk["num_layers"], tk["num_heads"]
        c.vocab_size, c.max_positions, c.ln_eps, c.act_dtype = tk["vocab_size"], tk["max_positions"], 1e-5, code
        self.text_model = _TextModel(c, seed + 1, tk["eos_token_id"])
        self.text_model.set_training(train_text)
        g = torch.Generator().manual_seed(seed + 2)
        self.visual_projection = nn.Linear(vk["hidden_size"], P, bias=False)
        self.text_projection = nn.Linear(tk["hidden_size"], P, bias=False)
        with torch.no_grad():
            self.visual_projection.weight.copy_(torch.randn(P, vk["hidden_size"], generator=g) * vk["hidden_size"] ** -0.5)
            self.text_projection.weight.copy_(torch.randn(P, tk["hidden_size"], generator=g) * tk["hidden_size"] ** -0.5)
        self.logit_scale = nn.Parameter(torch.tensor(LOGIT_SCALE_INIT))
        self.precision = PRECISION_NAMES[code]
        self.config = SimpleNamespace(_name_or_path=model_name, projection_dim=P, logit_scale_init_value=LOGIT_SCALE_INIT,
                                      text_config=SimpleNamespace(**tk), vision_config=SimpleNamespace(**vk))

    # ---- gradient checkpointing: the vision tower's -------------------------------------------------------------------------------------------
    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        self.vision_tower.gradient_checkpointing_enable()

    def gradient_checkpointing_disable(self):
        self.vision_tower.gradient_checkpointing_disable()

    # ---- text-tower training: opt-in ----------------------------------------------------------------------------------------------------------
    @property
    def train_text(self) -> bool:
        return self.text_model.train_text

    def set_text_training(self, enable: bool) -> bool:
        """With it on, a forward in grad mode with some ``text_model`` tensor trainable runs the text tower's training forward, and ``loss.backward()`` reaches its
        parameters; with it off (the default) such a backward is refused and the tower always runs its inference forward.  Toggling it between a forward and its
        backward makes that backward refuse.  Returns whether the setting changed."""
        return self.text_model.set_training(enable)

    # ---- weights -------------------------------------------------------------------------------------------------------------------------
    def load_hf_state_dict(self, sd: Dict[str, Tensor]):
        """transformers ``CLIPModel.state_dict()`` keys; unknown keys (``position_ids``) are ignored."""
        own = dict(self.named_parameters())
        with torch.no_grad():
            for k, v in sd.items():
                if k in own:
                    own[k].data.copy_(torch.as_tensor(v).to(own[k].device, torch.float32).reshape(own[k].shape))
        self.vision_model.mark_params_dirty()
        self.text_model.mark_params_dirty()

    # ---- features -------------------------------------------------------------------------------------------------------------------------
    def _image_pooled(self, pixel_values: Tensor, interpolate_pos_encoding: Optional[bool] = None) -> Tensor:
        if not torch.is_tensor(pixel_values) or not pixel_values.is_cuda:
            raise L.GgError("pixel_values must live on the GPU; there is no CPU fallback")
        vm = self.vision_model
        last = self.vision_tower(pixel_values=pixel_values, return_last_hidden=True, interpolate_pos_encoding=interpolate_pos_encoding).last_hidden_state
        if last.requires_grad:
            return _PoolerFn.apply(vm, last)
        return ops.layernorm_fwd(_row0(last), vm._params["post_layernorm.weight"].data, vm._params["post_layernorm.bias"].data, eps=vm.cfg.ln_eps,
                                 save_stats=False)[0]

    def _text_pooled(self, input_ids: Tensor) -> Tensor:
        tm = self.text_model
        if tm.wants_training():      # train_text on, grad mode on, some text tensor requires grad
            return _TextFn.apply(tm, input_ids, tm._anchor(), False)[0]
        return tm.forward_hip(input_ids, None, False)[0]

    def get_image_features(self, pixel_values: Tensor = None, interpolate_pos_encoding: Optional[bool] = None, **_) -> Tensor:
        """``interpolate_pos_encoding``: transformers' keyword, passed to the vision tower (``None``: the tower's default)."""
        with torch.no_grad():
            return ops.gemm_nt(self._image_pooled(pixel_values, interpolate_pos_encoding), self.visual_projection.weight.detach())

    def get_text_features(self, input_ids: Tensor = None, attention_mask=None, **_) -> Tensor:
        with torch.no_grad():
            return ops.gemm_nt(self._text_pooled(input_ids), self.text_projection.weight.detach())

    def forward(self, input_ids: Tensor = None, pixel_values: Tensor = None, attention_mask=None, return_loss: bool = False,
                interpolate_pos_encoding: Optional[bool] = None, **_):
        pooled_txt = self._text_pooled(input_ids)
        pooled_img = self._image_pooled(pixel_values, interpolate_pos_encoding)
        if return_loss and pooled_img.shape[0] != pooled_txt.shape[0]:
            raise L.GgError(f"return_loss needs as many images as texts (got {pooled_img.shape[0]} images, {pooled_txt.shape[0]} texts)")
        loss, lpi, lpt, te, ie = _HeadFn.apply(self, pooled_img, pooled_txt, self.visual_projection.weight, self.text_projection.weight, self.logit_scale,
                                               bool(return_loss), torch.is_grad_enabled())
        return SimpleNamespace(loss=loss if return_loss else None, logits_per_image=lpi, logits_per_text=lpt, text_embeds=te, image_embeds=ie)
