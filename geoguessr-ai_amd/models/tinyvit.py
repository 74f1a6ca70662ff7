"""Drop-in for the reference's ``models/tinyvit.py`` (``TinyViTAdapter``, :17-150): same constructor, same
``.config`` / ``.vision_model.encoder.layers`` shims, same ``freeze_*`` / ``train`` semantics, same forward return
(``pooler_output`` (B,C), ``last_hidden_state`` (B,1,C)), same ``backbone.*`` state-dict keys (timm names,
SURVEY.md App. A.5) -- but the encoder itself is the HIP runtime in ``csrc/tinyvit.hip`` (one C call for the
whole forward, one for the whole backward) instead of ``timm.create_model``.

Parameters are views into ONE flat fp32 device buffer (gradients likewise), which is what the RCCL gradient
all-reduce and the fused AdamW kernel operate on.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from types import SimpleNamespace
from typing import List, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .flat import EncoderNode, EncoderRuntime

# timm variants; drop_path_rate is timm's per-variant default
VARIANTS = {
    "tiny_vit_5m_224": dict(embed_dims=(64, 128, 160, 320), num_heads=(2, 4, 5, 10), window_sizes=(7, 7, 14, 7),
                            img_size=224, drop_path_rate=0.0),
    "tiny_vit_11m_224": dict(embed_dims=(64, 128, 256, 448), num_heads=(2, 4, 8, 14), window_sizes=(7, 7, 14, 7),
                             img_size=224, drop_path_rate=0.1),
    "tiny_vit_21m_224": dict(embed_dims=(96, 192, 384, 576), num_heads=(3, 6, 12, 18), window_sizes=(7, 7, 14, 7),
                             img_size=224, drop_path_rate=0.2),
    "tiny_vit_21m_384": dict(embed_dims=(96, 192, 384, 576), num_heads=(3, 6, 12, 18), window_sizes=(12, 12, 24, 12),
                             img_size=384, drop_path_rate=0.1),
    "tiny_vit_21m_512": dict(embed_dims=(96, 192, 384, 576), num_heads=(3, 6, 12, 18), window_sizes=(16, 16, 32, 16),
                             img_size=512, drop_path_rate=0.1),
}
DEPTHS = (2, 2, 6, 2)


PRECISIONS = {"bf16": 0, "bfloat16": 0, "fp32": 1, "f32": 1, "float32": 1, "fp32_split": 3}      # fp32_split: f32 storage, the transformer blocks' Linears as f32-accurate split-bf16 products


def default_precision() -> str:
    """``GG_PRECISION`` = "fp32" (default: the reference's own arithmetic -- f32 activations, f32 MFMA, fp32-accurate GELU)
    or "bf16" (bf16 activations / MFMA operands, fp32 accumulation and master weights: 3.4x the throughput, bf16-level parity)."""
    p = os.environ.get("GG_PRECISION", "fp32").lower()
    if p not in PRECISIONS:
        raise ValueError(f"GG_PRECISION='{p}' (known: bf16, fp32, fp32_split)")
    return p


def check_attention16(attention16: bool, precision: Optional[str], who: str) -> None:
    """``attention16=True`` is a switch of the bf16 mode: refused by name for ``fp32`` and ``fp32_split`` (their attention is f32-accurate by contract; the wording
    and the reason of ``pretrain.clip_embedder.check_attention16``)."""
    prec = precision or default_precision()
    if attention16 and PRECISIONS.get(prec, 0) in (1, 3):
        raise L.GgError(f"{who}: attention16=True is a switch of the bf16 mode; precision='{'fp32_split' if PRECISIONS[prec] == 3 else 'fp32'}' keeps its f32-accurate "
                        "attention (leave attention16 off)")


def check_attention16_train(attention16_train: bool, precision: Optional[str], who: str) -> None:
    """``attention16_train=True`` is a switch of the bf16 training step: refused by name for ``fp32`` and ``fp32_split`` (their attention is f32-accurate by
    contract; ``check_attention16``'s wording)."""
    prec = precision or default_precision()
    if attention16_train and PRECISIONS.get(prec, 0) in (1, 3):
        raise L.GgError(f"{who}: attention16_train=True is a switch of the bf16 mode; precision='{'fp32_split' if PRECISIONS[prec] == 3 else 'fp32'}' keeps its "
                        "f32-accurate attention (leave attention16_train off)")


def make_cfg(model_name: str, **overrides) -> tuple:
    base = model_name.split(".")[0]
    if base not in VARIANTS:
        raise ValueError(f"unknown TinyViT variant '{model_name}' (known: {sorted(VARIANTS)})")
    v = dict(VARIANTS[base])
    v.update(overrides)
    depths = tuple(v.get("depths", DEPTHS))
    c = L.TinyVitCfg()
    c.img_size, c.in_chans = v["img_size"], 3
    c.embed_dims = (C.c_int * 4)(*v["embed_dims"])
    c.depths = (C.c_int * 4)(*depths)
    c.num_heads = (C.c_int * 4)(*v["num_heads"])
    c.window_sizes = (C.c_int * 4)(*v["window_sizes"])
    c.mlp_ratio, c.mbconv_expand_ratio = 4.0, 4.0
    c.bn_eps, c.ln_eps, c.bn_momentum = 1e-5, 1e-5, 0.1
    prec = v.get("precision") or default_precision()
    if prec not in PRECISIONS:
        raise ValueError(f"precision='{prec}' (known: {', '.join(PRECISIONS)})")
    c.act_dtype = PRECISIONS[prec]
    c.features_only = int(bool(v.get("features_only", False)))
    c.recompute = int(bool(v.get("grad_checkpointing", False)))      # activation recompute (TinyVitBackbone.set_grad_checkpointing)
    return c, v, depths


def _tensor_table(cfg: L.TinyVitCfg):
    lib = L.lib()
    n = lib.gg_tinyvit_num_tensors(C.byref(cfg))
    if n < 0:
        raise L.GgError(lib.gg_last_error().decode())
    out = []
    name = C.create_string_buffer(256)
    off, numel, ndim, kind = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
    shape = (C.c_int64 * 4)()
    for i in range(n):
        L.check(lib.gg_tinyvit_tensor_info(C.byref(cfg), i, name, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape,
                                           C.byref(kind)), "gg_tinyvit_tensor_info")
        out.append(dict(name=name.value.decode(), offset=off.value, numel=numel.value,
                        shape=tuple(shape[j] for j in range(ndim.value)), kind=kind.value, index=i))
    return out


def _init_tensor(name: str, shape, g: torch.Generator) -> torch.Tensor:
    """timm TinyVit init: Linear trunc_normal(.02)/0, LayerNorm 1/0, Conv2d torch default, BN 1/0 except the last
    BN of an MBConv (0), attention biases 0."""
    if name.endswith("conv.weight"):
        fan_in = shape[1] * shape[2] * shape[3]
        return (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
    if name.endswith("bn.weight"):
        return torch.zeros(shape) if (name.startswith("stages.0.") and ".conv3." in name) else torch.ones(shape)
    if name.endswith("norm.weight"):
        return torch.ones(shape)
    if name.endswith("attention_biases") or name.endswith(".bias"):
        return torch.zeros(shape)
    if name.endswith(".weight"):
        t = torch.empty(shape)
        nn.init.trunc_normal_(t, std=0.02, generator=g)
        return t
    raise AssertionError(name)


class TinyVitBackbone(EncoderRuntime):
    """Owner of the flat parameter / buffer storage and of the HIP workspace (``self.backbone`` of the adapter)."""
    _name, _switch, _gen_why = "TinyViT", "set_grad_checkpointing", "saved activations live in ONE workspace per backbone, so "

    def __init__(self, model_name: str, seed: Optional[int] = None, attention16: bool = False, attention16_train: bool = False,
                 deterministic_bias_grad: bool = False, **overrides):
        """``attention16=True`` (bf16 only; opt-in): this backbone's inference forwards run with ``gg_tinyvit_set_attention16(1)`` -- windows beyond 256 tokens
        (tiny_vit_21m_384 / _512 stage 2) through ``gg_attention_flash16_win_fwd`` (include/gg_attn16w.h); training forwards are unaffected.
        ``attention16_train=True`` (bf16 only; opt-in, independent of ``attention16``): this backbone's training forwards and backwards run with
        ``gg_tinyvit_set_attention16_train(1)`` -- the same windows' training forward, recompute replay and attention backward through
        ``gg_attention_flash16_win_fwd`` / ``gg_attention_flash16_win_bwd`` (include/gg_attn16wb.h); inference forwards are unaffected.
        ``deterministic_bias_grad=True`` (every precision; opt-in, composes with the other switches, recompute, padded sizes and trainable masks): this
        backbone's backwards run with ``gg_tinyvit_set_deterministic_dbias(1)`` -- the gradient of every trainable ``attention_biases`` comes from
        ``gg_attention_dbias`` (include/gg_attn_dbias.h), which adds in a fixed order: every gradient of a step is then bit-reproducible."""
        super().__init__()
        check_attention16(attention16, overrides.get("precision"), type(self).__name__)
        check_attention16_train(attention16_train, overrides.get("precision"), type(self).__name__)
        self.attention16 = bool(attention16)
        self.attention16_train = bool(attention16_train)
        self.deterministic_bias_grad = bool(deterministic_bias_grad)
        self.cfg, self.variant, self.depths = make_cfg(model_name, **overrides)
        self.model_name = model_name.split(".")[0]
        self.precision = "fp32" if self.cfg.act_dtype in (1, 3) else "bf16"          # storage / arithmetic class ("fp32_split" stores and checks like fp32)
        self.split = self.cfg.act_dtype == 3
        self.table = _tensor_table(self.cfg)
        lib = L.lib()
        self.num_features = int(self.variant["embed_dims"][-1])
        self.param_floats = lib.gg_tinyvit_param_floats(C.byref(self.cfg))
        self.buffer_floats = lib.gg_tinyvit_buffer_floats(C.byref(self.cfg))
        self.num_counters = lib.gg_tinyvit_num_counters(C.byref(self.cfg))
        self.num_drop_slots = lib.gg_tinyvit_num_drop_slots(C.byref(self.cfg))
        n_blocks = sum(self.depths)
        rates = torch.linspace(0, float(self.variant["drop_path_rate"]), n_blocks).tolist()
        slot_rates: List[float] = []
        for b in range(n_blocks):
            slot_rates += [rates[b]] if b < self.depths[0] else [rates[b], rates[b]]
        self.drop_rates = slot_rates
        g = torch.Generator().manual_seed(torch.initial_seed() if seed is None else seed)
        self._register_table(lambda name, shape: _init_tensor(name, shape, g))

    grad_checkpointing = property(lambda self: bool(self.cfg.recompute))          # (timm's attribute)
    img_size = property(lambda self: int(self.cfg.img_size))                      # the input side the model was built for (``img_size=`` override or the variant's own)

    @property
    def padded_maps(self) -> tuple:
        """``(stage, res, padded_res)`` of every stage whose token map the attention window does not divide (``img_size=`` other than the variant's own): its
        TinyVitBlocks zero-pad the map at the bottom and right to ``padded_res`` in front of the attention module and crop the result back (timm
        ``TinyVitBlock.forward``; csrc/window_pad.hip).  Empty for sizes that divide -- those take the schedule without a pad or crop launch."""
        out = []
        for s in (1, 2, 3):
            res, ws = self.cfg.img_size // (4 * 2 ** s), self.cfg.window_sizes[s]
            if res % ws:
                out.append((s, res, -(-res // ws) * ws))
        return tuple(out)

    def set_grad_checkpointing(self, enable: bool = True):
        """timm's switch (``model.set_grad_checkpointing()``; the reference's ``adapter.backbone`` is the timm model): activation recompute of the
        training step (``GgTinyVitCfg.recompute``, include/gg.h).  The workspace keeps each segment's input (an MBConv, a PatchMerging, a
        TinyVitBlock), the ConvNorms' batch statistics and PatchEmbed; the backward re-forms a segment's other tensors right before its backward.
        Output, gradients, running statistics and ``num_batches_tracked`` are bit-identical to the step without recompute (the attention-bias
        gradients only to rounding: the attention backward sums them with float atomics, so they vary in their last bits between any two steps).  Unlike
        ``torch.utils.checkpoint``, whose recompute runs BatchNorm in train mode again and so updates the running statistics twice, the recompute
        reuses the forward's batch statistics: the running buffers are updated once per step.  Inference ignores the setting."""
        self.set_recompute(enable)
        return self

    # -- HIP calls ------------------------------------------------------------------------------------------
    def _wcache_bytes(self) -> int:
        return L.lib().gg_tinyvit_wcache_bytes(C.byref(self.cfg))

    def _refresh(self, only):
        a = (C.byref(self.cfg), L.ptr(self._flat, torch.float32, "params"), L.ptr(self._wcache))
        if only is None:
            L.check(L.lib().gg_tinyvit_refresh_weights(*a, L.stream()), "gg_tinyvit_refresh_weights")
        else:
            L.check(L.lib().gg_tinyvit_refresh_weights_masked(*a, only, L.stream()), "gg_tinyvit_refresh_weights_masked")

    def _workspace_bytes(self, batch: int, training: bool, mask) -> int:
        return L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(self.cfg), batch, int(training), mask)

    def make_drop_scales(self, batch: int, generator: Optional[torch.Generator] = None) -> Optional[torch.Tensor]:
        """timm DropPath (scale_by_keep): per-sample Bernoulli(1-p)/(1-p), one row per slot, drawn by ``gg_drop_path_scales`` (a counter-based
        generator on the device).  The seed comes from torch's RNG once per backbone (so ``torch.manual_seed`` makes runs repeatable), the counter
        advances with every call.  With ``generator`` the rows are a function of that generator's seed and of how many times that generator object has
        been passed here (its own state is neither read on the device nor advanced); these per-generator counts are not part of ``drop_path_state()``."""
        if max(self.drop_rates) <= 0:
            return None
        dev = self._flat.device
        rates = getattr(self, "_rates_dev", None)
        if rates is None or rates.device != dev:          # cached on the device: no host-to-device copy per step (graph-capturable)
            rates = self._rates_dev = torch.tensor(self.drop_rates, dtype=torch.float32, device=dev)
        if generator is not None:
            # host-side (seed, counter) from the generator's seed + a per-generator call count: no device round trip (a CUDA generator's randint +
            # .item() was a blocking sync per step), deterministic for a given generator seed and call order.  The count lives with the generator OBJECT
            # (torch generators can be neither weakly referenced nor given attributes: the entry holds a strong reference, so the object's id cannot be
            # reused by another generator while the entry lives; the table keeps the 16 most recently used generators) and restarts when the generator is
            # given another seed; re-seeding it with the SAME seed continues the count (initial_seed() cannot tell) -- use a fresh generator for that
            counts = self.__dict__.setdefault("_drop_gen_counts", {})
            seed = int(generator.initial_seed()) & (2 ** 62 - 1)
            ent = counts.pop(id(generator), None)
            if ent is None or ent[0] is not generator or ent[1] != seed:
                ent = [generator, seed, 0]
            counter = ent[2]
            ent[2] += 1
            counts[id(generator)] = ent                 # (re-inserted last: dicts keep insertion order, the oldest entry leaves first)
            while len(counts) > 16:
                counts.pop(next(iter(counts)))
        else:
            if getattr(self, "_drop_seed", None) is None:
                self._drop_seed, self._drop_counter = int(torch.randint(0, 2 ** 62, (1,)).item()), 0      # (CPU RNG, once per backbone)
            seed, counter = self._drop_seed, self._drop_counter
            self._drop_counter += 1
        out = torch.empty((self.num_drop_slots, batch), dtype=torch.float32, device=dev)
        L.check(L.lib().gg_drop_path_scales(L.ptr(rates), self.num_drop_slots, batch, seed, counter, L.ptr(out), L.stream()), "gg_drop_path_scales")
        return out

    # DropPath stream position: kept OUT of state_dict (its keys are the timm contract) and saved by checkpoint.save_checkpoint under its own key, so
    # a resumed run continues the mask sequence instead of replaying it from counter 0
    def drop_path_state(self):
        return dict(drop_seed=getattr(self, "_drop_seed", None), drop_counter=getattr(self, "_drop_counter", 0))

    def load_drop_path_state(self, state):
        if state and state.get("drop_seed") is not None:
            self._drop_seed, self._drop_counter = int(state["drop_seed"]), int(state.get("drop_counter", 0))

    def forward_hip(self, x: torch.Tensor, training: bool, drop_scales: Optional[torch.Tensor] = None, features_only: Optional[bool] = None) -> torch.Tensor:
        """``features_only`` (None: the backbone's own setting): this ONE call returns the pooled last feature map without head.norm (True) or with it
        (False) from the same parameters, weight cache and workspace -- the plan does not depend on the flag (TinyViTClassifier.pooled_features)."""
        L.require_gpu()
        cfg = self.cfg
        if features_only is not None and int(bool(features_only)) != cfg.features_only:
            cfg = L.TinyVitCfg.from_buffer_copy(self.cfg)
            cfg.features_only = int(bool(features_only))
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != self.cfg.img_size or x.shape[3] != self.cfg.img_size:
            raise L.GgError(f"TinyViT expects (B,3,{self.cfg.img_size},{self.cfg.img_size}) pixel_values, got {tuple(x.shape)}")
        if not self._flat.is_cuda:
            raise L.GgError("TinyViTAdapter parameters are on the CPU; call .to('cuda') -- there is no CPU fallback")
        x = x.to(device=self._flat.device, dtype=torch.float32).contiguous()
        B = x.shape[0]
        mask, ws = self._prepare(B, training)
        out = torch.empty((B, self.num_features), dtype=torch.float32, device=x.device)
        if drop_scales is not None:
            assert drop_scales.shape == (self.num_drop_slots, B) and drop_scales.dtype == torch.float32
        lib = L.lib()
        prev = lib.gg_tinyvit_set_attention16(1) if self.attention16 else None      # process-wide switch, read when the forward is enqueued: set for this call only
        prev_t = lib.gg_tinyvit_set_attention16_train(1) if self.attention16_train and training else None      # the same, the training step's switch
        try:
            L.check(lib.gg_tinyvit_forward(C.byref(cfg), B, int(training), L.ptr(self._flat), L.ptr(self._flat_buf),
                                           L.ptr(self._counters), L.ptr(self._wcache), L.ptr(x), L.ptr(drop_scales), L.ptr(ws),
                                           L.ptr(out), mask, L.stream()),
                    "gg_tinyvit_forward")
        finally:
            if prev is not None:
                lib.gg_tinyvit_set_attention16(prev)
            if prev_t is not None:
                lib.gg_tinyvit_set_attention16_train(prev_t)
        if training:
            self._counters += 1          # num_batches_tracked (int64 bookkeeping)
            self._record_forward(B, mask, drop_scales)
        return out

    def _stage_ranges(self):
        """Flat float range of each backward stage id: 3, 2, 1 (TinyVitStages), 0 (MBConv stage), -1 (patch_embed); the range of
        stage 3 also holds head.norm (final before the stage loop starts)."""
        if getattr(self, "_stage_rng", None) is None:
            first = {}
            for t in self.table:
                if t["kind"] != 0:
                    continue
                key = -1 if t["name"].startswith("patch_embed.") else (int(t["name"].split(".")[1]) if t["name"].startswith("stages.") else 4)
                first.setdefault(key, t["offset"])
            order = [-1, 0, 1, 2, 3]
            ends = {k: (first[order[i + 1]] if i + 1 < len(order) else self.param_floats) for i, k in enumerate(order)}
            self._stage_rng = {k: (first[k], ends[k]) for k in order}
        return self._stage_rng

    def backward_hip(self, d_out: torch.Tensor, gen: Optional[int] = None):
        B, drop, ws = self._pending(gen, d_out.shape[0])
        fg = self.attach_grads()
        mask = self._same_mask()
        hook = self._grad_ready_hook
        cb = L.STAGE_DONE_FN(0)
        failed = []
        if hook is not None:
            rng = self._stage_ranges()

            def _stage_done(stage, _user):
                # ctypes swallows an exception raised inside a callback (it only prints "Exception ignored ..."), and a rank that skips one
                # bucket would then launch its collectives in another order than its peers: keep the first failure, send nothing further
                # from inside this backward (allreduce_grads() sends whatever is left in one fixed order) and re-raise below
                if failed:
                    return
                try:
                    hook(*rng[stage])
                except BaseException as exc:      # noqa: BLE001 -- must not escape into the C caller
                    failed.append(exc)
            cb = L.STAGE_DONE_FN(_stage_done)
        lib = L.lib()
        prev_t = lib.gg_tinyvit_set_attention16_train(1) if self.attention16_train else None      # read when the backward is enqueued (its recompute replay included)
        prev_d = lib.gg_tinyvit_set_deterministic_dbias(1) if self.deterministic_bias_grad else None      # the same: the fixed-order bias gradient
        try:
            L.check(lib.gg_tinyvit_backward(C.byref(self.cfg), B, L.ptr(self._flat), L.ptr(self._wcache), L.ptr(drop), L.ptr(ws),
                                            L.ptr(d_out.contiguous(), torch.float32, "d_out"), L.ptr(fg), mask, L.stream(), cb, None),
                    "gg_tinyvit_backward")
        finally:
            if prev_t is not None:
                lib.gg_tinyvit_set_attention16_train(prev_t)
            if prev_d is not None:
                lib.gg_tinyvit_set_deterministic_dbias(prev_d)
        if failed:
            raise L.GgError(f"TinyViT backward: the gradient-ready hook failed ({type(failed[0]).__name__}: {failed[0]}); the gradients are "
                            "complete, but no further bucket was sent from inside this backward pass") from failed[0]

    def activation(self, name: str, batch: int) -> torch.Tensor:
        """Raw bytes of a saved activation of the last training forward (parity tests)."""
        off, nbytes = C.c_int64(), C.c_int64()
        L.check(L.lib().gg_tinyvit_activation_info_masked(C.byref(self.cfg), batch, name.encode(), self._train_mask, C.byref(off),
                                                          C.byref(nbytes)), "gg_tinyvit_activation_info")
        return self._ws[True][off.value:off.value + nbytes.value]

    def forward(self, x):
        return _EncoderFn.apply(self, x, self._anchor() if self.wants_grad() else self._anchor().detach())


class _EncoderFn(EncoderNode):
    """Whole-encoder autograd node (``EncoderRuntime._anchor``)."""

    @staticmethod
    def forward(ctx, bb: TinyVitBackbone, x: torch.Tensor, anchor: torch.Tensor):
        need_grad = ctx.needs_input_grad[2]      # (grad mode is off inside Function.forward)
        training = bb.training
        drop = bb.make_drop_scales(x.shape[0]) if training else None
        out = bb.forward_hip(x, training, drop)
        bb._enter_node(ctx, training and need_grad)
        return out


class TinyViTAdapter(nn.Module):
    """See module docstring.  ``pretrained=True`` cannot download (no network): weights are looked up in
    ``$GG_PRETRAINED_DIR/<model_name>.pt`` (a timm state dict) and otherwise a warning is issued and the timm
    initialisation is used."""

    def __init__(self, model_name: str = "tiny_vit_21m_512.dist_in22k_ft_in1k", pretrained: bool = True,
                 global_pool: str = "avg", features_only: bool = False, **overrides):
        """``overrides`` (not in the reference): ``precision="bf16"|"fp32"`` (default ``$GG_PRECISION`` or fp32), ``seed``,
        ``drop_path_rate``, ``img_size`` (any multiple of 32: where the attention window does not divide a stage's map the blocks pad it --
        ``backbone.padded_maps``) ... (timm ``create_model`` kwargs), ``grad_checkpointing=True`` (activation recompute from the start;
        the same as ``adapter.backbone.set_grad_checkpointing()``), ``attention16=True`` (bf16 only, opt-in: the inference forward's windows beyond
        256 tokens on the 16-bit MFMA -- ``TinyVitBackbone``; ``precision="fp32"`` / ``"fp32_split"`` with it raises), ``attention16_train=True`` (bf16 only, opt-in,
        independent of ``attention16``: the training step's windows beyond 256 tokens -- forward, recompute replay and backward -- on the 16-bit MFMA; the same
        refusals), ``deterministic_bias_grad=True`` (every precision, opt-in: the ``attention_biases`` gradients from the fixed-order kernel of
        include/gg_attn_dbias.h, so that every gradient of a step is bit-reproducible -- ``TinyVitBackbone``)."""
        super().__init__()
        check_attention16(overrides.get("attention16", False), overrides.get("precision"), "TinyViTAdapter")
        check_attention16_train(overrides.get("attention16_train", False), overrides.get("precision"), "TinyViTAdapter")
        if global_pool != "avg":
            raise NotImplementedError("only global_pool='avg' (the reference's setting) is built")
        # features_only=True (models/tinyvit.py:38-46): timm returns the stage feature maps and the adapter's forward pools the last
        # one (:139-143) -- i.e. the encoder output WITHOUT head.norm; the runtime writes exactly that vector
        self.features_only = features_only
        self.backbone = TinyVitBackbone(model_name, features_only=features_only, **overrides)
        hidden = self.backbone.num_features
        self.config = SimpleNamespace(hidden_size=hidden, hidden_sizes=[hidden], _name_or_path=model_name)
        stages = self.backbone._modules["stages"]
        self.vision_model = SimpleNamespace(encoder=SimpleNamespace(layers=list(stages)))
        self._fully_frozen = False
        if pretrained:
            d = os.environ.get("GG_PRETRAINED_DIR")
            path = os.path.join(d, model_name + ".pt") if d else None
            if path and os.path.exists(path):
                self.backbone.load_state_dict(torch.load(path, map_location="cpu"), strict=False)
            else:
                warnings.warn(f"pretrained weights for {model_name} not available offline (set GG_PRETRAINED_DIR); "
                              "using the timm initialisation")

    def build_transform(self):
        raise RuntimeError("timm data transforms not available in this environment.")   # models/tinyvit.py:83-86

    def freeze_all(self, eval_mode: bool = True):
        for p in self.parameters():
            p.requires_grad = False
        self._fully_frozen = True
        if eval_mode:
            super().train(False)
        return self

    def unfreeze_all(self):
        for p in self.parameters():
            p.requires_grad = True
        self._fully_frozen = False
        return self

    def freeze_all_but_last_stage(self):
        layers = list(self.vision_model.encoder.layers)
        for m in layers[:-1]:
            for p in m.parameters():
                p.requires_grad = False
        return self

    def train(self, mode: bool = True):
        if self._fully_frozen:
            return super().train(False)
        return super().train(mode)

    def forward(self, pixel_values: torch.Tensor = None, x: Optional[torch.Tensor] = None):
        if pixel_values is None and x is not None:
            pixel_values = x
        out = self.backbone(pixel_values)
        return SimpleNamespace(pooler_output=out, last_hidden_state=out.unsqueeze(1))
