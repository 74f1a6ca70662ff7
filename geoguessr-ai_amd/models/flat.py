"""Flat parameter storage shared by the encoder runtimes (TinyViT, CLIP): every parameter of the module tree is a view into ONE flat fp32
device buffer described by the runtime's tensor table (``gg_*_tensor_info``), gradients are views into one flat gradient buffer.  That
layout is what the RCCL gradient all-reduce and the fused AdamW kernel (``optim.AdamW``) operate on; the module nesting is rebuilt from the
dotted tensor names so that state-dict keys come out with the upstream library's names (timm / transformers)."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch
import torch.nn as nn

from .._lib import GgError, lib


class _Tree(nn.Module):
    """Anonymous container mirroring timm's module nesting so that state-dict keys come out with timm names."""

    def __iter__(self):
        return iter(self.children())

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, i):
        return list(self.children())[i]


class FlatStore(_Tree):
    """Needs from the subclass, before ``_register_table``: ``self.table`` (list of dicts name / offset / numel / shape / kind with kind
    0 = parameter, 1 = float buffer, 2 = int64 counter), ``self.param_floats``, ``self.buffer_floats``, ``self.num_counters``."""

    def _register_table(self, init: Callable[[str, tuple], torch.Tensor]):
        self._flat = torch.zeros(self.param_floats)
        self._flat_buf = torch.zeros(self.buffer_floats)
        self._counters = torch.zeros(self.num_counters, dtype=torch.int64)
        self._flat_grad: Optional[torch.Tensor] = None
        self._params: Dict[str, nn.Parameter] = {}
        for t in self.table:
            parent, leaf = self._walk(t["name"])
            if t["kind"] == 0:
                view = self._flat[t["offset"]:t["offset"] + t["numel"]].view(t["shape"])
                view.copy_(init(t["name"], t["shape"]))
                p = nn.Parameter(view)
                parent.register_parameter(leaf, p)
                self._params[t["name"]] = p
            elif t["kind"] == 1:
                view = self._flat_buf[t["offset"]:t["offset"] + t["numel"]].view(t["shape"])
                view.fill_(1.0 if leaf == "running_var" else 0.0)
                parent.register_buffer(leaf, view)
            else:
                parent.register_buffer(leaf, self._counters[t["offset"]])

    # -- module tree helpers ---------------------------------------------------------------------------
    def _walk(self, name: str):
        parts = name.split(".")
        mod = self
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Tree())
            mod = mod._modules[p]
        return mod, parts[-1]

    def _apply(self, fn, *a, **k):
        """``.to(device)`` moves every parameter separately; re-point them into fresh flat buffers afterwards."""
        super()._apply(fn, *a, **k)
        self._reflatten()
        return self

    def _reflatten(self):
        some = next(iter(self._params.values()))
        dev = some.device
        flat = torch.zeros(self.param_floats, device=dev)
        buf = torch.zeros(self.buffer_floats, device=dev)
        cnt = torch.zeros(self.num_counters, dtype=torch.int64, device=dev)
        grad = None
        if any(p.grad is not None for p in self._params.values()):
            grad = torch.zeros(self.param_floats, device=dev)
        for t in self.table:
            parent, leaf = self._walk(t["name"])
            sl = slice(t["offset"], t["offset"] + t["numel"])
            if t["kind"] == 0:
                p = parent._parameters[leaf]
                flat[sl].view(t["shape"]).copy_(p.data.to(torch.float32))
                p.data = flat[sl].view(t["shape"])
                if p.grad is not None:
                    grad[sl].view(t["shape"]).copy_(p.grad)
                    p.grad = grad[sl].view(t["shape"])
            elif t["kind"] == 1:
                buf[sl].view(t["shape"]).copy_(parent._buffers[leaf].to(torch.float32))
                parent._buffers[leaf] = buf[sl].view(t["shape"])
            else:
                cnt[t["offset"]] = parent._buffers[leaf].to(torch.int64)
                parent._buffers[leaf] = cnt[t["offset"]]
        self._flat, self._flat_buf, self._counters, self._flat_grad = flat, buf, cnt, grad

    # -- flat views used by the optimizer / all-reduce ---------------------------------------------------
    @property
    def flat_params(self) -> torch.Tensor:
        return self._flat

    def flat_grads(self) -> torch.Tensor:
        if self._flat_grad is None or self._flat_grad.device != self._flat.device:
            self._flat_grad = torch.zeros_like(self._flat)
        return self._flat_grad

    def attach_grads(self, zero_missing: bool = True):
        """Make every trainable parameter's ``.grad`` a view of the flat gradient buffer.  If a ``zero_grad(set_to_none)``
        dropped the views the buffer is zeroed first (its contents belonged to the previous step)."""
        fg = self.flat_grads()
        dropped = any(p.requires_grad and p.grad is None for p in self._params.values())
        if dropped and zero_missing:
            fg.zero_()
        for t in self.table:
            if t["kind"] != 0:
                continue
            p = self._params[t["name"]]
            if p.requires_grad:
                if p.grad is None or p.grad.data_ptr() != fg.data_ptr() + 4 * t["offset"]:
                    p.grad = fg[t["offset"]:t["offset"] + t["numel"]].view(t["shape"])
        return fg

    def trainable_mask(self) -> bytes:
        return bytes(int(t["kind"] == 0 and self._params[t["name"]].requires_grad) for t in self.table)

    def trainable_ranges(self):
        """Contiguous [start, end) float ranges of the flat buffer covering runs of trainable tensors."""
        ranges, cur = [], None
        for t in self.table:
            if t["kind"] != 0:
                continue
            tr = self._params[t["name"]].requires_grad
            end = t["offset"] + (t["numel"] + 7) // 8 * 8
            if tr:
                cur = [t["offset"], end] if cur is None else [cur[0], end]
            elif cur is not None:
                ranges.append(tuple(cur)); cur = None
        if cur is not None:
            ranges.append(tuple(cur))
        return ranges

    def _param_version(self):
        """Changes whenever any parameter is written through torch (``torch.optim`` steps, ``load_state_dict``, ``p.copy_``):
        after ``_reflatten`` every Parameter is its own view with its own version counter, so the flat buffer's counter alone
        misses those writes.  Raw-pointer writers (the fused AdamW kernel) call ``EncoderRuntime.mark_params_dirty`` instead."""
        return (self._flat._version, sum(p._version for p in self._params.values()), self._flat.data_ptr())


class EncoderRuntime(FlatStore):
    """The step lifecycle of an encoder whose forward and backward are one C call each (``TinyVitBackbone``, CLIP's ``_VisionModel``): the weight
    cache and its refresh, one workspace per ``training`` flag, the record of the training forward whose activations the workspace holds, the
    backward's refusals, the recompute toggle and the autograd anchor.  Needs from the subclass: ``self.cfg`` (with ``.recompute``), ``forward_hip``
    / ``backward_hip(*grads, gen)`` around the C calls, and three hooks: ``_wcache_bytes()``, ``_workspace_bytes(batch, training, mask)`` and
    ``_refresh(only)``, which rebuilds the weight cache (``only`` = a tensor mask that covers every change, or None; a model may ignore it)."""
    _name, _switch, _gen_why = "encoder", "recompute", ""      # in the refusals: display name, the model's name for its recompute toggle, TinyViT's extra clause
    _mask_changed = ("requires_grad changed between forward and backward for {changed} ...: the training forward laid out its workspace for the mask "
                     "it saw (activations only a frozen weight's gradient needs are not kept); run the forward again")

    def __init__(self):
        super().__init__()
        self._wcache = self._anchor_t = None
        self._wcache_version = self._synced_ver = -1      # _param_version() of the last refresh; mark_params_dirty resets only the first
        self._dirty_all, self._dirty_only = True, None
        self._ws: Dict[bool, torch.Tensor] = {}
        self._gen, self._last = 0, None     # generation of the training workspace contents (one per training forward); (batch, payload, generation) of that forward
        self._train_mask = self._last_recompute = None      # the trainable mask and cfg.recompute its workspace was laid out for
        self._grad_ready_hook = None        # set by optim.AdamW.overlap_allreduce: fn(lo, hi) over flat gradient floats

    def _reflatten(self):
        super()._reflatten()
        self._wcache, self._wcache_version, self._ws = None, -1, {}      # (they lived on the old device)

    def mark_params_dirty(self, only: Optional[bytes] = None):
        """A raw-pointer writer (the fused AdamW kernel, a broadcast, a checkpoint load) changed parameters behind torch's version counters: the
        weight cache must be rebuilt.  ``only`` = the trainable mask the writer went by (one byte per tensor): then only those tensors' cached
        forms are rebuilt (masks of several writes are OR-ed); ``None`` = anything may have changed."""
        self._wcache_version = -1
        if only is None:
            self._dirty_all, self._dirty_only = True, None
        elif not self._dirty_all:
            self._dirty_only = bytes(only) if self._dirty_only is None else bytes(a | b for a, b in zip(self._dirty_only, only))

    def _ensure_weights(self):
        if self._wcache is None:
            self._wcache = torch.zeros(self._wcache_bytes(), dtype=torch.uint8, device=self._flat.device)
            self._wcache_version, self._dirty_all = -1, True
        ver = self._param_version()
        if self._wcache_version != ver:
            # full rebuild unless the only writers since the last sync were masked raw-pointer writers (the fused optimizer) AND torch's own
            # version counters did not move (no load_state_dict / copy_ / torch.optim step in between)
            self._refresh(None if (self._dirty_all or self._synced_ver != ver) else self._dirty_only)
            self._wcache_version = self._synced_ver = ver
            self._dirty_all, self._dirty_only = False, None

    def _workspace(self, batch: int, training: bool, mask: Optional[bytes] = None) -> torch.Tensor:
        need = self._workspace_bytes(batch, training, mask)
        if need < 0:
            raise GgError(lib().gg_last_error().decode())
        ws = self._ws.get(training)
        if ws is None or ws.numel() < need or ws.device != self._flat.device:
            ws = self._ws[training] = None          # let go of the old buffer first: at the large sizes the two do not fit side by side
            ws = self._ws[training] = torch.empty(need, dtype=torch.uint8, device=self._flat.device)
        return ws

    def set_recompute(self, enable: bool) -> bool:      # True if it changed: the training workspace was laid out for the other plan and is released
        changed = bool(enable) != bool(self.cfg.recompute)
        if changed:
            self.cfg.recompute = int(bool(enable))
            self._ws.pop(True, None)
        return changed

    def _prepare(self, batch: int, training: bool):      # -> (mask, workspace): a training workspace keeps no activation that only a frozen weight's gradient reads
        self._ensure_weights()
        mask = self.trainable_mask() if training else None
        return mask, self._workspace(batch, training, mask)

    def _record_forward(self, batch: int, mask: bytes, payload=None):      # after a TRAINING forward (an eval forward leaves the record alone)
        self._gen += 1
        self._last = (batch, payload, self._gen)
        self._train_mask, self._last_recompute = mask, self.cfg.recompute

    def _pending(self, gen: Optional[int], batch: Optional[int] = None):      # -> (batch, payload, workspace) of the forward a backward may use
        if self._last is None:
            raise GgError(f"{self._name} backward without a training forward")
        B, payload, last_gen = self._last
        if gen is not None and gen != last_gen:
            raise GgError(f"{self._name} backward for training forward #{gen}, but the workspace now holds the activations of forward "
                          f"#{last_gen}: {self._gen_why}every training forward must be followed by its backward before the next training forward")
        if batch is not None and batch != B:
            raise GgError(f"{self._name} backward: gradient batch {batch} != forward batch {B}")
        if self.cfg.recompute != self._last_recompute:
            raise GgError(f"{self._switch} changed between the training forward and its backward: the forward laid out its workspace for "
                          f"recompute={self._last_recompute} (the checkpointed layout keeps other tensors); run the forward again")
        ws = self._ws.get(True)
        if ws is None:
            raise GgError(f"{self._name} backward: the training workspace was released ({self._switch} changed since the training forward); "
                          "run the forward again")
        return B, payload, ws

    def _same_mask(self) -> bytes:      # the workspace was laid out (and activations were dropped) for the forward's mask: backward needs the same
        mask = self.trainable_mask()
        if mask != self._train_mask:
            changed = [t["name"] for t, a, b in zip(self.table, mask, self._train_mask) if bool(a) != bool(b)]
            raise GgError(self._mask_changed.format(changed=", ".join(changed[:4])))
        return mask

    def wants_grad(self) -> bool:
        return torch.is_grad_enabled() and any(p.requires_grad for p in self._params.values())

    def _anchor(self) -> torch.Tensor:
        """Zero-dim input that keeps the whole-encoder autograd node alive: parameter gradients go straight into the flat buffer (``p.grad`` views)."""
        if self._anchor_t is None or self._anchor_t.device != self._flat.device:
            self._anchor_t = torch.zeros((), device=self._flat.device, requires_grad=True)
        return self._anchor_t

    def _enter_node(self, ctx, trained: bool = True):          # from the model's EncoderNode.forward, after forward_hip
        ctx.enc, ctx.valid, ctx.gen = self, trained, self._gen


class EncoderNode(torch.autograd.Function):
    """Base of the models' whole-encoder autograd nodes: theirs is ``forward(ctx, enc, x, anchor, ...)``, which ends in ``enc._enter_node``."""
    @staticmethod
    def backward(ctx, *grads):
        if not ctx.valid:
            raise GgError(f"backward through a {ctx.enc._name} forward that ran in eval mode (running-stat BatchNorm keeps no "
                          "activations); call .train() before the forward pass")
        ctx.enc.backward_hip(*grads, ctx.gen)
        d_anchor = torch.zeros((), device=next(g for g in grads if g is not None).device)
        return (None, None, d_anchor) + (None,) * (len(ctx.needs_input_grad) - 3)
