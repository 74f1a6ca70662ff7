"""Drop-in for the loop of the reference's ``finetune_tinyvit/train_tinyvit_timm.py`` (:122-210): ``create_model`` / ``evaluate`` / ``train`` with the same
hyper-parameters (AdamW lr 5e-4, weight decay 0.05 on every parameter, cosine annealing stepped per epoch, plain mean cross-entropy), the same metrics
(top-1 / top-5 in percent, weighted by batch size), the same per-epoch line and the same ``best.pt`` layout (``{"model", "class_to_id", "args"}``).

Differences, on purpose: batches arrive on the device (any iterable of ``{"pixel_values", "labels"}``; an iterable that can be walked once per epoch,
e.g. a list or a DataLoader); there is no fp16 autocast and no GradScaler -- the arithmetic is the model's precision mode (fp32 / fp32_split / bf16),
unscaled; the checkpoint's tensors are saved from the CPU."""
from __future__ import annotations

import math
import os
from typing import Dict, Iterable, Optional

import torch

from ..models.tinyvit_classifier import TinyViTClassifier
from ..optim import AdamW


def build_class_map(countries: Iterable) -> Dict[str, int]:
    """``ImageCSVDataset.__init__`` (:39-41): the unique country strings, sorted, numbered from 0."""
    return {c: i for i, c in enumerate(sorted({str(c) for c in countries}))}


def class_id(class_to_id: Dict[str, int], country) -> int:
    """``ImageCSVDataset.__getitem__`` (:71), quirk included: a country the map has not seen becomes ``class_to_id.setdefault("UNKNOWN", 0)`` -- the map
    GAINS the key "UNKNOWN" with id 0, so every unseen label is trained and scored as class 0 (the alphabetically first country), and ``len(class_to_id)``
    grows by one from then on (which is what ``load_model_for_features`` reads as ``num_classes``)."""
    name = str(country)
    if name in class_to_id:
        return int(class_to_id[name])
    return int(class_to_id.setdefault("UNKNOWN", 0))


def cosine_lr(epoch: int, epochs: int, lr: float) -> float:
    """Closed form of ``CosineAnnealingLR(T_max=epochs)`` (eta_min 0) after ``epoch`` scheduler steps."""
    return lr * (1.0 + math.cos(math.pi * epoch / epochs)) / 2.0


def create_model(num_classes: int, model_name: str = "tiny_vit_5m_224", pretrained: bool = True, **overrides) -> TinyViTClassifier:
    return TinyViTClassifier(model_name, num_classes=num_classes, pretrained=pretrained, **overrides)


def evaluate(model: TinyViTClassifier, batches: Iterable, device=None) -> Dict[str, float]:
    """``{"val_top1", "val_top5"}`` in percent (``timm.utils.accuracy`` with ``topk=(1, min(5, C))``), weighted by batch size.  The hits come from the
    kernel's ``rank`` (top-k hit <=> rank < k)."""
    model.eval()
    hit1 = hit5 = n = 0
    with torch.no_grad():
        for batch in batches:
            x, y = batch["pixel_values"], batch["labels"]
            logits = model(x)
            _, rank = model.loss_and_metrics(logits, y)
            k = min(5, logits.shape[1])
            h1, h5 = torch.stack([(rank < 1).sum(), (rank < k).sum()]).tolist()
            hit1, hit5, n = hit1 + h1, hit5 + h5, n + int(y.numel())
    return {"val_top1": 100.0 * hit1 / max(1, n), "val_top5": 100.0 * hit5 / max(1, n)}


def _plain(args) -> dict:
    """``vars(args)`` of the reference's checkpoint as a dict of plain values (anything else is saved as its string)."""
    if args is None:
        return {}
    d = dict(args) if isinstance(args, dict) else dict(vars(args))
    return {str(k): (v if isinstance(v, (bool, int, float, str, type(None))) else str(v)) for k, v in d.items()}


def train(model: TinyViTClassifier, train_batches: Iterable, val_batches: Iterable, epochs: int = 5, lr: float = 5e-4, weight_decay: float = 0.05,
          out_dir: str = "finetune_tinyvit/outputs", class_to_id: Optional[Dict[str, int]] = None, args=None) -> Dict[str, float]:
    """The reference's epoch loop (:169-210).  Returns ``{"best_top1", "best_ckpt", "history"}``."""
    os.makedirs(out_dir, exist_ok=True)
    optimizer = AdamW(model, lr=lr, weight_decay=weight_decay)          # every trainable parameter decays, norms and biases included (as model.parameters() does)
    best_top1, best_ckpt, history = -1.0, os.path.join(out_dir, "best.pt"), []
    for epoch in range(1, epochs + 1):
        optimizer.param_groups[0]["lr"] = cosine_lr(epoch - 1, epochs, lr)
        model.train()
        running_loss, seen = 0.0, 0
        for batch in train_batches:
            x, y = batch["pixel_values"], batch["labels"]
            optimizer.zero_grad(set_to_none=True)
            loss, _ = model.loss_and_metrics(model(x), y)
            loss.backward()
            optimizer.step()
            running_loss += float(loss.detach()) * int(y.numel())
            seen += int(y.numel())
        metrics = evaluate(model, val_batches)
        avg_loss = running_loss / max(1, seen)
        history.append(dict(epoch=epoch, loss=avg_loss, lr=optimizer.param_groups[0]["lr"], **metrics))
        print(f"Epoch {epoch:02d}/{epochs} | loss {avg_loss:.4f} | val@1 {metrics['val_top1']:.3f} | val@5 {metrics['val_top5']:.3f}")
        if metrics["val_top1"] > best_top1:
            best_top1 = metrics["val_top1"]
            torch.save({"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "class_to_id": dict(class_to_id or {}),
                        "args": _plain(args)}, best_ckpt)
            print(f"Saved best checkpoint to {best_ckpt}")
    return {"best_top1": best_top1, "best_ckpt": best_ckpt, "history": history}
