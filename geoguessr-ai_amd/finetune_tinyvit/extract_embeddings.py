"""Drop-in for the reference's ``finetune_tinyvit/extract_embeddings.py`` (:52-118): reload the best checkpoint, run the pooled last feature map of every
image (``forward_to_emb``: ``forward_features`` + ``adaptive_avg_pool2d`` -- no ``head.norm``), lay the rows out as
``location_id, filepath, lat, lon, country, emb_0 .. emb_{D-1}``.  Writing Parquet needs ``pyarrow`` or ``fastparquet``; neither is a dependency of this
package, so ``write_parquet`` says so instead of failing inside pandas."""
from __future__ import annotations

import importlib.util
import os
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from ..models.tinyvit_classifier import TinyViTClassifier

META_COLUMNS = ("location_id", "filepath", "lat", "lon", "country")


def load_model_for_features(ckpt_path: str, model_name: str = "tiny_vit_5m_224", **overrides) -> Tuple[TinyViTClassifier, Dict[str, int]]:
    """``num_classes`` is the size of the checkpoint's ``class_to_id`` (1 when it is empty or absent); the weights load with ``strict=False``, so a head
    of another size (the UNKNOWN quirk grows the map after the model was built) is skipped while the encoder loads.  The model comes back in eval mode,
    on the CPU: move it with ``.to("cuda")``."""
    ckpt = torch.load(ckpt_path, map_location="cpu")
    class_to_id = ckpt.get("class_to_id", {}) or {}
    model = TinyViTClassifier(model_name, num_classes=len(class_to_id) if class_to_id else 1, pretrained=False, **overrides)
    model.load_state_dict(ckpt["model"], strict=False)
    model.eval()
    return model, class_to_id


def extract_embeddings(model: TinyViTClassifier, batches: Iterable) -> np.ndarray:
    """(rows, D) float32: ``model.pooled_features`` of every batch (a dict with ``"pixel_values"``, or the tensor itself), in order."""
    model.eval()
    rows = []
    for batch in batches:
        x = batch["pixel_values"] if isinstance(batch, dict) else batch
        rows.append(model.pooled_features(x).cpu().numpy())
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, model.num_features), dtype=np.float32)


def embeddings_frame(embeddings: np.ndarray, metas: Optional[Sequence[dict]] = None):
    """The reference's table: one row per image, the metadata columns (a missing one is None) and then ``emb_0 .. emb_{D-1}``."""
    import pandas as pd
    emb = np.asarray(embeddings)
    metas = [{}] * emb.shape[0] if metas is None else list(metas)
    if len(metas) != emb.shape[0]:
        raise ValueError(f"embeddings_frame: {len(metas)} metadata rows for {emb.shape[0]} embeddings")
    cols = {c: [m.get(c) for m in metas] for c in META_COLUMNS}
    cols.update({f"emb_{j}": emb[:, j] for j in range(emb.shape[1])})
    return pd.DataFrame(cols)


def write_parquet(df, out_parquet: str) -> None:
    if importlib.util.find_spec("pyarrow") is None and importlib.util.find_spec("fastparquet") is None:
        raise RuntimeError("write_parquet: pandas needs pyarrow or fastparquet to write Parquet and neither is installed; install one of them, or keep "
                           "the DataFrame of embeddings_frame() (e.g. DataFrame.to_csv / numpy.save)")
    d = os.path.dirname(out_parquet)
    if d:
        os.makedirs(d, exist_ok=True)
    df.to_parquet(out_parquet, index=False)
    print(f"Wrote embeddings to {out_parquet} with shape {df.shape}")
