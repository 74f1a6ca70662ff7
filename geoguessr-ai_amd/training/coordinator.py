"""The batch side of the reference's coordinator loop (``main_coordinator_idun_s3.py``): rows as ``LocalGeoMapDataset`` reads them -- a panorama's views as JPEG
file bytes, ``lat``, ``lon`` -- become what the model takes: ``pixel_values`` through a ``DevicePanoramaTransform`` (the dataset's resize and the loop's interpolation
and normalisation, :26-138 and :339-381, on the device), ``labels`` as (lon, lat) float32 and, with centroids, ``labels_clf`` as the nearest centroid's index
(:384-391).  Reading the rows from SQLite or S3 stays with the caller."""
from typing import Iterable, Optional, Sequence

import torch

from .. import ops
from .preprocess import DevicePanoramaTransform


class panorama_batches:
    """``rows`` (dicts with ``images`` -- a list of views -- or ``image``, and ``lat`` / ``lon``) -> ``{"pixel_values", "labels"[, "labels_clf"]}`` batches of
    ``batch_size`` rows, lazily, one ``transform`` call per batch: the twin of ``finetune_tinyvit.augmented`` / ``eval_transformed`` for the panorama fine-tune.  A view
    is JPEG file bytes, a raw image or ``None``; ``images`` rows give (n, V, 3, Ht, Wt) ``pixel_values``, ``image`` rows (n, 3, Ht, Wt).  ``centroids``: (K, 2) (lon, lat)
    float32; ``labels_clf = argmin haversine_matrix(labels, centroids)`` (``ops.haversine_matrix``).  ``shuffle``: a new order per walk, drawn from ``seed`` + the
    walk's number.  Like a DataLoader the object can be walked once per epoch."""

    def __init__(self, rows: Sequence[dict], batch_size: int, transform: DevicePanoramaTransform, centroids: Optional[torch.Tensor] = None, shuffle: bool = False,
                 seed: int = 0):
        if batch_size < 1:
            raise ValueError(f"panorama_batches: batch_size={batch_size}")
        self.rows, self.batch_size, self.transform, self.shuffle, self.seed = rows, int(batch_size), transform, bool(shuffle), int(seed)
        self.centroids = None if centroids is None else torch.as_tensor(centroids, dtype=torch.float32).to(transform.device).contiguous()
        self._walks = 0

    def __len__(self) -> int:
        return (len(self.rows) + self.batch_size - 1) // self.batch_size

    def order(self, walk: int) -> torch.Tensor:
        n = len(self.rows)
        return torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + walk)) if self.shuffle else torch.arange(n)

    def __iter__(self) -> Iterable[dict]:
        order = self.order(self._walks)
        self._walks += 1
        dev = self.transform.device
        for i in range(0, len(order), self.batch_size):
            rows = [self.rows[int(j)] for j in order[i:i + self.batch_size]]
            if all("images" in r for r in rows):
                views = [list(r["images"] or []) for r in rows]
            elif all("image" in r for r in rows):
                views = [r["image"] for r in rows]
            else:
                raise KeyError("panorama_batches: every row needs 'images' (or every row 'image')")
            labels = torch.tensor([[float(r["lon"]), float(r["lat"])] for r in rows], dtype=torch.float32).to(dev)
            batch = {"pixel_values": self.transform(views), "labels": labels}
            if self.centroids is not None:
                batch["labels_clf"] = torch.argmin(ops.haversine_matrix(labels, self.centroids), dim=-1)
            yield batch
