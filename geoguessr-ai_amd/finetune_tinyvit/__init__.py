"""Mirror of the reference's ``finetune_tinyvit`` package: the TinyViT country-classifier fine-tune (``train_tinyvit_timm.py``) and the feature export
(``extract_embeddings.py``) on ``models.tinyvit_classifier.TinyViTClassifier``.  Host-side data loading (the CSV datasets, timm's RandAugment transform,
``prepare_dataset.py``) is not mirrored: the loops take batches that are already on the device; the eval transform is the ``"timm"`` pipeline of
``training/preprocess.py``."""
from .train_tinyvit_timm import build_class_map, class_id, cosine_lr, create_model, evaluate, train                    # noqa: F401
from .extract_embeddings import embeddings_frame, extract_embeddings, load_model_for_features, write_parquet          # noqa: F401
