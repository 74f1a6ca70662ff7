"""Mirror of the reference's ``finetune_tinyvit`` package: the TinyViT country-classifier fine-tune (``train_tinyvit_timm.py``) and the feature export
(``extract_embeddings.py``) on ``models.tinyvit_classifier.TinyViTClassifier``, and the training transform of its dataset (timm's random-resized-crop, flip and
RandAugment) as a batched device transform (``augment.py``).  Host-side data loading (the CSV datasets, ``prepare_dataset.py``) is not mirrored: the loops take
batches that are already on the device -- ``pixel_values``, or raw uint8 images through ``augmented`` (training) or ``eval_transformed`` (validation, feature
export) -- and the eval transform is the ``"timm"`` pipeline of ``training/preprocess.py``."""
from .train_tinyvit_timm import build_class_map, class_id, cosine_lr, create_model, evaluate, train                    # noqa: F401
from .extract_embeddings import embeddings_frame, extract_embeddings, load_model_for_features, write_parquet          # noqa: F401
from .augment import DeviceTrainTransform, augmented, eval_transformed, sample_params                                  # noqa: F401
