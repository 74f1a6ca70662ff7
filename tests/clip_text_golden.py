"""Loader of tests/golden/clip_text_tiny.npz (written by tests/golden/make_golden_clip_text.py from transformers' CLIPModel) for the CPU and GPU tests of the
contrastive pre-training stage."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SCALE = 2.0 ** -11
TINY = dict(text=dict(hidden_size=128, intermediate_size=256, num_layers=2, num_heads=2, vocab_size=64, max_positions=77, eos_token_id=63),
            vision=dict(hidden_size=128, intermediate_size=256, num_layers=2, num_heads=2, image_size=32, patch_size=8), projection_dim=64)
MASKS = {
    "ref": lambda n: "visual_projection" in n or n == "logit_scale",
    "ref_text": lambda n: "visual_projection" in n or n == "logit_scale" or "text_projection" in n,
    "ref_vis": lambda n: "visual_projection" in n or n == "logit_scale" or n.startswith("vision_model.encoder.layers.1.") or n.startswith("vision_model.post_layernorm"),
}
_cache = {}


def load():
    if "z" not in _cache:
        z = np.load(os.path.join(HERE, "golden", "clip_text_tiny.npz"))
        _cache["z"] = {k: z[k] for k in z.files}
        g = np.load(os.path.join(HERE, "golden", "clip_text_tiny_grads.npz"))          # the gradients of the big matrices, whole
        _cache["z"].update({k: g[k] for k in g.files})
    return _cache["z"]


def decode_state_dict(z=None):
    """HF key -> float32 tensor: `q.` entries are int8 multiples of 2^-11, `w.` entries float32."""
    z = z or load()
    sd = {}
    for k, v in z.items():
        if k.startswith("q."):
            sd[k[2:]] = torch.from_numpy(v.astype(np.float32) * np.float32(SCALE))
        elif k.startswith("w."):
            sd[k[2:]] = torch.from_numpy(v.astype(np.float32))
    return sd


def tiny_config(eos_token_id=63):
    c = dict(TINY)
    c["text"] = dict(TINY["text"], eos_token_id=eos_token_id)
    return c
