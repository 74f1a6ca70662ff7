"""Writes tests/golden/clip_interp_tiny.npz: transformers' own ``CLIPVisionModel(pixel_values, interpolate_pos_encoding=True)`` on the CPU (fp32) for the tiny
tower of tests/clip_interp_cases.py at two foreign input sizes -- 40 x 56 (a 5 x 7 grid: non-square upscale) and 24 x 24 (3 x 3: downscale).  Per size:
``last_hidden_state`` (no post_layernorm), its token mean, and the gradient of ``pooled.square().sum()`` with respect to the position table (through the library's
``F.interpolate``).  The file carries the seeds and the configuration, no weights: tests regenerate weights and inputs from tests/clip_interp_cases.py, and two
checksums catch a changed rng stream.

Run from the repository root:  python tests/golden/make_golden_clip_interp.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import clip_interp_cases as IC      # noqa: E402

SIZES = [(40, 56), (24, 24)]


def main():
    import transformers
    from transformers import CLIPVisionConfig, CLIPVisionModel
    hs, inter, nl, nh, img, ps = IC.TINY
    cfg = CLIPVisionConfig(hidden_size=hs, intermediate_size=inter, num_hidden_layers=nl, num_attention_heads=nh, image_size=img, patch_size=ps,
                           hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0)
    cfg._attn_implementation = "eager"
    model = CLIPVisionModel(cfg).eval()
    st = IC.tiny_weights()
    own = model.state_dict()
    prefix = "vision_model." if any(k.startswith("vision_model.") for k in own) else ""      # transformers 4.x nests, 5.x is flat
    missing, unexpected = model.load_state_dict({prefix + k: v for k, v in st.items()}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    pos = [p for n, p in model.named_parameters() if n.endswith("embeddings.position_embedding.weight")][0]
    out = dict(cfg=np.array(IC.TINY, np.int64), weight_seed=np.int64(IC.WEIGHT_SEED), sizes=np.array(SIZES, np.int64),
               transformers_version=np.array(transformers.__version__),
               w_checksum=np.float64(sum(float(v.double().sum()) for v in st.values())))
    for H, W in SIZES:
        x = IC.tiny_input(H, W)
        model.zero_grad()
        lh = model(pixel_values=x, interpolate_pos_encoding=True).last_hidden_state
        assert lh.shape == (x.shape[0], (H // ps) * (W // ps) + 1, hs)
        pooled = lh.mean(dim=1)
        pooled.square().sum().backward()
        key = f"{H}x{W}"
        out["x_checksum." + key] = np.float64(x.double().sum())
        out["last_hidden_state." + key] = lh.detach().numpy()
        out["pooled." + key] = pooled.detach().numpy()
        out["g_pos." + key] = pos.grad.detach().numpy().copy()
        # the restatement the tests' references are built on (tests/clip_interp_cases.py) against the library's own embeddings (the same F.interpolate: 0 here)
        emb = model.vision_model.embeddings if hasattr(model, "vision_model") else model.embeddings
        with torch.no_grad():
            e = emb(x, interpolate_pos_encoding=True)
            pe = emb.patch_embedding(x).flatten(2).transpose(1, 2)
            mine = torch.cat([emb.class_embedding.expand(x.shape[0], 1, -1), pe], 1) + IC.torch_interp(pos.detach(), H // ps, W // ps)[None]
        print(f"{key}: last_hidden {tuple(lh.shape)}, |g_pos| {float(pos.grad.norm()):.4f}, embeddings restated to {float((e - mine).abs().max()):.2e}")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_interp_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
