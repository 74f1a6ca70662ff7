"""Shared cases of the CLIP position-table resampling (include/gg_clip_interp.h) and of the tower at a foreign input size: the geometries, the fp64 reference --
the separable matrix form ``W_h . grid . W_w^T`` of torch's bicubic ``F.interpolate(align_corners=False)``: ``W_*`` is (Gout, Gs), Keys' weights with A = -0.75 at the
source coordinate ``(o + 0.5) Gs / Gout - 0.5``, a tap clamped to the border adding into the border column --, transformers' own restatement through
``F.interpolate``, and the tiny tower (hidden 128, 2 heads, intermediate 256, 2 layers, patch 8, image_size 32: a 4 x 4 grid, 17 tokens) with weights and inputs
seeded from numpy.  A plain module: no fixtures, no GPU."""
import numpy as np
import torch
import torch.nn.functional as F

# (Gs, Gh, Gw): upscale to a non-square grid; downscale; one side up and one down; a 2 x 2 table (every tap clamped); several blocks; ViT-L/14 336 -> 448; identity
GEOMETRIES = [(4, 5, 7), (4, 3, 3), (4, 9, 2), (2, 5, 3), (7, 16, 16), (24, 32, 32), (4, 4, 4)]
A = -0.75

TINY = (128, 256, 2, 2, 32, 8)      # hidden, intermediate, layers, heads, image_size, patch_size (tests/clip_golden.py's order)
WEIGHT_SEED = 20240917


def cubic_matrix(Gs: int, Gout: int) -> np.ndarray:
    """(Gout, Gs) fp64: row o holds the four cubic-convolution weights of destination index o, clamped taps summed into the border column."""
    Wm = np.zeros((Gout, Gs), np.float64)
    for o in range(Gout):
        s = (o + 0.5) * Gs / Gout - 0.5
        i0 = int(np.floor(s))
        t = s - i0
        w = [((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A,
             ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1,
             ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A]
        for a in range(4):
            Wm[o, min(max(i0 - 1 + a, 0), Gs - 1)] += w[a]
    return Wm


def interp_ref(pos, Gh: int, Gw: int) -> np.ndarray:
    """pos (Gs * Gs + 1, D) -> (Gh * Gw + 1, D), fp64: the class row kept, the grid as W_h . grid . W_w^T, flattened row-major."""
    pos = np.asarray(pos, np.float64)
    Gs = int(round((pos.shape[0] - 1) ** 0.5))
    assert Gs * Gs + 1 == pos.shape[0]
    grid = pos[1:].reshape(Gs, Gs, -1)
    out = np.einsum("ys,sxd,wx->ywd", cubic_matrix(Gs, Gh), grid, cubic_matrix(Gs, Gw))
    return np.concatenate([pos[:1], out.reshape(Gh * Gw, -1)], 0)


def interp_ref_bwd(d_out, Gs: int, Gh: int, Gw: int) -> np.ndarray:
    """The transposed form: d_out (Gh * Gw + 1, D) -> (Gs * Gs + 1, D), fp64."""
    d_out = np.asarray(d_out, np.float64)
    g = d_out[1:].reshape(Gh, Gw, -1)
    d = np.einsum("ys,ywd,wx->sxd", cubic_matrix(Gs, Gh), g, cubic_matrix(Gs, Gw))
    return np.concatenate([d_out[:1], d.reshape(Gs * Gs, -1)], 0)


def torch_interp(pos: torch.Tensor, Gh: int, Gw: int) -> torch.Tensor:
    """transformers' CLIPVisionEmbeddings.interpolate_pos_encoding restated on a bare table, in ``pos``'s dtype (differentiable).  At the native square grid
    the library returns the table as it is."""
    Gs = int(round((pos.shape[0] - 1) ** 0.5))
    if Gh == Gs and Gw == Gs:
        return pos
    D = pos.shape[1]
    patch = pos[1:].reshape(1, Gs, Gs, D).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(Gh, Gw), mode="bicubic", align_corners=False)
    return torch.cat([pos[:1], patch.permute(0, 2, 3, 1).reshape(Gh * Gw, D)], 0)


def table(Gs: int, D: int, seed: int) -> np.ndarray:
    """An N(0, 1) f32 table (Gs * Gs + 1, D)."""
    return np.random.default_rng(seed).standard_normal((Gs * Gs + 1, D), dtype=np.float32)


def tiny_spec():
    from oracle import clip_ref as R
    hs, inter, nl, nh, img, ps = TINY
    return R.ClipVisionConfig(hidden_size=hs, intermediate_size=inter, num_hidden_layers=nl, num_attention_heads=nh, image_size=img, patch_size=ps)


def tiny_weights(seed: int = WEIGHT_SEED, image_size: int = None):
    """{HF name without ``vision_model.``: f32 tensor} of the tiny tower, one numpy stream in oracle.clip_ref.param_spec's order: LayerNorm gains 1 + 0.1 N,
    biases 0.05 N, the class and position rows 0.3 N (the position table carries weight in the token sum), matrices 0.05 N.  ``image_size``: another native size
    (its position table is drawn LAST, so every other tensor is the same)."""
    from oracle import clip_ref as R
    cfg = tiny_spec()
    if image_size is not None:
        cfg.image_size = image_size
    rng = np.random.default_rng(seed)
    st, pos_shape = {}, None
    for name, shape in R.param_spec(cfg):
        if name == "embeddings.position_embedding.weight":
            pos_shape = shape
            continue
        n = rng.standard_normal(shape, dtype=np.float32)
        if name.endswith(("norm.weight", "norm1.weight", "norm2.weight")):
            v = np.float32(1.0) + np.float32(0.1) * n
        elif name.endswith(".bias"):
            v = np.float32(0.05) * n
        elif name == "embeddings.class_embedding":
            v = np.float32(0.3) * n
        else:
            v = np.float32(0.05) * n
        st[name] = torch.from_numpy(v)
    st["embeddings.position_embedding.weight"] = torch.from_numpy(np.float32(0.3) * rng.standard_normal(pos_shape, dtype=np.float32))
    return {name: st[name] for name, _ in R.param_spec(cfg)}


def tiny_input(H: int, W: int, B: int = 2, seed: int = 7) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed * 100003 + H * 1009 + W).standard_normal((B, 3, H, W), dtype=np.float32))


def tiny_tower(precision: str, image_size: int = None, weights=None, **kw):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    hs, inter, nl, nh, img, ps = TINY
    tower = CLIPVisionTower("openai/clip-vit-tiny-interp", hidden_size=hs, intermediate_size=inter, num_layers=nl, num_heads=nh,
                            image_size=image_size or img, patch_size=ps, precision=precision, **kw)
    tower.load_hf_state_dict(weights if weights is not None else tiny_weights(image_size=image_size))
    return tower


def oracle_forward(st, x, dtype=torch.float64):
    """oracle.clip_ref.forward fed the torch-interpolated table (the oracle takes any token count): pooled (B, D) in ``dtype``."""
    from oracle import clip_ref as R
    ps = TINY[5]
    st = {k: v.to(dtype) for k, v in st.items()}
    st["embeddings.position_embedding.weight"] = torch_interp(st["embeddings.position_embedding.weight"], x.shape[2] // ps, x.shape[3] // ps)
    return R.forward(tiny_spec(), st, x.to(dtype))


def oracle_grads(st, x):
    """fp64 autograd of ``pooled.square().sum()`` through oracle_forward: (pooled, {name: gradient}), the position table's through F.interpolate's own backward."""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in st.items()}
    from oracle import clip_ref as R
    ps = TINY[5]
    stg = dict(leaves)
    stg["embeddings.position_embedding.weight"] = torch_interp(leaves["embeddings.position_embedding.weight"], x.shape[2] // ps, x.shape[3] // ps)
    pooled = R.forward(tiny_spec(), stg, x.double())
    pooled.square().sum().backward()
    return pooled.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
