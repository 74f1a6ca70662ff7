"""CPU restatement (torch) of the fp8 mode's numerics contract (include/gg_fp8.h) for the tests of the CLIP tower's fp8 inference mode:

* ``quant_rows``: one f32 scale per row, OCP e4m3fn codes -- every step in f32, in the order the header states it;
* ``forward_fp8``: the op sequence of ``oracle/clip_ref.forward`` in fp64 (restated here: the oracle exports no per-op hooks), with ``quant_rows`` on the
  input rows and the weight rows of the four Linears of every encoder layer.  ``quant=False`` is the unquantised fp64 forward both error measures refer to.

A plain module: no fixtures, no GPU."""
import torch
import torch.nn.functional as F

E4M3_MAX = 448.0


def quant_rows(x):
    """x [..., K] (any float dtype; taken to f32) -> (codes uint8 [..., K], scale f32 [...]).  amax over the row; scale = amax / 448 and inv = 448 / amax as f32
    divisions; code = e4m3fn(x * inv) (one f32 multiply, round-to-nearest-even, saturating); a zero row gets scale 1 and zero codes."""
    x = x.to(torch.float32)
    amax = x.abs().amax(-1, keepdim=True)
    c448 = torch.tensor(E4M3_MAX, dtype=torch.float32)
    zero = amax == 0
    safe = torch.where(zero, torch.ones_like(amax), amax)
    scale = torch.where(zero, torch.ones_like(amax), safe / c448)
    inv = c448 / safe
    codes = (x * inv).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    codes = torch.where(zero, torch.zeros_like(codes), codes)
    return codes, scale.squeeze(-1)


def decode(codes):
    """uint8 e4m3fn codes -> fp64 values."""
    return codes.contiguous().view(torch.float8_e4m3fn).to(torch.float32).double()


def dequant(codes, scale):
    return decode(codes) * scale.double().unsqueeze(-1)


def e4m3_spacing(v):
    """Distance between neighbouring e4m3 values at magnitude v (fp64 tensor): 2^(floor(log2 v) - 3) from 2^-6 up, 2^-9 below."""
    v = v.abs().double().clamp(max=E4M3_MAX)
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** -6)))
    return torch.where(v >= 2.0 ** -6, 2.0 ** (e - 3), torch.full_like(v, 2.0 ** -9))


def _linear(a, W, b, quant):
    if quant:
        a, W = dequant(*quant_rows(a)), dequant(*quant_rows(W))
    return a @ W.T + b


def forward_fp8(cfg, st, x, quant=True):
    """cfg = (hidden, intermediate, layers, heads, image, patch); st: HF names without ``vision_model.``; x (B,3,H,W).  -> (pooled (B,D), last_hidden (B,T,D)), fp64."""
    hs, inter, nl, nh, img, ps = cfg
    st = {k: v.double() for k, v in st.items()}
    x = x.double()
    D, hd, B, eps = hs, hs // nh, x.shape[0], 1e-5
    pe = F.conv2d(x, st["embeddings.patch_embedding.weight"], None, ps).flatten(2).transpose(1, 2)
    h = torch.cat([st["embeddings.class_embedding"].expand(B, 1, D), pe], 1) + st["embeddings.position_embedding.weight"][None]
    h = F.layer_norm(h, (D,), st["pre_layrnorm.weight"], st["pre_layrnorm.bias"], eps)
    for i in range(nl):
        p = f"encoder.layers.{i}"
        a = F.layer_norm(h, (D,), st[p + ".layer_norm1.weight"], st[p + ".layer_norm1.bias"], eps)
        W = torch.cat([st[p + f".self_attn.{n}_proj.weight"] for n in "qkv"])
        b = torch.cat([st[p + f".self_attn.{n}_proj.bias"] for n in "qkv"])
        qkv = _linear(a, W, b, quant)
        T = h.shape[1]
        qq, kk, vv = (u.reshape(B, T, nh, hd).transpose(1, 2) for u in qkv.split(D, -1))
        o = (((qq @ kk.transpose(-2, -1)) * hd ** -0.5).softmax(-1) @ vv).transpose(1, 2).reshape(B, T, D)
        h = h + _linear(o, st[p + ".self_attn.out_proj.weight"], st[p + ".self_attn.out_proj.bias"], quant)
        m = F.layer_norm(h, (D,), st[p + ".layer_norm2.weight"], st[p + ".layer_norm2.bias"], eps)
        m = _linear(m, st[p + ".mlp.fc1.weight"], st[p + ".mlp.fc1.bias"], quant)
        m = m * torch.sigmoid(1.702 * m)
        h = h + _linear(m, st[p + ".mlp.fc2.weight"], st[p + ".mlp.fc2.bias"], quant)
    return h.mean(1), h


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm())


def one_minus_cos(a, b):
    """Worst 1 - cosine over the rows of two (B, D) embeddings."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((1.0 - F.cosine_similarity(a, b, dim=-1)).max())


def seeded_state(cfg, seed=0):
    """Random weights at a real shape, with the spread of a trained tower's tensors that matters to the quantiser: unit LayerNorm gains with noise, small biases."""
    from oracle import clip_ref as R
    hs, inter, nl, nh, img, ps = cfg
    c = R.ClipVisionConfig(hidden_size=hs, intermediate_size=inter, num_hidden_layers=nl, num_attention_heads=nh, image_size=img, patch_size=ps)
    g = torch.Generator().manual_seed(seed)
    st = {}
    for name, shape in R.param_spec(c):
        if name.endswith(("norm.weight", "norm1.weight", "norm2.weight")):
            st[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            st[name] = 0.02 * torch.randn(shape, generator=g)
        else:
            st[name] = 0.02 * torch.randn(shape, generator=g)
    return st
