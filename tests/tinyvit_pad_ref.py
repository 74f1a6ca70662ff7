"""The oracle's TinyVitBlock (oracle/tinyvit_ref.py::_tinyvit_block_m) with timm's padding path (timm 1.0.21 ``TinyVitBlock.forward``): a token map that the window
does not divide is zero-padded at the bottom and right up to a multiple of the window IN FRONT of the attention module (so in front of ``attn.norm``), window-partitioned,
attended -- nothing masks the pad tokens: LayerNorm maps a zero row to ``norm.bias``, so they carry the constant ``qkv(norm.bias)`` as key and value -- window-reversed
and cropped back to the map.  The oracle itself asserts divisibility; the tests install this block with ``monkeypatch.setattr(R, "_tinyvit_block_m", tinyvit_block_padded)``
(``R.forward`` looks the name up at call time).  On a map that divides it runs the oracle's own operations in the oracle's order.

``mask_pad_keys=True`` is NOT timm: the variant that hides the pad tokens from the softmax, kept to show that the tests tell the two apart."""
import torch
import torch.nn.functional as F

from oracle import tinyvit_ref as R


def padded_side(res: int, ws: int) -> int:
    return res + (ws - res % ws) % ws


def _attention_masked(c, x, p, nh, ws, valid):
    """R._attention with the keys where ``valid`` (B', N) is False left out of the softmax (plain fp arithmetic only: the masked variant is a CPU comparison)."""
    C = x.shape[-1]
    st = c.st
    xn = F.layer_norm(x, (C,), st[f"{p}.attn.norm.weight"], st[f"{p}.attn.norm.bias"], c.cfg.ln_eps)
    Bw, N, _ = xn.shape
    hd = C // nh
    qkv = F.linear(xn, st[f"{p}.attn.qkv.weight"], st[f"{p}.attn.qkv.bias"])
    q, k, v = qkv.view(Bw, N, nh, 3 * hd).split([hd, hd, hd], dim=3)
    q, k, v = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    bias = st[f"{p}.attn.attention_biases"][:, R.attention_bias_idxs(ws)]
    attn = (q @ k.transpose(-2, -1)) * (hd ** -0.5) + bias
    attn = attn.masked_fill(~valid[:, None, None, :], float("-inf"))
    o = (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(Bw, N, C)
    return F.linear(o, st[f"{p}.attn.proj.weight"], st[f"{p}.attn.proj.bias"])


def tinyvit_block_padded(c, x, p, nh, ws, masks, blk, mask_pad_keys=False):
    B, H, W, C = x.shape
    L = H * W
    sc = x
    if H == ws and W == ws:
        a = R._attention(c, x.reshape(B, L, C), p, nh, ws).view(B, H, W, C)
    else:
        pad_b, pad_r = (ws - H % ws) % ws, (ws - W % ws) % ws
        padded = pad_b > 0 or pad_r > 0
        xp = F.pad(x, (0, 0, 0, pad_r, 0, pad_b)) if padded else x
        pH, pW = H + pad_b, W + pad_r
        nH, nW = pH // ws, pW // ws
        xw = xp.view(B, nH, ws, nW, ws, C).transpose(2, 3).reshape(B * nH * nW, ws * ws, C)
        if mask_pad_keys and padded:
            valid = torch.zeros(B, pH, pW, dtype=torch.bool)
            valid[:, :H, :W] = True
            valid = valid.view(B, nH, ws, nW, ws).transpose(2, 3).reshape(B * nH * nW, ws * ws)
            a = _attention_masked(c, xw, p, nh, ws, valid)
        else:
            a = R._attention(c, xw, p, nh, ws)
        a = a.view(B, nH, nW, ws, ws, C).transpose(2, 3).reshape(B, pH, pW, C)
        if padded:
            a = a[:, :H, :W].contiguous()
    s1 = masks.scale(blk, 0) if masks is not None else None
    if s1 is not None:
        a = a * s1[:, None, None, None]
    x = c.q(sc + a)
    c.tap(f"{p}.x1", x)
    x = x.permute(0, 3, 1, 2)
    x = c.q(R._convnorm(c, x, f"{p}.local_conv", 1, 1, C, dense=False))
    x = x.reshape(B, C, L).transpose(1, 2)
    c.tap(f"{p}.x2", x)
    st = c.st
    h = c.q(F.layer_norm(x, (C,), st[f"{p}.mlp.norm.weight"], st[f"{p}.mlp.norm.bias"], c.cfg.ln_eps))
    h = F.linear(h, c.w(f"{p}.mlp.fc1.weight"), st[f"{p}.mlp.fc1.bias"])
    h = c.q(F.gelu(c.q(h)))
    h = F.linear(h, c.w(f"{p}.mlp.fc2.weight"), st[f"{p}.mlp.fc2.bias"])
    s2 = masks.scale(blk, 1) if masks is not None else None
    if s2 is not None:
        h = h * s2[:, None, None]
    x = c.q(x + h)
    c.tap(f"{p}.out", x)
    return x.view(B, H, W, C)


def windows_to_padded_map(t, batch, pres, ws):
    """The oracle taps ``attn.out`` per window, (B * nH * nW, ws * ws, C); the runtime keeps the padded map's row order, (B, pres * pres, C)."""
    C = t.shape[-1]
    n = pres // ws
    return t.view(batch, n, n, ws, ws, C).transpose(2, 3).reshape(batch, pres * pres, C)


# the four padded cases of the tests: (variant, img_size, depths or None = the variant's, images of the CPU plan / oracle checks)
PAD_CASES = [("tiny_vit_5m_224", 160, None, 8), ("tiny_vit_5m_224", 256, None, 4), ("tiny_vit_21m_384", 288, (1, 1, 2, 1), 4), ("tiny_vit_21m_512", 320, (1, 1, 1, 1), 4)]
