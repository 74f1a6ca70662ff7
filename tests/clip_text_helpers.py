"""Helpers shared by the GPU tests of include/gg_clip_text.h and by tools/make_flash_parent_golden.py: seeded qkv buffers, a raw GgAttnArgs call and the fp64
attention reference.  A plain module (no tests, no fixtures)."""
import ctypes as C

import torch


def causal(L, qkv, B, T, H, dtype, ld, want_lse=True, D=64, fn="gg_attention_causal_fwd", **over):
    """qkv: (B*T, ld) buffer whose columns [0, 3*H*D) hold q | k | v.  Returns rc, out (B*T, H*D), lse (B*T, H)."""
    dt = torch.bfloat16 if dtype == 0 else torch.float32
    out = torch.full((B * T, H * D), float("nan"), dtype=dt, device="cuda")
    lse = torch.full((B * T, H), float("nan"), dtype=torch.float32, device="cuda") if want_lse else None
    a = L.AttnArgs()
    a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), ld, 0, H * D, 2 * H * D, D, D
    a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = H, B, T, 0, D ** -0.5
    a.out, a.ldo, a.lse = out.data_ptr(), H * D, (lse.data_ptr() if want_lse else None)
    for k, v in over.items():
        setattr(a, k, v)
    rc = getattr(L.lib(), fn)(C.byref(a), dtype, L.stream())
    torch.cuda.synchronize()
    return rc, out, lse


def attn_ref(q, k, v, is_causal=True):
    """fp64: q, k, v (B, T, H, D) -> out (B*T, H*D), lse (B*T, H)."""
    B, T, H, D = q.shape
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * D ** -0.5
    if is_causal:
        s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool, device=q.device), 1), float("-inf"))
    lse = torch.logsumexp(s, -1)
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.double())
    return o.reshape(B * T, H * D), lse.permute(0, 2, 1).reshape(B * T, H)


def make_qkv(B, T, H, dtype, seed, pad=8):
    g = torch.Generator().manual_seed(seed)
    W = 3 * H * 64
    buf = torch.randn(B * T, W + pad, generator=g).cuda()
    if dtype == 0:
        buf = buf.to(torch.bfloat16)
    v = buf[:, :W].float().reshape(B, T, 3, H, 64)
    return buf, v[:, :, 0], v[:, :, 1], v[:, :, 2]
