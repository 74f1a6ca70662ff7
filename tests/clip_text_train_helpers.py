"""Helpers shared by the GPU tests of include/gg_clip_text_train.h and by tools/make_flash_bwd_parent_golden.py: a raw GgAttnArgs backward call on the buffers of
tests/clip_text_helpers.py, the seeded dout, and the lossless packing of tests/golden/flash_bwd_parent.npz.  A plain module (no tests, no fixtures)."""
import ctypes as C

import numpy as np
import torch

PARENT_CASES = ((2, 80, 2), (3, 50, 3))          # (heads, tokens, batch) of tests/golden/flash_bwd_parent.npz, head dim 64; dtypes 0, 1 and 3


def make_dout(B, T, H, dtype, seed, pad=4):
    """(B*T, H*64 + pad) buffer whose first H*64 columns hold dout."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B * T, H * 64 + pad, generator=g).cuda()
    return buf.to(torch.bfloat16) if dtype == 0 else buf


def attn_bwd(L, qkv, out, lse, dout, B, T, H, dtype, fn="gg_attention_causal_bwd", dqkv=None, D=64, **over):
    """qkv (B*T, ld) as tests/clip_text_helpers.make_qkv lays it out, out (B*T, H*D), lse (B*T, H), dout (B*T, lddo).  dqkv: a NaN-filled buffer shaped like qkv
    unless given (same pitch and offsets).  Returns rc, dqkv."""
    if dqkv is None:
        dqkv = torch.full_like(qkv, float("nan"))
    a = L.AttnArgs()
    a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), qkv.stride(0), 0, H * D, 2 * H * D, D, D
    a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = H, B, T, 0, D ** -0.5
    a.out, a.ldo, a.lse = out.data_ptr(), out.stride(0), lse.data_ptr()
    a.dout, a.lddo, a.dqkv = dout.data_ptr(), dout.stride(0), dqkv.data_ptr()
    for k, v in over.items():
        setattr(a, k, v)
    rc = getattr(L.lib(), fn)(C.byref(a), dtype, L.stream())
    torch.cuda.synchronize()
    return rc, dqkv


def bits(t):
    """The bit pattern of a bf16 / f32 tensor as a numpy uint16 / uint32 array."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy().view(np.uint32)


def pack_parent(b0, b1, b3):
    """dqkv bit patterns of one case in dtype 0 / 1 / 3 -> the stored arrays: dtype 0 and 3 whole, dtype 1 as its XOR with dtype 3 (both are f32 roundings of the
    same values, so the high bits cancel and deflate finds them): lossless, the three together stay below the size limit of a committed file."""
    return dict(d0=b0, d3=b3, d1x3=np.bitwise_xor(b1, b3))


def unpack_parent(z, key):
    return {0: z[f"{key}_d0"], 3: z[f"{key}_d3"], 1: np.bitwise_xor(z[f"{key}_d1x3"], z[f"{key}_d3"])}


def parent_case(L, H, T, B, dtype, fwd="gg_attention_flash_fwd", bwd="gg_attention_flash_bwd"):
    """The seeded non-causal case of flash_bwd_parent.npz: forward for out / lse, then the backward.  Returns the dqkv bit pattern (pad columns dropped)."""
    from tests.clip_text_helpers import causal, make_qkv
    qkv, _, _, _ = make_qkv(B, T, H, dtype, 900 + T)
    rc, out, lse = causal(L, qkv, B, T, H, dtype, qkv.shape[1], fn=fwd)
    assert rc == 0, L.lib().gg_last_error()
    dout = make_dout(B, T, H, dtype, 950 + T)
    rc, dqkv = attn_bwd(L, qkv, out, lse, dout, B, T, H, dtype, fn=bwd)
    assert rc == 0, L.lib().gg_last_error()
    return bits(dqkv[:, :3 * H * 64])
