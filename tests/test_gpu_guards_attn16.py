"""Memory discipline of include/gg_attn16.h, in the way tests/test_gpu_guards.py holds include/gg.h: every tensor of the call lives in a guarded
buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and asserts that the input
is unchanged, that only -- and all of -- the logical outputs were written, that the two runs agree bit for bit, and that the values match an fp64 reference.
lse has exactly its capacity, [tokens][heads]."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
CASES = {"test_flash16_forward": ("gg_attention_flash16_fwd",)}
EXEMPT = {
    "gg_attention_flash16_calls": "query: reads a host counter, no device pointer",
    "gg_clip_set_attention16": "switch: sets a host flag, no device pointer (the tower's own buffers are guarded by tests/test_gpu_guards_model.py)",
}


def test_every_attn16_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_attn16.h is called by the guard case of this file or is in EXEMPT with its reason -- exactly one of the two."""
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_attn16.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    assert len(guarded) + len(EXEMPT) == len(declared) == 3


@gpu
@pytest.mark.parametrize("storage", ["f16", "bf16"])
@pytest.mark.parametrize("layout", ["clip", "tinyvit"])
@pytest.mark.parametrize("nh,N,nw,pad", [(2, 50, 2, 8), (2, 257, 1, 24), (3, 577, 1, 8)])
def test_flash16_forward(storage, layout, nh, N, nw, pad):
    """gg_attention_flash16_fwd at 50, 257 and 577 tokens: qkv is a column slice of a wider buffer, out has padded rows, lse is exactly [tokens][heads].
    Reference: fp64 softmax attention on the storage-rounded inputs; out within 1.5e-2 (bf16) / 2e-3 (fp16) of max |ref| -- several units of the output's last
    place, the tolerance of tests/test_gpu_guards_text.py for bf16 and the ratio of the two significands for fp16 -- and lse within 1e-5."""
    dt = torch.float16 if storage == "f16" else torch.bfloat16
    tokens, width = nw * N, 3 * nh * 64
    qkv = rnd(tokens, width, seed=43, dtype=dt)
    if layout == "clip":
        q_off, k_off, v_off, hs = 0, nh * 64, 2 * nh * 64, 64
        v5 = qkv.reshape(nw, N, 3, nh, 64)
        q, k, v = (v5[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    else:
        q_off, k_off, v_off, hs = 0, 64, 128, 192
        v5 = qkv.reshape(nw, N, nh, 3, 64)
        q, k, v = (v5[:, :, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125
    ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(tokens, nh * 64)
    lse_ref = torch.logsumexp(s, -1).permute(0, 2, 1).reshape(tokens, nh)

    def call(S, L):
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=width + pad + 8, col_off=8)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, q_off, k_off, v_off, hs, 64
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = nh, nw, N, 0, 0.125
        out, lse = S.out("out", tokens, nh * 64, dt, ld=nh * 64 + pad), S.out("lse", tokens, nh, torch.float32)
        a.out, a.ldo, a.lse = out.ptr, out.ld, lse.ptr
        L.check(L.lib().gg_attention_flash16_fwd(C.byref(a), 2 if storage == "f16" else 0, L.stream()), "gg_attention_flash16_fwd")

        def check(val):
            tol = 2e-3 if storage == "f16" else 1.5e-2
            assert float((val["out"].double() - ref).abs().max()) <= tol * float(ref.abs().max())
            assert float((val["lse"].double() - lse_ref).abs().max()) <= 1e-5 * float(lse_ref.abs().max())
        return {"out": out, "lse": lse}, check
    run_guarded(call)
