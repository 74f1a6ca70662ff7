"""Memory discipline of include/gg_attn16b.h, in the way tests/test_gpu_guards_attn16.py holds include/gg_attn16.h: every tensor of the call lives in a
guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and asserts that the
inputs are unchanged, that only -- and all of -- the logical outputs were written, that the two runs agree bit for bit, and that the values match the fp64
gradients.  qkv, out and dout are column slices of wider buffers, dqkv has qkv's pitch and column offset, lse has exactly its capacity, [tokens][heads]."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
CASES = {"test_flash16_backward": ("gg_attention_flash16_bwd",)}
EXEMPT = {
    "gg_attention_flash16_bwd_calls": "query: reads a host counter, no device pointer",
    "gg_clip_set_attention16_train": "switch: sets a host flag, no device pointer (the tower's own buffers are guarded by tests/test_gpu_guards_model.py)",
}


def test_every_attn16b_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_attn16b.h is called by the guard case of this file or is in EXEMPT with its reason -- exactly one of the two."""
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_attn16b.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    assert len(guarded) + len(EXEMPT) == len(declared) == 3


@gpu
@pytest.mark.parametrize("layout", ["clip", "tinyvit"])
@pytest.mark.parametrize("nh,N,nw,pad", [(2, 50, 2, 8), (2, 257, 1, 24), (3, 577, 1, 8)])
def test_flash16_backward(layout, nh, N, nw, pad):
    """gg_attention_flash16_bwd at 50, 257 and 577 tokens.  Reference: fp64 autograd through softmax attention on the bf16-rounded inputs; the kernel is given
    that forward's out rounded to bf16 and its lse in f32.  dq, dk, dv within 1.5e-2 of max |ref| each -- the bf16 tolerance of tests/test_gpu_guards_attn16.py."""
    dt = torch.bfloat16
    tokens, width = nw * N, 3 * nh * 64
    qkv = rnd(tokens, width, seed=47, dtype=dt)
    dout = rnd(tokens, nh * 64, seed=48, dtype=dt)
    if layout == "clip":
        q_off, k_off, v_off, hs = 0, nh * 64, 2 * nh * 64, 64
        split = lambda t: [t.reshape(nw, N, 3, nh, 64)[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
        join = lambda a, b, c: torch.stack([x.permute(0, 2, 1, 3) for x in (a, b, c)], 2).reshape(tokens, width)
    else:
        q_off, k_off, v_off, hs = 0, 64, 128, 192
        split = lambda t: [t.reshape(nw, N, nh, 3, 64)[:, :, :, i].permute(0, 2, 1, 3) for i in range(3)]
        join = lambda a, b, c: torch.stack([x.permute(0, 2, 1, 3) for x in (a, b, c)], 3).reshape(tokens, width)
    q, k, v = (x.double().clone().requires_grad_(True) for x in split(qkv))
    s = q @ k.transpose(-1, -2) * 0.125
    o = torch.softmax(s, -1) @ v
    o.backward(dout.double().reshape(nw, N, nh, 64).permute(0, 2, 1, 3))
    ref = join(q.grad, k.grad, v.grad)
    out_in = o.detach().permute(0, 2, 1, 3).reshape(tokens, nh * 64).to(dt)
    lse_in = torch.logsumexp(s.detach(), -1).permute(0, 2, 1).reshape(tokens, nh).float()
    parts = dict(zip(("dq", "dk", "dv"), split(ref)))

    def call(S, L):
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=width + pad + 8, col_off=8)
        oi = S.inp("out", out_in, ld=nh * 64 + pad + 8, col_off=8)
        di = S.inp("dout", dout.to(dt), ld=nh * 64 + pad + 16, col_off=16)
        li = S.inp("lse", lse_in)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, q_off, k_off, v_off, hs, 64
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = nh, nw, N, 0, 0.125
        dq = S.out("dqkv", tokens, width, dt, ld=width + pad + 8, col_off=8)
        a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = oi.ptr, oi.ld, li.ptr, di.ptr, di.ld, dq.ptr
        L.check(L.lib().gg_attention_flash16_bwd(C.byref(a), 0, L.stream()), "gg_attention_flash16_bwd")

        def check(val):
            got = dict(zip(("dq", "dk", "dv"), split(val["dqkv"].double())))
            for n in got:
                e = float((got[n] - parts[n]).abs().max()) / float(parts[n].abs().max())
                print(f"[guards flash16 bwd {layout} N={N}] {n} {e:.2e}")
                assert e <= 1.5e-2, (n, e)
        return {"dqkv": dq}, check
    run_guarded(call)
