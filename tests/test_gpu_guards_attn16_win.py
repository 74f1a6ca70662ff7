"""Memory discipline of include/gg_attn16w.h, in the way tests/test_gpu_guards_attn16.py holds include/gg_attn16.h: every tensor of the call lives in
a guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and asserts that
the inputs -- qkv and the bias table -- are unchanged, that only -- and all of -- the logical outputs were written, that the two runs agree bit for bit, and that the
values match an fp64 reference.  lse has exactly its capacity, [tokens][heads]; the table exactly [heads][ws * ws]."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attention_cases as AC
from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
CASES = {"test_flash16_win_forward": ("gg_attention_flash16_win_fwd",)}
EXEMPT = {
    "gg_attention_flash16_win_calls": "query: reads a host counter, no device pointer",
    "gg_tinyvit_set_attention16": "switch: sets a host flag, no device pointer (the model's own buffers are guarded by tests/test_gpu_guards_model.py)",
}


def test_every_attn16w_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_attn16w.h is called by the guard case of this file or is in EXEMPT with its reason -- exactly one of the two."""
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_attn16w.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    assert len(guarded) + len(EXEMPT) == len(declared) == 3


@gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("layout", ["tinyvit", "clip"])
@pytest.mark.parametrize("nh,ws,nw,pad", [(2, 9, 8, 8), (3, 17, 4, 4), (2, 17, 4, 24)])
def test_flash16_win_forward(bias, layout, nh, ws, nw, pad):
    """gg_attention_flash16_win_fwd at 81 and 289 tokens, the windows gathered from 2 x 2-window maps: qkv is a column slice of a wider buffer (pad 4: rows 8-byte
    aligned, the two-load form), out has padded rows, lse is exactly [tokens][heads], the table exactly [heads][ws * ws].  Reference: fp64 softmax attention on
    the bf16-rounded inputs with the f32 table; out within 1.5e-2 of max |ref| -- several units of the output's last place, the bf16 tolerance of
    tests/test_gpu_guards_attn16.py -- and lse within 1e-5."""
    dt = torch.bfloat16
    N, m = ws * ws, 2
    tokens, width = nw * N, 3 * nh * 32
    qkv = rnd(tokens, width, seed=47, dtype=dt)
    table = 0.5 * rnd(nh, N, seed=48)
    idx = AC.token_index("tinyvit", N, nw, ws, m * ws)                      # (windows, N) rows of the map
    q_off, k_off, v_off, hs = AC.columns(layout, nh, 32)
    g = qkv[idx].double()                                                   # (nw, N, width)
    q, k, v = (torch.stack([g[:, :, off + h * hs:off + h * hs + 32] for h in range(nh)], 1) for off in (q_off, k_off, v_off))
    s = q @ k.transpose(-1, -2) * 32 ** -0.5
    if bias:
        s = s + table.double()[:, AC.bias_idxs(ws)]
    ref = torch.zeros(tokens, nh * 32, dtype=torch.float64)
    ref[idx] = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(nw, N, nh * 32)
    lse_ref = torch.zeros(tokens, nh, dtype=torch.float64)
    lse_ref[idx] = torch.logsumexp(s, -1).permute(0, 2, 1)

    def call(S, L):
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=width + pad + 8, col_off=8)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, q_off, k_off, v_off, hs, 32
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = nh, nw, N, ws, m * ws, m * ws, 32 ** -0.5
        if bias:
            a.bias_table = S.inp("bias_table", table).ptr
        out, lse = S.out("out", tokens, nh * 32, dt, ld=nh * 32 + pad), S.out("lse", tokens, nh, torch.float32)
        a.out, a.ldo, a.lse = out.ptr, out.ld, lse.ptr
        L.check(L.lib().gg_attention_flash16_win_fwd(C.byref(a), 0, L.stream()), "gg_attention_flash16_win_fwd")

        def check(val):
            assert float((val["out"].double() - ref).abs().max()) <= 1.5e-2 * float(ref.abs().max())
            assert float((val["lse"].double() - lse_ref).abs().max()) <= 1e-5 * float(lse_ref.abs().max())
        return {"out": out, "lse": lse}, check
    run_guarded(call)
