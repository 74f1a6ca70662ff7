"""Memory discipline of include/gg_attn16wb.h, in the way tests/test_gpu_guards_attn16_bwd.py holds include/gg_attn16b.h: every tensor of the call
lives in a guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and
asserts that the inputs -- qkv, out, dout, lse and the bias table -- are read only inside their tensors and unchanged, that dqkv, dbias and EXACTLY
gg_attention_flash16_win_dbias_rows rows of scratch are the only writes, that the two runs agree (dqkv bit for bit; dbias, whose LDS adds land in no fixed order,
to 1e-5 of its magnitude) -- so nothing depends on the guard fill or on what the scratch held before --, and that the values match the fp64 gradients.  qkv, out
and dout are column slices of wider buffers, dqkv has qkv's pitch and column offset, lse has exactly its capacity [tokens][heads], the table and dbias exactly
[heads][ws * ws]."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attention_cases as AC
from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
CASES = {"test_flash16_win_backward": ("gg_attention_flash16_win_bwd",)}
EXEMPT = {
    "gg_attention_flash16_win_bwd_calls": "query: reads a host counter, no device pointer",
    "gg_attention_flash16_win_dbias_rows": "query: arithmetic on its arguments, no device pointer (the guard case sizes its scratch by it)",
    "gg_tinyvit_set_attention16_train": "switch: sets a host flag, no device pointer (the model's own buffers are guarded by tests/test_gpu_guards_model.py)",
}


def test_every_attn16wb_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_attn16wb.h is called by the guard case of this file or is in EXEMPT with its reason -- exactly one of the two."""
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_attn16wb.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    assert len(guarded) + len(EXEMPT) == len(declared) == 4


@gpu
@pytest.mark.parametrize("mode", ["dbias", "bias", "plain"])
@pytest.mark.parametrize("layout,nh,ws,m,nw,pad", [("tinyvit", 2, 5, 2, 4, 8), ("clip", 2, 9, 1, 2, 4), ("tinyvit", 3, 17, 2, 4, 4), ("clip", 2, 32, 1, 1, 8)])
def test_flash16_win_backward(mode, layout, nh, ws, m, nw, pad):
    """gg_attention_flash16_win_bwd at 25, 81, 289 and 1024 tokens (ws 5 and 17 gathered from 2 x 2-window maps), with the bias gradient (a zeroed dbias and a
    scratch of exactly the rows the library asks for), with the table only, and without a table.  Reference: fp64 autograd through softmax attention with the
    f32 table on the bf16-rounded inputs; the kernel is given that forward's out rounded to bf16 and its lse in f32.  dq, dk, dv within 1.5e-2 of max |ref| each
    -- the bf16 tolerance of tests/test_gpu_guards_attn16_bwd.py --, dbias within 1.5e-2 of max |ref| as well (its error is that of out's bf16 rounding inside
    delta, summed over the table entry's pairs)."""
    dt = torch.bfloat16
    N = ws * ws
    tokens, width = nw * N, 3 * nh * 32
    qkv = rnd(tokens, width, seed=47, dtype=dt)
    dout = rnd(tokens, nh * 32, seed=48, dtype=dt)
    table = 0.5 * rnd(nh, N, seed=49)
    idx = AC.token_index("tinyvit", N, nw, ws, m * ws)                      # (windows, N) rows of the map
    q_off, k_off, v_off, hs = AC.columns(layout, nh, 32)
    g = qkv[idx].double()                                                   # (nw, N, width)
    q, k, v = (torch.stack([g[:, :, off + h * hs:off + h * hs + 32] for h in range(nh)], 1).clone().requires_grad_(True) for off in (q_off, k_off, v_off))
    tab = table.double().clone().requires_grad_(True)
    s = q @ k.transpose(-1, -2) * 32 ** -0.5
    if mode != "plain":
        s = s + tab[:, AC.bias_idxs(ws)]
    o = torch.softmax(s, -1) @ v
    o.backward(dout[idx].double().view(nw, N, nh, 32).permute(0, 2, 1, 3))
    unflat = lambda x, cols: torch.zeros(tokens, cols, dtype=torch.float64).index_put_((idx.reshape(-1),), x.reshape(nw * N, cols))
    out_in = unflat(o.detach().permute(0, 2, 1, 3).reshape(nw, N, nh * 32), nh * 32).to(dt)
    lse_in = unflat(torch.logsumexp(s.detach(), -1).permute(0, 2, 1), nh).float()
    cc = dict(idx=idx, heads=nh, hd=32, head_stride=hs, q_off=q_off, k_off=k_off, v_off=v_off)
    parts = dict(dq=q.grad, dk=k.grad, dv=v.grad)

    def call(S, L):
        lib = L.lib()
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=width + pad + 8, col_off=8)
        oi = S.inp("out", out_in, ld=nh * 32 + pad + 8, col_off=8)
        di = S.inp("dout", dout.to(dt), ld=nh * 32 + pad + 16, col_off=16)
        li = S.inp("lse", lse_in)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, q_off, k_off, v_off, hs, 32
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = nh, nw, N, ws, m * ws, m * ws, 32 ** -0.5
        outs = {}
        if mode != "plain":
            a.bias_table = S.inp("bias_table", table).ptr
        if mode == "dbias":
            outs["dbias"] = S.out("dbias", nh, N, torch.float32, init=torch.zeros(nh, N))          # ACCUMULATED into
            a.dbias = outs["dbias"].ptr
            rows = lib.gg_attention_flash16_win_dbias_rows(nw, N)
            a.dbias_scratch = S.scratch("dbias_scratch", rows * nh * N * 4, row_bytes=nh * N * 4).ptr
        dq = outs["dqkv"] = S.out("dqkv", tokens, width, dt, ld=width + pad + 8, col_off=8)
        a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = oi.ptr, oi.ld, li.ptr, di.ptr, di.ld, dq.ptr
        L.check(lib.gg_attention_flash16_win_bwd(C.byref(a), 0, L.stream()), "gg_attention_flash16_win_bwd")

        def check(val):
            got = dict(zip(("dq", "dk", "dv"), AC.canon_dqkv(cc, val["dqkv"])))
            if mode == "dbias":
                got["dbias"], parts["dbias"] = val["dbias"].double(), tab.grad
            for n in got:
                e = float((got[n] - parts[n]).abs().max()) / float(parts[n].abs().max())
                print(f"[guards flash16 win bwd {layout} ws={ws} {mode}] {n} {e:.2e}")
                assert e <= 1.5e-2, (n, e)
        return outs, check
    run_guarded(call, atomic=("dbias",))
