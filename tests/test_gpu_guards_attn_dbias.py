"""Memory discipline of include/gg_attn_dbias.h, in the way tests/test_gpu_guards_attn16_win_bwd.py holds include/gg_attn16wb.h: every tensor of the
call lives in a guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and
asserts that the inputs -- qkv, out, dout, lse and the bias table -- are read only inside their tensors and unchanged, that dbias and EXACTLY
gg_attention_dbias_rows rows of scratch are the only writes, that the two runs agree BIT FOR BIT (the order of the adds is fixed: nothing depends on the guard
fill, on neighbouring columns, on padding rows or on what the scratch held before), and that the values match the fp64 gradient.  qkv, out and dout are column
slices of wider buffers with padded rows, lse has exactly its capacity [tokens][heads], the table and dbias exactly [heads][ws * ws]."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attention_cases as AC
from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
CASES = {"test_attention_dbias": ("gg_attention_dbias",)}
EXEMPT = {
    "gg_attention_dbias_rows": "query: arithmetic on the geometry of its arguments, no device pointer is looked at (the guard case sizes its scratch by it)",
    "gg_attention_dbias_calls": "query: reads a host counter, no device pointer",
    "gg_tinyvit_set_deterministic_dbias": "switch: sets a host flag, no device pointer (the model's own buffers are guarded by tests/test_gpu_guards_model.py)",
}


def test_every_attn_dbias_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_attn_dbias.h is called by the guard case of this file or is in EXEMPT with its reason -- exactly one of the two."""
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_attn_dbias.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    assert len(guarded) + len(EXEMPT) == len(declared) == 4


# (storage dtype code, heads, ws, windows per map side, windows, pad): 25 tokens gathered from 2 x 2-window maps; 600 windows of 9 tokens (more windows than the 512
# window groups: a workgroup walks two windows); 289 tokens (ragged last strip and tile, key rows straddling tiles); 1024 tokens (1024 bins, 16 key tiles)
@gpu
@pytest.mark.parametrize("dtype,nh,ws,m,nw,pad", [(0, 2, 5, 2, 4, 8), (1, 2, 5, 2, 4, 4), (0, 1, 3, 2, 600, 8), (1, 3, 17, 2, 4, 4), (0, 3, 17, 2, 4, 24), (0, 2, 32, 1, 1, 8),
                                                  (3, 2, 32, 1, 1, 4)])
def test_attention_dbias(dtype, nh, ws, m, nw, pad):
    """gg_attention_dbias with a pre-loaded dbias (ACCUMULATED into) and a scratch of exactly the rows the library asks for.  Reference: fp64 autograd through softmax
    attention with the f32 table on the stored inputs; the kernel is given that forward's out rounded to the storage type and its lse in f32.  f32 storage within
    1e-5 of max |ref|; bf16 within 1.5e-2, the bf16 tolerance of tests/test_gpu_guards_attn16_win_bwd.py (out's bf16 rounding inside delta)."""
    dt = torch.bfloat16 if dtype == 0 else torch.float32
    al = 8 if dtype == 0 else 4
    N = ws * ws
    tokens, width = nw * N, 3 * nh * 32
    qkv = rnd(tokens, width, seed=47, dtype=dt)
    dout = rnd(tokens, nh * 32, seed=48, dtype=dt)
    table = 0.5 * rnd(nh, N, seed=49)
    pre = rnd(nh, N, seed=50)
    idx = AC.token_index("tinyvit", N, nw, ws, m * ws)
    q_off, k_off, v_off, hs = AC.columns("tinyvit", nh, 32)
    g = qkv[idx].double()
    q, k, v = (torch.stack([g[:, :, off + h * hs:off + h * hs + 32] for h in range(nh)], 1) for off in (q_off, k_off, v_off))
    tab = table.double().clone().requires_grad_(True)
    s = q @ k.transpose(-1, -2) * 32 ** -0.5 + tab[:, AC.bias_idxs(ws)]
    o = torch.softmax(s, -1) @ v
    o.backward(dout[idx].double().view(nw, N, nh, 32).permute(0, 2, 1, 3))
    unflat = lambda x, cols: torch.zeros(tokens, cols, dtype=torch.float64).index_put_((idx.reshape(-1),), x.reshape(nw * N, cols))
    out_in = unflat(o.detach().permute(0, 2, 1, 3).reshape(nw, N, nh * 32), nh * 32).to(dt)
    lse_in = unflat(torch.logsumexp(s.detach(), -1).permute(0, 2, 1), nh).float()

    def call(S, L):
        lib = L.lib()
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=width + pad + al, col_off=al)
        oi = S.inp("out", out_in, ld=nh * 32 + pad + al, col_off=al)
        di = S.inp("dout", dout.to(dt), ld=nh * 32 + pad + 2 * al, col_off=2 * al)
        li = S.inp("lse", lse_in)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, q_off, k_off, v_off, hs, 32
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = nh, nw, N, ws, m * ws, m * ws, 32 ** -0.5
        a.bias_table = S.inp("bias_table", table).ptr
        a.out, a.ldo, a.lse, a.dout, a.lddo = oi.ptr, oi.ld, li.ptr, di.ptr, di.ld
        rows = lib.gg_attention_dbias_rows(C.byref(a), dtype)
        assert rows == min(nw, 512) + 64
        db = S.out("dbias", nh, N, torch.float32, init=pre.clone())
        a.dbias = db.ptr
        a.dbias_scratch = S.scratch("dbias_scratch", rows * nh * N * 4, row_bytes=nh * N * 4).ptr
        L.check(lib.gg_attention_dbias(C.byref(a), dtype, 0, L.stream()), "gg_attention_dbias")

        def check(val):
            got = val["dbias"].double() - pre.double()
            e = float((got - tab.grad).abs().max()) / float(tab.grad.abs().max())
            tol = 1.5e-2 if dtype == 0 else 1e-5
            print(f"[guards attention_dbias dtype={dtype} ws={ws} windows={nw}] dbias {e:.2e} (tolerance {tol:.1e})")
            assert e <= tol, e
        return {"dbias": db}, check
    run_guarded(call)
