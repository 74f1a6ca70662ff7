"""Memory discipline of the third header (include/gg_clip_text_train.h), in the way tests/test_gpu_guards_text.py holds the second: every tensor of every call
lives in a guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and
asserts that inputs are unchanged, that only -- and all of -- the logical outputs were written, that the two runs agree bit for bit, and that the values match
the reference of the parity test.  Scratch buffers have exactly the size of their capacity function.  The tower's training step additionally runs from a
zero-filled workspace: same bits as from the NaN-filled one.

CASES is the registry; test_every_text_train_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import guards as G
from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
CASES = {}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


_QUERY = "query: host arithmetic on the configuration and the mask, no device pointer"
_CAP = "capacity function: host arithmetic; its ANSWER sizes the scratch of a guard case exactly, which is how it is tested"
EXEMPT = {
    "gg_clip_text_first_trained_layer": _QUERY,
    "gg_clip_text_train_workspace_bytes": _CAP,
    "gg_embedding_scatter_add_scratch_bytes": _CAP,
}


def _declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_clip_text_train.h")).read(), flags=re.S)
    return set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))


def test_every_text_train_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_clip_text_train.h is called by a guard case of this file or is in EXEMPT with its reason -- exactly one of the two; and a
    case really calls what it registers."""
    from tests.test_guards_cpu import _coverage_gaps
    declared = _declared()
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing, f"entry points of include/gg_clip_text_train.h with neither a guard test nor an exemption: {missing}"
    assert not unknown, f"registry / exemption names the header does not declare: {unknown}"
    assert not both, f"both guarded and exempt: {both}"
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    for victim in ("gg_attention_causal_bwd", "gg_embedding_scatter_add_f32", "gg_clip_text_backward"):
        assert _coverage_gaps(declared, guarded - {victim}, EXEMPT)[0] == [victim]
    assert len(guarded) == 4 and len(guarded) + len(EXEMPT) == len(declared) == 7


# ------------------------------------------------------------------------------------------- causal attention backward
# (heads, tokens, sequences, pad): one token; a ragged single tile; exactly one tile; one key past it; the longest sequence at 12 heads
CAUSAL_SHAPES = [(2, 1, 2, 8), (2, 17, 2, 24), (1, 64, 3, 8), (2, 65, 1, 8), (12, 77, 1, 24)]


@case("gg_attention_causal_bwd")
@gpu
@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("nh,N,nw,pad", CAUSAL_SHAPES)
def test_causal_attention_backward(dtype, nh, N, nw, pad):
    """gg_attention_causal_bwd; qkv and dqkv are column slices of wider buffers with padded rows (same pitch and offsets), out and dout have padded rows, lse is
    exactly [tokens][heads].  out / lse: the fp64 reference's (rounded to the storage type).  Reference: fp64 autograd; tolerances of
    tests/test_gpu_clip_text_train.py (f32 storage 2e-5 of max|ref|, bf16 1.5e-2)."""
    from tests.clip_text_helpers import attn_ref
    dt = BF if dtype == 0 else F32
    tokens, width = nw * N, 3 * nh * 64
    qkv = rnd(tokens, width, seed=41, dtype=dt)
    dout = rnd(tokens, nh * 64, seed=42, dtype=dt)
    v = qkv.reshape(nw, N, 3, nh, 64)
    q, k, vv = (v[:, :, i].double().clone().requires_grad_() for i in range(3))
    ro, rl = attn_ref(q, k, vv)
    ro.backward(dout.double())
    ref = torch.stack([q.grad, k.grad, vv.grad], 2).reshape(tokens, width)
    out_in, lse_in = ro.detach().to(dt).float(), rl.detach().float()

    def call(S, L):
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=width + pad + 8, col_off=8)
        oi, li = S.inp("out", out_in.to(dt), ld=nh * 64 + pad), S.inp("lse", lse_in)
        di = S.inp("dout", dout.to(dt), ld=nh * 64 + 8)
        dq = S.out("dqkv", tokens, width, dt, ld=width + pad + 8, col_off=8)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, 0, nh * 64, 2 * nh * 64, 64, 64
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = nh, nw, N, 0, 0.125
        a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = oi.ptr, oi.ld, li.ptr, di.ptr, di.ld, dq.ptr
        L.check(L.lib().gg_attention_causal_bwd(C.byref(a), dtype, L.stream()), "gg_attention_causal_bwd")

        def check(val):
            # (bf16: out was rounded to storage before delta = sum dO O was formed from it, as in the tower; the gate is the bf16 storage gate)
            assert float((val["dqkv"].double() - ref).abs().max()) <= (1.5e-2 if dtype == 0 else 2e-5) * float(ref.abs().max())
        return {"dqkv": dq}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- embedding scatter-add
@case("gg_embedding_scatter_add_f32")
@gpu
@pytest.mark.parametrize("rows,D,vocab", [(1, 128, 64), (45, 128, 64), (7392, 768, 1000)])
def test_embedding_scatter_add(rows, D, vocab):
    """gg_embedding_scatter_add_f32 with scratch of exactly gg_embedding_scatter_add_scratch_bytes(rows); dtable is ACCUMULATED into (it starts from known values),
    so `written` does not apply: the rows of ids that occur must change, the others keep their bits."""
    dx = rnd(rows, D, seed=81)
    ids = torch.randint(0, vocab, (rows,), generator=torch.Generator().manual_seed(82)).to(I32)
    ids[0], ids[-1] = 0, vocab - 1
    pre = rnd(vocab, D, seed=83)
    ref = pre.double().index_add_(0, ids.long(), dx.double())

    def call(S, L):
        xi, ii = S.inp("dx", dx), S.inp("ids", ids)
        tab = S.out("dtable", vocab, D, F32, init=pre, written=False)
        scr = S.scratch("scratch", L.lib().gg_embedding_scatter_add_scratch_bytes(rows), row_bytes=8)
        L.check(L.lib().gg_embedding_scatter_add_f32(xi.ptr, ii.ptr, tab.ptr, rows, D, vocab, scr.ptr, L.stream()), "gg_embedding_scatter_add_f32")

        def check(val):
            assert float((val["dtable"].double() - ref).abs().max()) < 1e-6 * float(ref.abs().max())
            hit = torch.zeros(vocab, dtype=torch.bool)
            hit[ids.long()] = True
            assert torch.equal(val["dtable"][~hit], pre[~hit]) or bool(hit.all())
        return {"dtable": tab}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- text tower, training forward + backward
def _text_top(n):
    return n.startswith("encoder.layers.1.") or n.startswith("final_layer_norm")


@case("gg_clip_text_forward_train", "gg_clip_text_backward")
@gpu
@pytest.mark.parametrize("mask_name", ["null", "text_top", "zero"])
@pytest.mark.parametrize("act_dtype", [1, 3, 0])
def test_text_tower_training_step(act_dtype, mask_name):
    """gg_clip_text_forward_train + gg_clip_text_backward on the fixture's weights, 5 x 9 ids, masks NULL / text_top / all-zero.  The parameter buffer has exactly
    gg_clip_text_param_floats floats with the fill between its tensors; the workspace has exactly gg_clip_text_train_workspace_bytes bytes and starts as the fill
    -- and, a third run, as zeros; the flat gradient buffer starts as zeros (it is accumulated into).  last_hidden, pooled and every gradient are the same bits in
    all three runs; frozen tensors' ranges of the gradient buffer (and the fill between tensors) are never written; the all-zero mask's backward touches nothing."""
    from geoguessr_ai_amd import _lib as L
    from tests import clip_text_golden as T
    L.require_gpu()
    lib, z, sd = L.lib(), T.load(), T.decode_state_dict()
    cfg = L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, act_dtype)
    nfl = lib.gg_clip_text_param_floats(C.byref(cfg))
    name, off, numel = C.create_string_buffer(256), C.c_int64(), C.c_int64()
    table = []
    for i in range(lib.gg_clip_text_num_tensors(C.byref(cfg))):
        L.check(lib.gg_clip_text_tensor_info(C.byref(cfg), i, name, 256, C.byref(off), C.byref(numel), None, None), "gg_clip_text_tensor_info")
        table.append((name.value.decode(), off.value, numel.value))
    mask = None if mask_name == "null" else bytes(int(mask_name == "text_top" and _text_top(n)) for n, _, _ in table)
    on = [mask is None or bool(mask[i]) for i in range(len(table))]
    ids, eos = torch.from_numpy(z["input_ids"]).to(I32), torch.from_numpy(z["eos_pos"]).to(I32)
    B, Tn = ids.shape
    dpool, dlast = rnd(B, 128, seed=91), rnd(B * Tn, 128, seed=92, scale=0.1)
    got = {}
    for fill in ("nan", "finite", "zero"):
        S = G.GuardSet("nan" if fill == "zero" else fill)
        pad = {"nan": float("nan"), "finite": 51015.28, "zero": float("nan")}[fill]
        flat = torch.full((nfl,), pad)
        for n, o, ne in table:
            flat[o:o + ne] = sd["text_model." + n].flatten()
        pi, ii, ei = S.inp("params", flat), S.inp("input_ids", ids), S.inp("eos_pos", eos)
        dpi, dli = S.inp("d_pooled", dpool), S.inp("d_last_hidden", dlast)
        wc = S.scratch("wcache", lib.gg_clip_text_wcache_bytes(C.byref(cfg)), row_bytes=4 * 256)
        ws = S.scratch("workspace", lib.gg_clip_text_train_workspace_bytes(C.byref(cfg), B, Tn, mask), row_bytes=4 * 384, zero=fill == "zero")
        last, pooled = S.out("last_hidden", B * Tn, 128, F32), S.out("pooled", B, 128, F32)
        grads = S.out("grads", 1, nfl, F32, init=torch.zeros(1, nfl), written=False)
        L.check(lib.gg_clip_text_refresh_weights(C.byref(cfg), pi.ptr, wc.ptr, L.stream()), "gg_clip_text_refresh_weights")
        torch.cuda.synchronize()
        wc_before = wc.buf.clone()
        L.check(lib.gg_clip_text_forward_train(C.byref(cfg), B, Tn, pi.ptr, wc.ptr, ii.ptr, ei.ptr, ws.ptr, last.ptr, pooled.ptr, mask, L.stream()), "gg_clip_text_forward_train")
        torch.cuda.synchronize()
        ws_mid = ws.buf.clone()
        L.check(lib.gg_clip_text_backward(C.byref(cfg), B, Tn, pi.ptr, wc.ptr, ii.ptr, ei.ptr, ws.ptr, dpi.ptr, dli.ptr, grads.ptr, mask, L.stream()), "gg_clip_text_backward")
        S.check()
        assert torch.equal(wc.buf, wc_before), "the step wrote into the weight cache"
        gv = grads.view.clone().flatten()
        live = torch.zeros(nfl, dtype=torch.bool, device=gv.device)
        for (n, o, ne), t in zip(table, on):
            if t:
                live[o:o + ne] = True
                assert bool(torch.isfinite(gv[o:o + ne]).all()), n
                if not n.endswith("k_proj.bias") and "token_embedding" not in n and "position_embedding" not in n:
                    assert float(gv[o:o + ne].abs().max()) > 0.0, n
        assert not bool((~live).any()) or float(gv[~live].abs().max()) == 0.0, "a frozen range (or the space between tensors) of the gradient buffer was written"
        if mask_name == "zero":
            assert torch.equal(ws.buf, ws_mid), "the all-zero mask's backward touched the workspace"
        got[fill] = (last.view.clone(), pooled.view.clone(), gv)
    for other in ("finite", "zero"):
        for i, what in enumerate(("last_hidden", "pooled", "grads")):
            G.assert_bit_identical(got["nan"][i], got[other][i], f"{what} nan vs {other}")
    pooled = got["nan"][1].cpu().double()
    want = torch.from_numpy(z["text_pooled"]).double()
    assert float((pooled - want).norm() / want.norm()) < (2e-2 if act_dtype == 0 else 1e-4)
