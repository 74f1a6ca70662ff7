"""Memory discipline of the second header (include/gg_clip_text.h), in the way tests/test_gpu_guards.py holds include/gg.h: every tensor of every call lives
in a guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and asserts
that inputs are unchanged, that only -- and all of -- the logical outputs were written, that the two runs agree bit for bit, and that the values match the
reference of the parity test.  Scratch buffers have exactly the size of their capacity function.  The text forward additionally runs from a zero-filled
workspace and weight cache: same bits as from the NaN-filled ones.

CASES is the registry; test_every_text_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import guards as G
from tests.test_gpu_guards import close, rnd, run_guarded

gpu = pytest.mark.gpu
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
CASES = {}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


_QUERY = "query: host arithmetic on the configuration, no device pointer"
_CAP = "capacity function: host arithmetic; its ANSWER sizes the scratch of a guard case exactly, which is how it is tested"
EXEMPT = {
    **{n: _QUERY for n in ("gg_clip_text_num_tensors", "gg_clip_text_tensor_info", "gg_clip_text_param_floats")},
    **{n: _CAP for n in ("gg_clip_text_wcache_bytes", "gg_clip_text_workspace_bytes", "gg_clip_contrastive_scratch_floats", "gg_grad_sq_norm_scratch_doubles")},
}


def _declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_clip_text.h")).read(), flags=re.S)
    return set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))


def test_every_text_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_clip_text.h is called by a guard case of this file or is in EXEMPT with its reason -- exactly one of the two; and a case
    really calls what it registers."""
    from tests.test_guards_cpu import _coverage_gaps
    declared = _declared()
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing, f"entry points of include/gg_clip_text.h with neither a guard test nor an exemption: {missing}"
    assert not unknown, f"registry / exemption names the header does not declare: {unknown}"
    assert not both, f"both guarded and exempt: {both}"
    assert all(any(k in n for k in ("_floats", "_doubles", "_bytes", "_info", "_num_")) for n in EXEMPT)
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    for victim in ("gg_clip_contrastive", "gg_row_scatter_f32", "gg_clip_text_forward"):
        assert _coverage_gaps(declared, guarded - {victim}, EXEMPT)[0] == [victim]
    assert len(guarded) == 7 and len(guarded) + len(EXEMPT) == len(declared) == 14


# ------------------------------------------------------------------------------------------- causal attention
# (heads, tokens, sequences, pad): one token; a ragged single tile; exactly one tile; one key past it; the longest sequence at 12 heads
CAUSAL_SHAPES = [(2, 1, 2, 8), (2, 17, 2, 24), (1, 64, 3, 8), (2, 65, 1, 8), (12, 77, 1, 24)]


@case("gg_attention_causal_fwd")
@gpu
@pytest.mark.parametrize("dtype", [0, 1, 3])
@pytest.mark.parametrize("nh,N,nw,pad", CAUSAL_SHAPES)
def test_causal_attention(dtype, nh, N, nw, pad):
    """gg_attention_causal_fwd; qkv is a column slice of a wider buffer, out has padded rows, lse is exactly [tokens][heads].  Reference: fp64; tolerances of
    tests/test_gpu_clip_text.py (f32 storage 1e-5 of max|ref|; bf16 1.5e-2, its lse 1e-5)."""
    from tests.clip_text_helpers import attn_ref
    dt = BF if dtype == 0 else F32
    tokens, width = nw * N, 3 * nh * 64
    qkv = rnd(tokens, width, seed=41, dtype=dt)
    v = qkv.reshape(nw, N, 3, nh, 64)
    ref, lse_ref = attn_ref(v[:, :, 0], v[:, :, 1], v[:, :, 2])

    def call(S, L):
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=width + pad + 8, col_off=8)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, 0, nh * 64, 2 * nh * 64, 64, 64
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = nh, nw, N, 0, 0.125
        out, lse = S.out("out", tokens, nh * 64, dt, ld=nh * 64 + pad), S.out("lse", tokens, nh, F32)
        a.out, a.ldo, a.lse = out.ptr, out.ld, lse.ptr
        L.check(L.lib().gg_attention_causal_fwd(C.byref(a), dtype, L.stream()), "gg_attention_causal_fwd")

        def check(val):
            tol = 1.5e-2 if dtype == 0 else 1e-5
            assert float((val["out"].double() - ref).abs().max()) <= tol * float(ref.abs().max())
            assert float((val["lse"].double() - lse_ref).abs().max()) <= 1e-5 * float(lse_ref.abs().max())
        return {"out": out, "lse": lse}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- row gather / scatter
@case("gg_row_gather_f32", "gg_row_scatter_f32")
@gpu
@pytest.mark.parametrize("B,T,Cc,with_pos", [(1, 1, 8, True), (5, 9, 128, True), (3, 50, 772, False), (4, 77, 768, True)])
def test_row_gather_and_scatter(B, T, Cc, with_pos):
    """pooled[b] = x[b, pos[b]] and its backward, which writes EVERY element of dx (zeros but for the picked rows); pos NULL = row 0."""
    x, dp = rnd(B * T, Cc, seed=51), rnd(B, Cc, seed=52)
    pos = torch.randint(0, T, (B,), generator=torch.Generator().manual_seed(53)).to(I32)
    pick = pos.long() if with_pos else torch.zeros(B, dtype=torch.long)

    def call(S, L):
        xi, di = S.inp("x", x), S.inp("dpooled", dp)
        pi = S.inp("pos", pos) if with_pos else None
        po, dx = S.out("pooled", B, Cc, F32), S.out("dx", B * T, Cc, F32)
        L.check(L.lib().gg_row_gather_f32(xi.ptr, pi.ptr if pi else None, po.ptr, B, T, Cc, L.stream()), "gg_row_gather_f32")
        L.check(L.lib().gg_row_scatter_f32(di.ptr, pi.ptr if pi else None, dx.ptr, B, T, Cc, L.stream()), "gg_row_scatter_f32")

        def check(val):
            assert torch.equal(val["pooled"], x.reshape(B, T, Cc)[torch.arange(B), pick])
            want = torch.zeros(B, T, Cc)
            want[torch.arange(B), pick] = dp
            assert torch.equal(val["dx"], want.reshape(B * T, Cc))
        return {"pooled": po, "dx": dx}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- contrastive head
def _contrastive_ref(img, txt, ls, g):
    img, txt = img.double().clone().requires_grad_(), txt.double().clone().requires_grad_()
    lsv = torch.tensor(float(ls), dtype=F64, requires_grad=True)
    i_n, t_n = img / img.norm(dim=-1, keepdim=True), txt / txt.norm(dim=-1, keepdim=True)
    lpt = lsv.exp() * t_n @ i_n.t()
    r = dict(lpt=lpt.detach(), i_n=i_n.detach(), t_n=t_n.detach())
    if img.shape[0] == txt.shape[0]:
        tgt = torch.arange(img.shape[0])
        loss = (torch.nn.functional.cross_entropy(lpt, tgt) + torch.nn.functional.cross_entropy(lpt.t(), tgt)) / 2
        (loss * g).backward()
        r.update(loss=loss.detach(), d_img=img.grad, d_txt=txt.grad, d_ls=lsv.grad)
    return r


# (Bi, Bt, P, want_loss): batches that are no multiple of 4 (the contraction padding of the gradient products), one pair, the real projection width, rectangular forwards
@case("gg_clip_contrastive")
@gpu
@pytest.mark.parametrize("Bi,Bt,P,want_loss", [(1, 1, 64, 1), (5, 5, 64, 1), (66, 66, 768, 1), (257, 257, 64, 1), (1, 7, 64, 0), (3, 1, 68, 0), (6, 6, 64, 0)])
def test_contrastive(Bi, Bt, P, want_loss):
    """gg_clip_contrastive with img / txt as column slices of wider buffers and scratch of exactly gg_clip_contrastive_scratch_floats: the K-padding columns of
    the matrices it keeps there are its own to zero.  Tolerances of test_contrastive_head_against_fp64 (loss rel 1e-5, gradients rel-L2 1e-5)."""
    img, txt, ls, g = rnd(Bi, P, seed=61, scale=3.0), rnd(Bt, P, seed=62, scale=0.5), 2.6592, 0.5
    ref = _contrastive_ref(img, txt, ls, g)

    def call(S, L):
        a = L.ContrastiveArgs()
        ii, ti, li = S.inp("img", img, ld=P + 12, col_off=4), S.inp("txt", txt, ld=P + 8, col_off=8), S.inp("logit_scale", torch.tensor([ls]))
        a.img, a.ldi, a.txt, a.ldt, a.Bi, a.Bt, a.P, a.logit_scale = ii.ptr, ii.ld, ti.ptr, ti.ld, Bi, Bt, P, li.ptr
        outs = {"img_n": S.out("img_n", Bi, P, F32), "txt_n": S.out("txt_n", Bt, P, F32), "logits_per_text": S.out("logits_per_text", Bt, Bi, F32),
                "logits_per_image": S.out("logits_per_image", Bi, Bt, F32)}
        a.img_n, a.txt_n, a.logits_per_text, a.logits_per_image = (outs[k].ptr for k in ("img_n", "txt_n", "logits_per_text", "logits_per_image"))
        a.want_loss, a.d_loss_scale = want_loss, g
        if want_loss:
            outs.update(loss=S.out("loss", 1, 1, F32), d_logit_scale=S.out("d_logit_scale", 1, 1, F32), d_img=S.out("d_img", Bi, P, F32), d_txt=S.out("d_txt", Bt, P, F32))
            a.loss, a.d_logit_scale, a.d_img, a.d_txt = (outs[k].ptr for k in ("loss", "d_logit_scale", "d_img", "d_txt"))
        a.scratch = S.scratch("scratch", 4 * L.lib().gg_clip_contrastive_scratch_floats(Bi, Bt, P), row_bytes=4 * max(P, Bi, Bt)).ptr
        L.check(L.lib().gg_clip_contrastive(C.byref(a), L.stream()), "gg_clip_contrastive")

        def check(val):
            rl2 = lambda x, y: float((x.double().flatten() - y.flatten()).norm() / y.norm())
            assert rl2(val["logits_per_text"], ref["lpt"]) < 1e-5 and torch.equal(val["logits_per_image"], val["logits_per_text"].t())
            assert rl2(val["img_n"], ref["i_n"]) < 1e-6 and rl2(val["txt_n"], ref["t_n"]) < 1e-6
            if not want_loss:
                return
            if Bi == 1:
                assert abs(float(val["loss"])) < 1e-6 and float(val["d_img"].abs().max()) < 1e-6 and float(val["d_txt"].abs().max()) < 1e-6
                return
            assert abs(float(val["loss"]) - float(ref["loss"])) < 1e-5 * float(ref["loss"])
            assert rl2(val["d_img"], ref["d_img"]) < 1e-5 and rl2(val["d_txt"], ref["d_txt"]) < 1e-5
        return outs, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- gradient norm
@case("gg_grad_sq_norm")
@gpu
@pytest.mark.parametrize("n,accumulate", [(1, 0), (1000, 1), (4097, 0), (4096 * 1024 + 5, 1)])
def test_grad_sq_norm(n, accumulate):
    """Sum of squares of n floats (an unaligned start included) with scratch of exactly gg_grad_sq_norm_scratch_doubles(n) doubles; out is written, or
    (accumulate) added to."""
    gr = rnd(1, n, seed=71)

    def call(S, L):
        gi = S.inp("g", gr, misalign=4)
        scr = S.scratch("scratch", 8 * L.lib().gg_grad_sq_norm_scratch_doubles(n), row_bytes=8)
        out = S.out("out", 1, 1, F64, init=torch.tensor([[2.5]], dtype=F64) if accumulate else None)
        L.check(L.lib().gg_grad_sq_norm(gi.ptr, n, scr.ptr, out.ptr, accumulate, L.stream()), "gg_grad_sq_norm")

        def check(val):
            want = float((gr.double() ** 2).sum()) + (2.5 if accumulate else 0.0)
            assert abs(float(val["out"]) - want) <= 1e-12 * want
        return {"out": out}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- text tower
@case("gg_clip_text_refresh_weights", "gg_clip_text_forward")
@gpu
@pytest.mark.parametrize("act_dtype", [1, 3, 0])
def test_text_tower_forward(act_dtype):
    """gg_clip_text_refresh_weights + gg_clip_text_forward on the fixture's weights.  The parameter buffer has exactly gg_clip_text_param_floats floats with the fill
    between its tensors; weight cache and workspace have exactly their capacity functions' sizes and start as the fill -- and, a third run, as zeros: last_hidden
    and pooled are the same bits in all three.  The forward leaves parameters, weight cache, ids and positions unchanged."""
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
    ids, eos = torch.from_numpy(z["input_ids"]).to(I32), torch.from_numpy(z["eos_pos"]).to(I32)
    B, Tn = ids.shape
    got = {}
    for fill in ("nan", "finite", "zero"):
        S = G.GuardSet("nan" if fill == "zero" else fill)
        pad = {"nan": float("nan"), "finite": 51015.28, "zero": float("nan")}[fill]
        flat = torch.full((nfl,), pad)
        for n, o, ne in table:
            flat[o:o + ne] = sd["text_model." + n].flatten()
        pi, ii, ei = S.inp("params", flat), S.inp("input_ids", ids), S.inp("eos_pos", eos)
        wc = S.scratch("wcache", lib.gg_clip_text_wcache_bytes(C.byref(cfg)), row_bytes=4 * 256, zero=fill == "zero")
        ws = S.scratch("workspace", lib.gg_clip_text_workspace_bytes(C.byref(cfg), B, Tn), row_bytes=4 * 384, zero=fill == "zero")
        last, pooled = S.out("last_hidden", B * Tn, 128, F32), S.out("pooled", B, 128, F32)
        L.check(lib.gg_clip_text_refresh_weights(C.byref(cfg), pi.ptr, wc.ptr, L.stream()), "gg_clip_text_refresh_weights")
        torch.cuda.synchronize()
        wc_before = wc.buf.clone()
        L.check(lib.gg_clip_text_forward(C.byref(cfg), B, Tn, pi.ptr, wc.ptr, ii.ptr, ei.ptr, ws.ptr, last.ptr, pooled.ptr, L.stream()), "gg_clip_text_forward")
        S.check()
        assert torch.equal(wc.buf, wc_before), "the forward wrote into the weight cache"
        got[fill] = (last.view.clone(), pooled.view.clone())
    for other in ("finite", "zero"):
        G.assert_bit_identical(got["nan"][0], got[other][0], f"last_hidden nan vs {other}")
        G.assert_bit_identical(got["nan"][1], got[other][1], f"pooled nan vs {other}")
    pooled = got["nan"][1].cpu().double()
    want = torch.from_numpy(z["text_pooled"]).double()
    assert float((pooled - want).norm() / want.norm()) < (2e-2 if act_dtype == 0 else 1e-4)
