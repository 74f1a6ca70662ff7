"""GPU tests of the contrastive pre-training stage (include/gg_clip_text.h, pretrain/clip_model.py): causal attention against fp64 torch, exact causality, the
text tower and the whole training step against transformers' CLIPModel (tests/golden/clip_text_tiny.npz), the contrastive head against fp64, three AdamW steps
with gradient clipping, the refusals, and the fp32_split routing at the real B/32 and L/14-336 text dimensions.  Everything runs through libgg.so."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import clip_text_golden as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / b.norm())


from tests.clip_text_helpers import attn_ref, causal, make_qkv          # noqa: E402


@pytest.mark.parametrize("H", [2, 12])
def test_causal_attention_against_fp64(L, H):
    """dtype 1 / 3: out and lse within 1e-5 of max|ref| (the gate of test_split_attention_against_fp64), identical bits between the two; dtype 0: the bounds of the
    bf16 flash forward test (test_flash_attention_forward_backward in tests/test_gpu_precision.py: 1.5e-2, the bf16 storage of the result); its lse is f32 arithmetic
    on the bf16-exact inputs the reference also sees, so it keeps the f32 gate."""
    B = 3
    for T in (1, 7, 16, 17, 63, 64, 65, 77):
        for dtype in (1, 0):
            buf, q, k, v = make_qkv(B, T, H, dtype, 100 + T)
            ro, rl = attn_ref(q, k, v)
            rc, out, lse = causal(L, buf, B, T, H, dtype, buf.shape[1])
            assert rc == 0, L.lib().gg_last_error()
            eo = float((out.double() - ro).abs().max() / ro.abs().max())
            el = float((lse.double() - rl).abs().max() / rl.abs().max())
            print(f"causal attention H={H} T={T} dtype={dtype}: out {eo:.2e} lse {el:.2e} of max|ref|")
            if dtype == 1:
                assert eo < 1e-5 and el < 1e-5, (T, eo, el)
                rc3, out3, lse3 = causal(L, buf, B, T, H, 3, buf.shape[1])
                assert rc3 == 0 and torch.equal(out3, out) and torch.equal(lse3, lse)
                rcn, outn, _ = causal(L, buf, B, T, H, 1, buf.shape[1], want_lse=False)          # lse is optional
                assert rcn == 0 and torch.equal(outn, out)
            else:
                assert eo < 1.5e-2 and el < 1e-5, (T, eo, el)


@pytest.mark.parametrize("dtype", [1, 0])
def test_causality_is_exact(L, dtype):
    B, T, H = 2, 77, 2
    buf, q, k, v = make_qkv(B, T, H, dtype, 7)
    _, out, lse = causal(L, buf, B, T, H, dtype, buf.shape[1])
    g = torch.Generator().manual_seed(8)
    for p in (0, 15, 16, 63, 64):
        b2 = buf.clone().reshape(B, T, -1)
        b2[:, p + 1:] = (torch.randn(B, T - p - 1, b2.shape[2], generator=g) * 3).to(b2.dtype).cuda()
        _, out2, lse2 = causal(L, b2.reshape(B * T, -1), B, T, H, dtype, buf.shape[1])
        o1, o2 = out.reshape(B, T, -1), out2.reshape(B, T, -1)
        assert torch.equal(o1[:, :p + 1], o2[:, :p + 1]) and torch.equal(lse.reshape(B, T, H)[:, :p + 1], lse2.reshape(B, T, H)[:, :p + 1]), p
        assert not torch.equal(o1[:, p + 1:], o2[:, p + 1:])
    # a row-0 query returns v[0]
    v0 = v[:, 0].reshape(B, H * 64)
    got = out.reshape(B, T, -1)[:, 0].float()
    assert float((got - v0).abs().max()) <= (2.0 ** -7 if dtype == 0 else 2.0 ** -22) * float(v0.abs().max())


def test_noncausal_flash_forward_bits_unchanged(L):
    """gg_attention_flash_fwd, dtype 3 and dtype 0, 50 and 65 tokens: the bits of the build before the causal template parameter was added (arrays written by
    tools/make_flash_parent_golden.py run against that build's libgg.so; tests/golden/flash_fwd_parent.npz)."""
    z = np.load(os.path.join(HERE, "golden", "flash_fwd_parent.npz"))
    for T in (50, 65):
        for dtype in (3, 0):
            buf, _, _, _ = make_qkv(2, T, 2, dtype, 500 + T)
            rc, out, lse = causal(L, buf, 2, T, 2, dtype, buf.shape[1], fn="gg_attention_flash_fwd")
            assert rc == 0
            assert np.array_equal(out.float().cpu().numpy(), z[f"out_{T}_{dtype}"]) and np.array_equal(lse.cpu().numpy(), z[f"lse_{T}_{dtype}"]), (T, dtype)


def test_causal_attention_refusals_touch_nothing(L):
    buf, _, _, _ = make_qkv(1, 16, 2, 1, 3)
    bias = torch.zeros(16, device="cuda")
    cases = [dict(head_dim=32), dict(window_size=4, map_h=4, map_w=4), dict(bias_table=bias.data_ptr()), dict(bias=bias.data_ptr())]
    for over in cases:
        rc, out, lse = causal(L, buf, 1, 16, 2, 1, buf.shape[1], **over)
        assert rc != 0 and bool(torch.isnan(out).all()) and bool(torch.isnan(lse).all()), over
    rc, out, _ = causal(L, buf, 1, 16, 2, 2, buf.shape[1])
    assert rc != 0 and b"dtype" in L.lib().gg_last_error() and bool(torch.isnan(out).all())
    big, _, _, _ = make_qkv(1, 78, 2, 1, 4)
    rc, out, _ = causal(L, big, 1, 78, 2, 1, big.shape[1])
    assert rc != 0 and b"position" in L.lib().gg_last_error() and bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ model against the fixture
def tiny_model(precision, eos=63, **kw):
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel
    m = CLIPModel(config=G.tiny_config(eos), precision=precision, **kw)
    m.load_hf_state_dict(G.decode_state_dict())
    return m.cuda()


def inputs():
    z = G.load()
    return z, torch.from_numpy(z["input_ids"]).cuda(), torch.from_numpy(z["pixel_values"]).cuda()


@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
def test_text_tower_against_the_fixture(L, precision):
    z, ids, _ = inputs()
    m = tiny_model(precision)
    pooled, last = m.text_model.forward_hip(ids, None, True)
    te = m.get_text_features(input_ids=ids)
    te = te / te.norm(dim=-1, keepdim=True)
    eos = z["eos_pos"]
    rows = torch.cat([last[b, :eos[b] + 1] for b in range(5)])
    want = np.concatenate([z["text_last_hidden"][b, :eos[b] + 1] for b in range(5)])
    e = (rel_l2(rows, want), rel_l2(pooled, z["text_pooled"]), rel_l2(te, z["text_embeds"]))
    print(f"text tower [{precision}]: rel-L2 last_hidden {e[0]:.2e} pooled {e[1]:.2e} text_embeds {e[2]:.2e}")
    if precision == "bf16":
        assert max(e) < 2e-2                                         # tests/test_gpu_clip.py's bf16 forward bound (last_hidden rel-L2)
    else:
        assert max(e) < 1e-4
        np.testing.assert_allclose(pooled.cpu().numpy(), z["text_pooled"], rtol=1e-4, atol=2e-5)
    assert bool(torch.isfinite(last).all())                          # rows after eos are defined
    ids2 = ids.clone()
    for b in range(5):
        ids2[b, eos[b] + 1:] = 7                                     # other pad ids after EOS
    pooled2, _ = m.text_model.forward_hip(ids2, torch.from_numpy(eos).cuda(), False)
    assert torch.equal(pooled2, pooled)
    if precision == "fp32":                                          # the argmax rule (eos_token_id == 2) pools the same rows here
        assert torch.equal(tiny_model("fp32", eos=2).text_model.forward_hip(ids, None, False)[0], pooled)


def contrastive_ref(img, txt, ls, g=1.0):
    img, txt = img.double().clone().requires_grad_(), txt.double().clone().requires_grad_()
    ls = torch.tensor(float(ls), dtype=torch.float64, requires_grad=True)
    i_n, t_n = img / img.norm(dim=-1, keepdim=True), txt / txt.norm(dim=-1, keepdim=True)
    lpt = ls.exp() * t_n @ i_n.t()
    out = dict(lpt=lpt.detach(), i_n=i_n.detach(), t_n=t_n.detach())
    if img.shape[0] == txt.shape[0]:
        B = img.shape[0]
        tgt = torch.arange(B, device=img.device)
        loss = (torch.nn.functional.cross_entropy(lpt, tgt) + torch.nn.functional.cross_entropy(lpt.t(), tgt)) / 2
        (loss * g).backward()
        dS = (torch.softmax(lpt, 1) + torch.softmax(lpt, 0) - 2 * torch.eye(B, dtype=torch.float64, device=img.device)) / (2 * B) * g
        out.update(loss=loss.detach(), d_img=img.grad, d_txt=txt.grad, d_ls=ls.grad, abs_ls=float((dS * lpt).abs().sum()))
    return out


@pytest.mark.parametrize("P", [64, 768])
def test_contrastive_head_against_fp64(L, P):
    from geoguessr_ai_amd.pretrain.clip_model import contrastive
    for B in (1, 2, 5, 64, 257):
        for ls in (2.6592, 4.6052):
            g = torch.Generator().manual_seed(B * 1000 + P)
            img, txt = torch.randn(B, P, generator=g).cuda() * 3, torch.randn(B, P, generator=g).cuda() * 0.5
            lst = torch.tensor(ls, device="cuda")
            r = contrastive(img, txt, lst, True, 0.5)
            r2 = contrastive(img, txt, lst, True, 0.5)
            ref = contrastive_ref(img.cpu(), txt.cpu(), ls, 0.5)
            for k in ("loss", "d_logit_scale", "d_img", "d_txt", "logits_per_text", "logits_per_image", "image_embeds", "text_embeds"):
                assert torch.equal(getattr(r, k), getattr(r2, k)), k                       # no atomics: two calls, same bits
            e_loss = abs(float(r.loss) - float(ref["loss"])) / max(abs(float(ref["loss"])), 1e-30)
            e_ls = abs(float(r.d_logit_scale) - float(ref["d_ls"]))
            print(f"contrastive B={B} P={P} ls={ls}: loss rel {e_loss:.2e}, d_img {rel_l2(r.d_img, ref['d_img']) if B > 1 else 0:.2e}, "
                  f"d_txt {rel_l2(r.d_txt, ref['d_txt']) if B > 1 else 0:.2e}, d_ls abs {e_ls:.2e} of {ref['abs_ls']:.2e}")
            assert rel_l2(r.logits_per_text, ref["lpt"]) < 1e-5 and torch.equal(r.logits_per_image, r.logits_per_text.t())
            assert rel_l2(r.image_embeds, ref["i_n"]) < 1e-6 and rel_l2(r.text_embeds, ref["t_n"]) < 1e-6
            if B == 1:                                   # loss 0, every gradient 0 (one class): absolute
                assert abs(float(r.loss)) < 1e-6 and float(r.d_img.abs().max()) < 1e-6 and float(r.d_txt.abs().max()) < 1e-6 and e_ls < 1e-6
                continue
            assert e_loss < 1e-5
            assert rel_l2(r.d_img, ref["d_img"]) < 1e-5 and rel_l2(r.d_txt, ref["d_txt"]) < 1e-5
            assert e_ls <= 1e-5 * ref["abs_ls"]


def test_contrastive_rectangular_forward_and_refusal(L):
    from geoguessr_ai_amd.pretrain.clip_model import contrastive
    g = torch.Generator().manual_seed(5)
    for Bi, Bt in ((1, 7), (3, 1)):
        img, txt = torch.randn(Bi, 64, generator=g).cuda(), torch.randn(Bt, 64, generator=g).cuda()
        r = contrastive(img, txt, torch.tensor(2.6592, device="cuda"), False)
        ref = contrastive_ref(img.cpu(), txt.cpu(), 2.6592)
        assert r.logits_per_text.shape == (Bt, Bi) and rel_l2(r.logits_per_text, ref["lpt"]) < 1e-5 and torch.equal(r.logits_per_image, r.logits_per_text.t())
        with pytest.raises(L.GgError, match="as many images as texts"):
            contrastive(img, txt, torch.tensor(2.6592, device="cuda"), True)


def set_mask(m, name):
    for n, p in m.named_parameters():
        p.requires_grad = bool(G.MASKS[name](n))


def check_grads(m, z, mask, tol):
    worst = 0.0
    for n, p in m.named_parameters():
        if f"grad.{mask}.{n}" in z:
            e = rel_l2(p.grad, z[f"grad.{mask}.{n}"])
        else:
            assert not p.requires_grad, n
            continue
        if n.endswith("k_proj.bias"):
            # softmax is invariant to a shift of every key by the same vector: this gradient is exactly 0, both sides hold rounding noise.  It is measured
            # against the scale of its sibling, the q_proj.bias gradient of the same layer (same units, same reduction length).
            sib = z[f"grad.{mask}.{n.replace('k_proj', 'q_proj')}"]
            e = float((p.grad.double().cpu().flatten() - torch.from_numpy(z[f"grad.{mask}.{n}"]).double().flatten()).norm() / np.linalg.norm(sib.astype(np.float64)))
        worst = max(worst, e)
        assert e < tol, (mask, n, e)
    return worst


@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
@pytest.mark.parametrize("mask", ["ref", "ref_text", "ref_vis"])
def test_whole_step_against_the_fixture(L, precision, mask):
    z, ids, pix = inputs()
    m = tiny_model(precision)
    set_mask(m, mask)
    out = m(input_ids=ids, pixel_values=pix, attention_mask=torch.from_numpy(z["attention_mask"]).cuda(), return_loss=True)
    out.loss.backward()
    e_loss = abs(float(out.loss) - float(z["loss"])) / float(z["loss"])
    e_fwd = max(rel_l2(out.logits_per_image, z["logits_per_image"]), rel_l2(out.logits_per_text, z["logits_per_text"]), rel_l2(out.text_embeds, z["text_embeds"]),
                rel_l2(out.image_embeds, z["image_embeds"]))
    bf = precision == "bf16"
    worst = check_grads(m, z, mask, 0.15 if bf else 1e-4)            # bf16: tests/test_gpu_clip.py's bf16 training bounds (loss 5e-3, embedding 3e-2, worst gradient 0.15)
    print(f"step [{precision}, {mask}]: loss rel {e_loss:.2e}, forward rel-L2 {e_fwd:.2e}, worst gradient rel-L2 {worst:.2e}")
    assert e_loss < (5e-3 if bf else 1e-5) and e_fwd < (3e-2 if bf else 1e-4)
    # frozen tensors' ranges of the flat gradient buffers stay zero
    for bb in (m.vision_model, m.text_model):
        if bb._flat_grad is not None:
            live = torch.zeros(bb.param_floats, dtype=torch.bool, device="cuda")
            for s, e in bb.trainable_ranges():
                live[s:e] = True
            assert float(bb._flat_grad[~live].abs().max()) == 0.0
    if mask == "ref_vis":                                            # recompute on: bit-identical, in every precision
        m2 = tiny_model(precision)
        set_mask(m2, mask)
        m2.gradient_checkpointing_enable()
        out2 = m2(input_ids=ids, pixel_values=pix, return_loss=True)
        out2.loss.backward()
        assert torch.equal(out2.loss, out.loss)
        for (n, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
            if p.requires_grad:
                assert torch.equal(p.grad, p2.grad), n


def test_three_optimizer_steps_reproduce_the_fixture_trace(L):
    from geoguessr_ai_amd.optim import AdamW
    z, ids, pix = inputs()
    m = tiny_model("fp32")
    set_mask(m, "ref")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = AdamW(m, lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=1e-3)
    for step in range(3):
        opt.zero_grad()
        loss = m(input_ids=ids, pixel_values=pix, return_loss=True).loss
        loss.backward()
        norm = opt.clip_grad_norm_(1.0)
        opt.step()
        torch.cuda.synchronize()
        print(f"step {step}: loss {float(loss):.7f} (fixture {z['trace_loss'][step]:.7f}), norm {norm:.6f} ({z['trace_norm'][step]:.6f}), "
              f"logit_scale {float(m.logit_scale):.7f} ({z['trace_logit_scale'][step]:.7f})")
        assert abs(float(loss) - z["trace_loss"][step]) < 1e-5 * z["trace_loss"][step]
        assert abs(norm - z["trace_norm"][step]) < 1e-5 * z["trace_norm"][step]
        assert abs(float(m.logit_scale) - z["trace_logit_scale"][step]) < 1e-6
    assert z["trace_norm"][0] > 1.0
    assert rel_l2(m.visual_projection.weight, z["trace_visual_projection"]) < 1e-5
    for k, v in m.state_dict().items():
        if k not in ("logit_scale", "visual_projection.weight"):
            assert torch.equal(v, before[k]), k


def test_clip_coefficient_reaches_the_update(L):
    """With eps = 1e-6 an AdamW step hardly depends on a global gradient scale, so the trace above cannot show that clip_grad_norm_'s coefficient is applied.  With
    eps = 1e5 the first step is lr g s / (|g s| + eps), proportional to the scaled gradient to within |g| / eps <= norm / eps = 8e-5: a clipped step must equal, bit
    for bit, the step taken with grad_scale = s = min(1, 1 / (norm + 1e-6)), move each parameter s times as far as the unclipped step (gate 1e-3: the 8e-5 above plus
    the f32 rounding of a parameter next to its update, 2.4e-7 / 6e-3 for logit_scale), and leave the coefficient spent."""
    from geoguessr_ai_amd.optim import AdamW
    z, ids, pix = inputs()
    after = {}
    for how in ("clipped", "scaled", "plain"):
        m = tiny_model("fp32")
        set_mask(m, "ref")
        start = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
        opt = AdamW(m, lr=1e3, betas=(0.9, 0.98), eps=1e5, weight_decay=0.0)
        m(input_ids=ids, pixel_values=pix, return_loss=True).loss.backward()
        if how == "clipped":
            norm = opt.clip_grad_norm_(1.0)
            assert norm > 1.0 and opt._clip_coef == min(1.0, 1.0 / (norm + 1e-6))
            opt.step()
            assert opt._clip_coef == 1.0
        elif how == "scaled":
            opt.step(grad_scale=min(1.0, 1.0 / (norm + 1e-6)))
        else:
            opt.step()
        after[how] = {n: p.detach() - start[n] for n, p in m.named_parameters() if p.requires_grad}
    for n in after["plain"]:
        assert torch.equal(after["clipped"][n], after["scaled"][n]), n
        ratio = float(after["clipped"][n].double().norm() / after["plain"][n].double().norm())
        print(f"{n}: clipped / unclipped update {ratio:.6f}, 1 / norm {1 / norm:.6f}")
        assert abs(ratio * norm - 1.0) < 1e-3, (n, ratio, norm)


def test_model_refusals(L):
    z, ids, pix = inputs()
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel
    with pytest.raises(L.GgError):
        CLIPModel(config=G.tiny_config(), precision="fp16")
    m = tiny_model("fp32")
    with pytest.raises(L.GgError, match="position table"):
        m.text_model.forward_hip(torch.zeros(2, 78, dtype=torch.int64, device="cuda"))
    with pytest.raises(L.GgError, match="eos_pos outside"):
        m.text_model.forward_hip(ids, torch.full((5,), 9, dtype=torch.int32, device="cuda"))
    with pytest.raises(L.GgError, match="input_ids outside"):
        m.text_model.forward_hip(ids + 60)
    # a trainable text tensor at a loss backward is named
    set_mask(m, "ref")
    m.text_model._params["final_layer_norm.weight"].requires_grad = True
    out = m(input_ids=ids, pixel_values=pix, return_loss=True)
    with pytest.raises(L.GgError, match="text_model.final_layer_norm.weight"):
        out.loss.backward()
    assert m.visual_projection.weight.grad is None
    # C level: act_dtype 2, head dim 32 and 78 tokens write nothing (buffers sized for the 78-token call, so that nothing could land outside them either)
    ok = L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, 1)
    pooled = torch.full((5, 128), float("nan"), device="cuda")
    last = torch.full((5, 78, 128), float("nan"), device="cuda")
    ws = torch.full((2 * L.lib().gg_clip_text_workspace_bytes(C.byref(ok), 5, 77),), 0xFF, dtype=torch.uint8, device="cuda")
    ids78 = torch.zeros(5, 78, dtype=torch.int32, device="cuda")
    for bad, tok in ((L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, 2), 9), (L.ClipTextCfg(128, 256, 2, 4, 64, 77, 1e-5, 1), 9), (ok, 78)):
        rc = L.lib().gg_clip_text_forward(C.byref(bad), 5, tok, m.text_model._flat.data_ptr(), m.text_model._wcache.data_ptr(), ids78.data_ptr(),
                                          torch.zeros(5, dtype=torch.int32, device="cuda").data_ptr(), ws.data_ptr(), last.data_ptr(), pooled.data_ptr(), L.stream())
        torch.cuda.synchronize()
        assert rc != 0 and bool(torch.isnan(pooled).all()) and bool(torch.isnan(last).all()) and bool((ws == 0xFF).all()), tok
    assert b"position" in L.lib().gg_last_error()


@pytest.mark.parametrize("name", ["openai/clip-vit-base-patch32", "openai/clip-vit-large-patch14-336"])
def test_real_text_dimensions_split_against_fp32(L, name):
    """fp32_split against fp32 text_embeds, rel-L2 1e-5 (the gate of test_embedding_wrapper_matches_the_fp32_tower): routing at K = 512 / 768 / 2048 / 3072."""
    from geoguessr_ai_amd.pretrain.clip_model import CLIP_TEXT_CONFIGS, TEXT_DEFAULTS, _TextModel
    from geoguessr_ai_amd import ops
    tk = dict(TEXT_DEFAULTS, **CLIP_TEXT_CONFIGS[name])
    ids = torch.randint(0, 49407, (4, 77), generator=torch.Generator().manual_seed(1)).cuda()
    ids[:, -1] = 49407
    proj = (torch.randn(tk["projection_dim"], tk["hidden_size"], generator=torch.Generator().manual_seed(2)) * tk["hidden_size"] ** -0.5).cuda()
    emb = {}
    for code in (1, 3):
        c = L.ClipTextCfg(tk["hidden_size"], tk["intermediate_size"], tk["num_layers"], tk["num_heads"], tk["vocab_size"], tk["max_positions"], 1e-5, code)
        tm = _TextModel(c, 11, 2).cuda()
        te = ops.gemm_nt(tm.forward_hip(ids)[0], proj)
        emb[code] = te / te.norm(dim=-1, keepdim=True)
        del tm
    e = rel_l2(emb[3], emb[1])
    print(f"{name}: fp32_split vs fp32 text_embeds rel-L2 {e:.2e}")
    assert bool(torch.isfinite(emb[1]).all()) and e < 1e-5
