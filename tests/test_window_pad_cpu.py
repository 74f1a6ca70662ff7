"""Padded attention windows (include/gg_pad.h; TinyViT at an input size whose stage maps the window does not divide) on the host side: the padded reference block
the GPU tests compare against (tests/tinyvit_pad_ref.py) is pinned to timm's semantics, the header and its binding agree, and the workspace plan of the built
libgg.so accepts the padded cases -- regions aligned, disjoint and inside the total -- while every size that divides keeps the plan it had.  No GPU needed."""
import ctypes as C
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import tinyvit_pad_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FROZEN = ("stages.0.", "stages.1.", "stages.2.")


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


# ------------------------------------------------------------------------------------------- the reference block
def _state(cfg, seed, dtype=torch.float32):
    from oracle import tinyvit_ref as R
    st = R.init_state(cfg, seed=seed, randomize_norms=True)
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}


def test_helper_block_is_the_oracle_block_on_a_map_that_divides(monkeypatch):
    from oracle import tinyvit_ref as R
    cfg = R.config_for("tiny_vit_5m_224", drop_path_rate=0.1)
    st = _state(cfg, 3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 224, 224, generator=g)
    masks = [torch.rand(2, generator=g) > 0.3 for _ in range(cfg.depths[0] + 2 * sum(cfg.depths[1:]))]
    want = R.forward(cfg, {k: v.clone() for k, v in st.items()}, x, training=True, drop_masks=masks)
    monkeypatch.setattr(R, "_tinyvit_block_m", P.tinyvit_block_padded)
    got = R.forward(cfg, {k: v.clone() for k, v in st.items()}, x, training=True, drop_masks=masks)
    assert torch.equal(got, want)


def _one_block(mask_pad_keys=False, H=10, ws=7, C=64, nh=2, B=2, seed=5):
    """One padded block in fp64 with gradients: (output, d attn.norm.bias, the pieces the direct formulation needs)."""
    from oracle import tinyvit_ref as R
    cfg = R.config_for("tiny_vit_5m_224", embed_dims=(64, C, 160, 320), num_heads=(2, nh, 5, 10), window_sizes=(7, ws, 14, 7))
    st = _state(cfg, seed, torch.float64)
    p = "stages.1.blocks.0"
    with torch.no_grad():
        st[f"{p}.attn.norm.bias"].mul_(5.0)                       # a pad key that matters
    st = {k: (v.clone().requires_grad_(True) if k.startswith(p) and v.is_floating_point() and "running" not in k else v) for k, v in st.items()}
    c = R._Ctx(cfg, st, True, False, False, None)
    x = torch.randn(B, H, H, C, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 1))
    y = P.tinyvit_block_padded(c, x, p, nh, ws, None, 0, mask_pad_keys=mask_pad_keys)
    w = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 2))
    (y * w).sum().backward()
    return y.detach(), st[f"{p}.attn.norm.bias"].grad.clone(), (cfg, st, c, x, p)


def test_helper_block_is_the_specified_padding():
    """Pad tokens are zero rows in front of attn.norm, so they leave the norm as norm.bias and take part in their window as the constant key / value qkv(norm.bias); the
    result at the real tokens equals attention over [LayerNorm of the real tokens | norm.bias rows], to fp64 rounding."""
    from oracle import tinyvit_ref as R
    H, ws, C, nh, B = 10, 7, 64, 2, 2
    y, _, (cfg, st, c, x, p) = _one_block(H=H, ws=ws, C=C, nh=nh, B=B)
    with torch.no_grad():
        pres = P.padded_side(H, ws)
        assert pres == 14
        xn = F.layer_norm(x, (C,), st[f"{p}.attn.norm.weight"], st[f"{p}.attn.norm.bias"], cfg.ln_eps)
        full = st[f"{p}.attn.norm.bias"].detach().expand(B, pres, pres, C).clone()
        full[:, :H, :H] = xn
        n = pres // ws
        xw = full.view(B, n, ws, n, ws, C).transpose(2, 3).reshape(B * n * n, ws * ws, C)
        a = R._attention_core(c, xw, p, nh, ws).view(B, n, n, ws, ws, C).transpose(2, 3).reshape(B, pres, pres, C)[:, :H, :H]
        x1 = x + a
        # the rest of the block on the unpadded map, from the helper itself: feed x1 through a block whose attention branch is switched off
        rest = lambda t: _rest_of_block(c, t, p, C)
        want = rest(x1)
    assert float((y - want).abs().max()) <= 1e-12 * float(want.abs().max())


def _rest_of_block(c, x1, p, C):
    from oracle import tinyvit_ref as R
    B, H, W, _ = x1.shape
    st = c.st
    x = R._convnorm(c, x1.permute(0, 3, 1, 2), f"{p}.local_conv", 1, 1, C, dense=False).reshape(B, C, H * W).transpose(1, 2)
    h = F.layer_norm(x, (C,), st[f"{p}.mlp.norm.weight"], st[f"{p}.mlp.norm.bias"], c.cfg.ln_eps)
    h = F.linear(F.gelu(F.linear(h, st[f"{p}.mlp.fc1.weight"], st[f"{p}.mlp.fc1.bias"])), st[f"{p}.mlp.fc2.weight"], st[f"{p}.mlp.fc2.bias"])
    return (x + h).view(B, H, W, C)


def test_masking_the_pad_keys_is_a_different_block():
    y, db, _ = _one_block(False)
    ym, dbm, _ = _one_block(True)
    assert float((y - ym).abs().max()) > 1e-3 * float(y.abs().max())
    assert float(db.abs().max()) > 0 and float((db - dbm).norm()) > 1e-3 * float(db.norm())      # the pad keys / values send gradient into attn.norm.bias


# ------------------------------------------------------------------------------------------- header and binding
def test_pad_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_pad.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.PAD_SYMBOLS) == {"gg_window_pad", "gg_window_crop_add"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(L.PAD_SIGNATURES[n][1]), n
        assert args[-2:] == ["int dtype", "void* stream"], n
    # include/gg.h keeps its symbol set: the new entry points are declared in their own header only
    gg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", gg)) == set(L.SYMBOLS) and not declared & set(L.SYMBOLS)
    assert "gg_pad.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]


def test_bad_arguments_are_refused_without_a_device(L):
    lib = L.lib()
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) & ~15
    assert lib.gg_window_pad(p, p, 1, 5, 5, 4, 7, 64, 1, None) != 0 and b"gg_window_pad: bad shape" in lib.gg_last_error()          # padded side below the map's
    assert lib.gg_window_pad(p, p, 1, 5, 5, 7, 7, 6, 0, None) != 0 and b"16-byte" in lib.gg_last_error()                            # 12-byte rows
    assert lib.gg_window_pad(p, p, 1, 5, 5, 7, 7, 64, 2, None) != 0 and b"dtype" in lib.gg_last_error()
    assert lib.gg_window_crop_add(p, None, None, p + 4, 1, 5, 5, 7, 7, 64, 1, None) != 0 and b"aligned" in lib.gg_last_error()
    assert lib.gg_window_crop_add(None, None, None, p, 1, 5, 5, 7, 7, 64, 1, None) != 0 and b"null" in lib.gg_last_error()


# ------------------------------------------------------------------------------------------- workspace plan
def _cfg(name, img, depths, precision, recompute):
    from geoguessr_ai_amd.models.tinyvit import make_cfg, _tensor_table
    kw = dict(precision=precision, grad_checkpointing=bool(recompute), img_size=img)
    if depths is not None:
        kw["depths"] = depths
    cfg, _, depths = make_cfg(name, **kw)
    table = _tensor_table(cfg)
    freeze = bytes(int(t["kind"] == 0 and not t["name"].startswith(FROZEN)) for t in table)
    return cfg, depths, freeze


def _ws(L, cfg, batch, mask, training=1):
    n = L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(cfg), batch, training, mask)
    assert n > 0, L.lib().gg_last_error().decode()
    return n


def _info(L, cfg, batch, name, mask):
    off, nb = C.c_int64(), C.c_int64()
    rc = L.lib().gg_tinyvit_activation_info_masked(C.byref(cfg), batch, name.encode(), mask, C.byref(off), C.byref(nb))
    return (off.value, nb.value) if rc == 0 else L.lib().gg_last_error().decode()


@pytest.mark.parametrize("name,img,depths,batch", P.PAD_CASES)
@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
def test_padded_sizes_get_a_plan(L, name, img, depths, batch, precision):
    """The refusal ("... not divisible by window (padding path not built)") is gone: every query answers, training and inference, with and without a mask."""
    for rc in (0, 1):
        cfg, _, freeze = _cfg(name, img, depths, precision, rc)
        assert L.lib().gg_tinyvit_num_tensors(C.byref(cfg)) > 0, L.lib().gg_last_error().decode()
        assert _ws(L, cfg, batch, None) >= _ws(L, cfg, batch, freeze) > 0
        assert _ws(L, cfg, batch, None, training=0) > 0


def _block_names(s, i):
    b = f"stages.{s}.blocks.{i}"
    return [f"{b}.{leaf}" for leaf in ("attn.xpad", "ln1", "mean1", "rstd1", "qkv", "attn.out", "attn.lse", "x1", "local_conv.y", "local_conv.stat", "x2", "ln2", "mean2", "rstd2",
                                       "fc1.pre", "fc1.act", "out")]


@pytest.mark.parametrize("name,img,depths,batch", P.PAD_CASES)
@pytest.mark.parametrize("mode", ["recompute_off", "recompute_on", "freeze_mask"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_padded_plan_regions_are_aligned_disjoint_and_inside(L, name, img, depths, batch, mode, precision):
    """Every region that stays addressable under the plan (the padded blocks' included, at their padded sizes) is 256-byte aligned, inside the total, and overlaps no
    other; under recompute the segment-internal tensors are refused as recomputed and the segment region stands for them; under the freeze mask the temporaries are
    refused as temporaries and the ring they share is the first two gradient buffers."""
    cfg, dp, freeze = _cfg(name, img, depths, precision, mode == "recompute_on")
    mask = freeze if mode == "freeze_mask" else None
    es = 2 if precision == "bf16" else 4
    total = _ws(L, cfg, batch, mask)
    names = ["patch_embed.col1", "patch_embed.conv1.y", "patch_embed.col2", "patch_embed.conv2.y", "patch_embed.out", "head.pooled", "scratch.statpart", "scratch.padtmp",
             "scratch.bn", "scratch.ln", "scratch.colsum", "scratch.splitk", "scratch.foldw"] + [f"scratch.G{i}" for i in range(5)]
    if mode == "recompute_on":
        names.append("scratch.segment")
    for i in range(dp[0]):
        names += [f"stages.0.blocks.{i}.out", f"stages.0.blocks.{i}.conv1.y", f"stages.0.blocks.{i}.conv3.y"]
    padded = {}
    for s in (1, 2, 3):
        res, ws = img // (4 * 2 ** s), cfg.window_sizes[s]
        names += [f"stages.{s}.downsample.out", f"stages.{s}.downsample.conv2.y"]
        for i in range(dp[s]):
            names += [n for n in _block_names(s, i) if res % ws or not n.endswith("attn.xpad")]
            if res % ws:
                padded[f"stages.{s}.blocks.{i}"] = (batch * P.padded_side(res, ws) ** 2, cfg.embed_dims[s], cfg.num_heads[s])
            else:
                assert "no activation named" in _info(L, cfg, batch, f"stages.{s}.blocks.{i}.attn.xpad", mask)
    assert padded
    regions, refused = {}, {}
    for n in names:
        r = _info(L, cfg, batch, n, mask)
        (regions if isinstance(r, tuple) else refused)[n] = r
    for n, msg in refused.items():
        assert ("recompute" in msg) if mode == "recompute_on" else (mode == "freeze_mask" and "temporary" in msg), (n, msg)
    if mode == "recompute_off":
        assert not refused
    for n, (o, b) in regions.items():
        assert o >= 0 and b > 0 and o % 256 == 0 and o + b <= total, (n, o, b, total)
    spans = sorted((o, o + b, n) for n, (o, b) in regions.items())
    for (o0, e0, n0), (o1, e1, n1) in zip(spans, spans[1:]):
        assert e0 <= o1, (n0, n1)
    # the padded blocks' attention-branch tensors hold Mp rows
    al = lambda v: -(-v // 256) * 256
    for b, (Mp, Cc, nh) in padded.items():
        want = {"attn.xpad": Mp * Cc * es, "ln1": Mp * Cc * es, "mean1": Mp * 4, "rstd1": Mp * 4, "qkv": Mp * 3 * Cc * es, "attn.out": Mp * Cc * es, "attn.lse": Mp * nh * 4}
        for leaf, nbytes in want.items():
            if f"{b}.{leaf}" in regions:
                assert regions[f"{b}.{leaf}"][1] == al(nbytes), (b, leaf)
        if mode == "recompute_off":
            assert f"{b}.attn.xpad" in regions
        assert regions["scratch.padtmp"][1] >= Mp * Cc * es and regions["scratch.G2"][1] >= Mp * 3 * Cc * es


def test_native_sizes_keep_the_parent_plan_to_the_byte(L):
    """gg_tinyvit_workspace_bytes_masked of the five variants at their own size, batch 8, all modes, masks None / freeze policy, recompute off / on: the totals the commit
    in front of the padding path gave (tests/golden/tinyvit_plan_bytes_parent.json, written by tests/golden/make_golden_plan_bytes.py with that build)."""
    from geoguessr_ai_amd.models.tinyvit import VARIANTS
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "tinyvit_plan_bytes_parent.json")))
    assert len(want) == len(VARIANTS) * 3 * 2 * 2 == 60
    got = {}
    for name in VARIANTS:
        for precision in ("bf16", "fp32", "fp32_split"):
            for rc in (0, 1):
                cfg, _, freeze = _cfg(name, VARIANTS[name]["img_size"], None, precision, rc)
                for label, mask in (("none", None), ("freeze", freeze)):
                    got[f"{name}/{precision}/{label}/rc{rc}"] = _ws(L, cfg, 8, mask)
                    assert "no activation named" in _info(L, cfg, 8, "scratch.padtmp", mask)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_python_surface(L):
    import warnings
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter, VARIANTS
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, v in VARIANTS.items():
            if name.startswith("tiny_vit_21m_224") or name.startswith("tiny_vit_11m"):
                continue                      # (same maps as 5M-224: one of the three is enough for the constructor)
            assert TinyViTAdapter(name, pretrained=False, precision="fp32").backbone.padded_maps == ()
        m = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="fp32", img_size=160)
        assert m.backbone.padded_maps == ((1, 20, 21), (2, 10, 14), (3, 5, 7)) and m.backbone.img_size == 160
        assert TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="bf16", img_size=512).backbone.padded_maps == ((1, 64, 70), (2, 32, 42), (3, 16, 21))
        c = TinyViTClassifier("tiny_vit_5m_224", num_classes=7, img_size=256, precision="fp32")
        assert c.backbone.padded_maps == ((1, 32, 35), (2, 16, 28), (3, 8, 14))
        assert TinyViTAdapter("tiny_vit_21m_384", pretrained=False, precision="fp32", img_size=288, depths=(1, 1, 2, 1)).backbone.padded_maps == ((2, 18, 24), (3, 9, 12))
    with pytest.raises(L.GgError, match="multiple of 32"):
        TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="fp32", img_size=200)
