"""CPU-only checks of the CLIP tower's fp8 (e4m3) inference mode: the numerics contract as tests/clip_fp8_ref.py restates it, the precision names, and the host
side of the new entry points (size queries, refusals, the boundary of include/gg_fp8.h).  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import clip_fp8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _rows():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(9, 256, generator=g) * torch.tensor([1e-3, 1.0, 30.0, 1e4, 1.0, 1.0, 1.0, 1.0, 1.0])[:, None]
    x[4] = 0.0                                            # a zero row
    x[5] = 0.0; x[5, 77] = -0.37                          # one nonzero
    x[6, 0] = 3.0; x[6, 1:] *= 2.0 ** -13                 # one large element, the rest around and below e4m3's smallest normal (2^-6) after scaling
    x[7, 0] = 448.0                                       # inv == 1: the elements below sit exactly on e4m3 rounding ties
    x[7, 1:9] = torch.tensor([17.0, 19.0, -1.0625, 2.0 ** -10, 3 * 2.0 ** -10, 432.0, -2.0 ** -10, 208.0])
    return x


def test_quant_rows_properties():
    x = _rows()
    codes, scale = R.quant_rows(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scale.shape == (9,) and scale.dtype == torch.float32
    assert float(scale[4]) == 1.0 and int(codes[4].max()) == 0                       # zero row -> scale 1, zero codes
    assert not bool(((codes & 0x7F) == 0x7F).any())                                  # no NaN code (S.1111.111), i.e. every code finite
    val = R.decode(codes)
    assert float(val.abs().max()) <= 448.0
    y = x.double() / scale.double()[:, None]
    err = (val * scale.double()[:, None] - x.double()).abs()
    half = 0.5 * R.e4m3_spacing(y) * scale.double()[:, None]
    assert bool((err <= half * (1 + 1e-6) + 1e-30).all()), float((err / half).max())  # (1e-6: x * inv in f32 against x / scale in fp64)
    for r in (0, 1, 2, 3, 5, 6, 7, 8):                                               # the largest element of a row maps to +-448
        k = int(x[r].abs().argmax())
        assert float(val[r, k].abs()) == 448.0 and float(val[r, k].sign()) == float(x[r, k].sign())
    assert float(scale[5]) == float(torch.tensor(0.37, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32))
    # ties go to the even code, subnormals included: 17 -> 16, 19 -> 20, 1.0625 -> 1.0, 2^-10 -> 0, 3 * 2^-10 -> 2^-8, 432 -> 448, 208 -> 208
    assert val[7, 1:9].tolist() == [16.0, 20.0, -1.0, 0.0, 2.0 ** -8, 448.0, -0.0, 208.0]
    sub = (val[6, 1:].abs() < 2.0 ** -6) & (val[6, 1:] != 0)
    assert int(sub.sum()) >= 64                                                      # the subnormal range is used, not flushed


def test_precision_names(L):
    from geoguessr_ai_amd.pretrain import clip_embedder as E
    """The mode's code is GG_CLIP_ACT_FP8 = 8 and its name goes through ``tower_precision_code``, not through ``_precision_code``: code 4 and
    ``_precision_code("fp8")`` are what tests/test_clip_split_cpu.py keeps pinned as refused (an unknown mode, an unknown name), and stay so."""
    hdr = open(os.path.join(ROOT, "include", "gg_fp8.h")).read()
    assert int(re.search(r"#define GG_CLIP_ACT_FP8 (\d+)", hdr).group(1)) == E.FP8_CODE == 8
    assert E.tower_precision_code("fp8") == 8 and E.tower_precision_code("e4m3") == 8 and E.PRECISION_NAMES[8] == "fp8"
    assert E.tower_precision_code("fp16") == 2 and E.tower_precision_code("fp32_split") == 3 and E.tower_precision_code(None) == E._precision_code(None)
    with pytest.raises(ValueError, match=r"known: .*fp32_split.*fp8"):
        E.tower_precision_code("fp4")
    with pytest.raises(ValueError, match="fp32_split"):
        E._precision_code("fp8")
    tower = E.CLIPVisionTower("openai/clip-vit-base-patch32", precision="fp8", num_layers=1)
    assert tower.cfg.act_dtype == 8 and tower.precision == "fp8" and tower.backbone.precision == "fp8"


def test_gg_precision_does_not_take_fp8(L, monkeypatch):
    from geoguessr_ai_amd.pretrain import clip_embedder as E
    monkeypatch.setenv("GG_PRECISION", "fp8")
    with pytest.raises(ValueError, match="GG_PRECISION"):
        E.tower_precision_code(None)


def test_tinyvit_refuses_fp8():
    from geoguessr_ai_amd.models import tinyvit as T
    assert "fp8" not in T.PRECISIONS and "e4m3" not in T.PRECISIONS
    with pytest.raises(ValueError, match="precision='fp8'"):
        T.make_cfg("tiny_vit_5m_224", precision="fp8")


def _cfg(L, hs, inter, nl, nh, img, ps, act):
    c = L.ClipCfg()
    c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads, c.image_size, c.patch_size, c.ln_eps, c.act_dtype, c.recompute = hs, inter, nl, nh, img, ps, 1e-5, act, 0
    return c


@pytest.mark.parametrize("shape,batch", [((128, 512, 2, 2, 64, 32), 3), ((768, 3072, 12, 12, 224, 32), 8), ((1024, 4096, 24, 16, 336, 14), 2)])
def test_size_queries_answer_for_the_fp8_mode(L, shape, batch):
    lib = L.lib()
    hs, inter, nl = shape[:3]
    T = (shape[4] // shape[5]) ** 2 + 1
    c2, c4 = _cfg(L, *shape, 2), _cfg(L, *shape, 8)
    wc2, wc4 = lib.gg_clip_wcache_bytes(C.byref(c2)), lib.gg_clip_wcache_bytes(C.byref(c4))
    ws2, ws4 = lib.gg_clip_workspace_bytes(C.byref(c2), batch, 0, None), lib.gg_clip_workspace_bytes(C.byref(c4), batch, 0, None)
    assert wc2 > 0 and ws2 > 0 and wc4 > 0 and ws4 > 0, lib.gg_last_error()
    codes = nl * (4 * hs * hs + 2 * hs * inter)                       # e4m3 images of wqkv, wo, w1, w2
    scales = nl * 4 * (3 * hs + hs + inter + hs)
    assert wc4 - wc2 >= codes + scales
    assert ws4 - ws2 >= batch * T * max(hs, inter) + 4 * batch * T    # the code buffer and one scale row
    assert lib.gg_clip_num_tensors(C.byref(c4)) == lib.gg_clip_num_tensors(C.byref(c2))
    assert lib.gg_clip_param_floats(C.byref(c4)) == lib.gg_clip_param_floats(C.byref(c2))


def test_fp8_mode_refusals_on_the_host(L):
    lib = L.lib()
    c = _cfg(L, 192, 768, 2, 3, 64, 32, 8)
    assert lib.gg_clip_wcache_bytes(C.byref(c)) < 0
    msg = lib.gg_last_error().decode()
    assert "fp8" in msg and "128" in msg and "192" in msg, msg
    assert lib.gg_clip_workspace_bytes(C.byref(c), 2, 0, None) < 0
    assert lib.gg_clip_wcache_bytes(C.byref(_cfg(L, 192, 768, 2, 3, 64, 32, 2))) > 0      # the same shape is fine in the fp16 mode
    c = _cfg(L, 128, 320, 2, 2, 64, 32, 8)                                                  # intermediate_size not a multiple of 128
    assert lib.gg_clip_wcache_bytes(C.byref(c)) < 0 and "fp8" in lib.gg_last_error().decode()
    for bad in (4, 5, 7, 9):                                                                # the codes around the mode stay refused
        assert lib.gg_clip_wcache_bytes(C.byref(_cfg(L, 128, 512, 2, 2, 64, 32, bad))) < 0 and "act_dtype" in lib.gg_last_error().decode()
    # the text tower has no fp8 mode
    t = L.ClipTextCfg()
    t.hidden_size, t.intermediate_size, t.num_layers, t.num_heads, t.vocab_size, t.max_positions, t.ln_eps, t.act_dtype = 128, 512, 2, 2, 100, 77, 1e-5, 8
    assert lib.gg_clip_text_wcache_bytes(C.byref(t)) < 0
    assert "fp8" in lib.gg_last_error().decode()
    # training entry points answer before they touch a pointer
    c = _cfg(L, 128, 512, 2, 2, 64, 32, 8)
    one = C.c_void_p(256)
    assert lib.gg_clip_forward(C.byref(c), 1, 1, one, one, one, one, one, None, None, None) != 0
    assert "gg_clip_forward" in lib.gg_last_error().decode() and "fp8" in lib.gg_last_error().decode()
    assert lib.gg_clip_backward(C.byref(c), 1, one, one, one, one, None, one, None, None) != 0
    assert "gg_clip_backward" in lib.gg_last_error().decode() and "fp8" in lib.gg_last_error().decode()


def test_fp8_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_fp8.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.FP8_SYMBOLS) == {"gg_gemm_nt_e4m3", "gg_quant_rows_e4m3", "gg_layernorm_fwd_e4m3"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.FP8_SIGNATURES[n][1]), n
    assert "gg_fp8.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "gemm_fp8.hip" in mk and "gg_fp8.h" in mk
    # gg.h's symbol set is not extended
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg.h")).read(), flags=re.S)
    assert not (declared & set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", main)))


def test_kernel_refusals_answer_on_the_host(L):
    """Argument validation of the three kernels precedes any launch: it answers by name without a device."""
    lib = L.lib()
    a = L.GemmArgs()
    a.A, a.B, a.C, a.lda, a.ldb, a.ldc, a.M, a.N, a.K = 256, 256, 256, 128, 128, 64, 4, 64, 128
    sa = sw = C.c_void_p(256)

    def refused(word, **kw):
        b = L.GemmArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        assert lib.gg_gemm_nt_e4m3(C.byref(b), sa, sw, None) != 0, word
        msg = lib.gg_last_error().decode()
        assert "gg_gemm_nt_e4m3" in msg and word in msg, (word, msg)
    refused("preact", preact=256)
    refused("dact", dact_preact=256, dact=2)
    refused("colstats", colstats=256)
    refused("split", split_k=2)
    refused("K must be a multiple of 128", K=192, lda=192, ldb=192)
    refused("N must be a multiple of 16", N=40)
    refused("act", act=1)
    assert lib.gg_quant_rows_e4m3(C.c_void_p(256), 0, 100, 4, 100, C.c_void_p(256), 104, C.c_void_p(256), None) != 0
    assert "gg_quant_rows_e4m3" in lib.gg_last_error().decode()
    assert lib.gg_layernorm_fwd_e4m3(C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), 4, 2048, L.f32(1e-5), C.c_void_p(256), 2048, C.c_void_p(256), None) != 0
    assert "gg_layernorm_fwd_e4m3" in lib.gg_last_error().decode()
