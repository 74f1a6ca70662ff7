"""CPU-only checks of the 16-bit-MFMA window attention forward beyond 256 tokens (include/gg_attn16w.h): the header against the binding, TinyViT's
``attention16`` keyword and its refusals, the entry point's refusals (they answer on the host, before any launch), and the arithmetic contract restated in torch
(tests/attention16_win_cases.py) against the gates tests/test_gpu_attention16_win.py holds the kernel to -- which pins those gates to something a correct kernel
can meet.  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import attention16_win_cases as A
from tests import attention_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "gg_attention_flash16_win_fwd"


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_attn16w_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_attn16w.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.ATTN16W_SYMBOLS) == {"gg_attention_flash16_win_fwd", "gg_attention_flash16_win_calls", "gg_tinyvit_set_attention16"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(L.ATTN16W_SIGNATURES[n][1]), n
    assert L.ATTN16W_SIGNATURES["gg_attention_flash16_win_calls"][0] is C.c_int64
    assert "gg_attn16w.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "attention_flash16.hip" in mk.split("SRCS")[1].split("\n")[0] and "attention_flash16_win.hip" not in mk      # one translation unit holds both entry points
    assert "gg_attn16w.h" in mk.split("attention_flash16.hip.o ../lib/obj/tinyvit.hip.o:")[1].split("\n")[0]
    for other in ("gg.h", "gg_attn16.h"):                                   # the new symbols live in their own header
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not (declared & set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", text))), other
    assert not (declared & set(L.SYMBOLS)) and not (declared & set(L.ATTN16_SYMBOLS))


def test_switch_defaults_off_and_returns_the_previous_value(L):
    lib = L.lib()
    n, n64 = lib.gg_attention_flash16_win_calls(), lib.gg_attention_flash16_calls()
    assert lib.gg_tinyvit_set_attention16(1) == 0 and lib.gg_tinyvit_set_attention16(5) == 1 and lib.gg_tinyvit_set_attention16(0) == 1
    assert lib.gg_tinyvit_set_attention16(0) == 0
    assert lib.gg_clip_set_attention16(0) == 0                              # CLIP's switch is another one
    assert lib.gg_attention_flash16_win_calls() == n and lib.gg_attention_flash16_calls() == n64          # a switch flip launches nothing


def test_keyword_and_its_refusals(L, monkeypatch):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter, TinyVitBackbone
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    kw = dict(depths=(1, 1, 1, 1), drop_path_rate=0.0)
    on = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="bf16", attention16=True, **kw)
    assert on.backbone.attention16 is True and on.backbone.precision == "bf16"
    assert TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="bf16", **kw).backbone.attention16 is False
    assert TinyViTClassifier("tiny_vit_5m_224", num_classes=3, precision="bf16", attention16=True, **kw).backbone.attention16 is True
    assert TinyVitBackbone("tiny_vit_5m_224", precision="bf16", attention16=True, **kw).attention16 is True
    for precision in ("fp32", "fp32_split"):
        with pytest.raises(L.GgError, match=rf"TinyViTAdapter: attention16=True .*precision='{precision}'"):
            TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision=precision, attention16=True, **kw)
        with pytest.raises(L.GgError, match=rf"TinyVitBackbone: attention16=True .*precision='{precision}'"):
            TinyVitBackbone("tiny_vit_5m_224", precision=precision, attention16=True, **kw)
        with pytest.raises(L.GgError, match=rf"TinyViTClassifier: attention16=True .*precision='{precision}'"):
            TinyViTClassifier("tiny_vit_5m_224", num_classes=3, precision=precision, attention16=True, **kw)
        monkeypatch.setenv("GG_PRECISION", precision)                       # the embedder has no precision keyword: the process default decides
        with pytest.raises(L.GgError, match=rf"TinyViTEmbedding: attention16=True .*precision='{precision}'"):
            TinyViTEmbedding("tiny_vit_5m_224", device="cpu", attention16=True)
        with pytest.raises(L.GgError, match=rf"TinyViTAdapter: attention16=True .*precision='{precision}'"):
            TinyViTAdapter("tiny_vit_5m_224", pretrained=False, attention16=True, **kw)
        TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision=precision, attention16=False, **kw)
    src = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "tinyvit.hip")).read()
    assert "GG_ATTENTION16" not in src                                      # no environment variable
    assert ".add((int)attn16)" in src.split('key.add(\'F\')')[1].split("gg_graph_run")[0]          # the switch is part of the forward's graph key


def _args(L, **over):
    a = L.AttnArgs()
    a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = 256, 192, 0, 32, 64, 96, 32
    a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = 2, 4, 289, 17, 34, 34, 32 ** -0.5
    a.bias_table, a.out, a.ldo = 1024, 512, 64
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(head_dim=64), 0, "head_dim must be 32"), (dict(head_dim=16), 0, "head_dim must be 32"),
    (dict(window_size=0, map_h=0, map_w=0), 0, "window_size must be 1 .. 32 (got 0"), (dict(window_size=33, tokens_per_window=1089, map_h=66, map_w=66), 0, "window_size must be 1 .. 32 (got 33"),
    (dict(window_size=-1), 0, "window_size must be 1 .. 32"),
    (dict(bias=256, bias_table=None), 0, "bias (the expanded bf16 table) without bias_table"),
    (dict(window_map=256, num_windows_dev=256), 0, "window_map"), (dict(num_windows_dev=256), 0, "num_windows_dev"), (dict(dbias=256), 0, "dbias"),
    (dict(), 1, "dtype must be 0"), (dict(), 2, "dtype must be 0"), (dict(), 3, "dtype must be 0"), (dict(), 8, "dtype must be 0"),
    (dict(tokens_per_window=288), 0, "window_size^2 != tokens_per_window"), (dict(map_h=35), 0, "map not divisible"), (dict(map_w=0), 0, "map not divisible"),
    (dict(num_windows=3), 0, "window count"),
    (dict(tokens_per_window=0), 0, "token count"), (dict(num_heads=0), 0, "token count"), (dict(qkv=None), 0, "null qkv"), (dict(out=None), 0, "bad out"),
    (dict(ld=194), 0, "multiples of 4"), (dict(k_off=34), 0, "multiples of 4"), (dict(head_stride=98), 0, "multiples of 4"),
    (dict(ldo=66), 0, "bad out"), (dict(ldo=32), 0, "bad out"), (dict(qkv=264), 0, "16-byte aligned"), (dict(out=520), 0, "bad out"),
    (dict(lse=258), 0, "lse must be 4-byte aligned"), (dict(bias_table=1026), 0, "bias_table must be 4-byte aligned"),
]


@pytest.mark.parametrize("over,dtype,msg", REFUSALS)
def test_refusals_answer_on_the_host_by_name(L, over, dtype, msg):
    """Argument validation precedes the launch: every refusal answers without a device, names the entry point and what it refuses."""
    lib = L.lib()
    before = lib.gg_attention_flash16_win_calls()
    assert lib.gg_attention_flash16_win_fwd(C.byref(_args(L, **over)), dtype, None) != 0
    err = lib.gg_last_error().decode()
    assert err.startswith(WHO + ":") and msg in err, err
    assert lib.gg_attention_flash16_win_calls() == before
    assert lib.gg_attention_flash16_win_fwd(None, 0, None) != 0 and "null" in lib.gg_last_error().decode()


def test_the_linear_entry_point_keeps_refusing_windows(L):
    """gg_attention_flash16_fwd is not widened: head dim 32, a window geometry and a bias table stay refused there."""
    lib = L.lib()
    for over, msg in ((dict(), "head_dim must be 64"), (dict(head_dim=64), "window_size must be 0"), (dict(head_dim=64, window_size=0), "bias_table")):
        assert lib.gg_attention_flash16_fwd(C.byref(_args(L, **over)), 0, None) != 0
        assert msg in lib.gg_last_error().decode()


@pytest.mark.parametrize("ws", [s[0] for s in A.SIZES])
def test_tiled_contract_meets_the_gpu_gates(ws):
    """The restated contract (64-key tiles, the bias in the running maximum, P rounded per tile) against attention_cases.gates on every case of the GPU file."""
    worst = 0.0
    for w, cls in A.params():
        if w != ws:
            continue
        c = A.get_case(w, cls)
        assert c["table"] is not None and c["kw"]["map_h"] == A.GEOM[ws][0] * ws
        got = A.tiled_contract(c)
        bad = AC.check(c, got, f"contract ws={ws}", tensors=("out", "lse"))
        assert not bad, bad
        e, g = AC.errors(c, got), AC.gates(c)
        worst = max([worst] + [e[t][x] / g[t][x] for t in ("out", "lse") for x in ("all", "rows") if e[t][x] is not None])
    print(f"\n[contract ws={ws}] worst error / gate {worst:.2f}")
    assert worst <= 1.0


def test_case_table_is_the_issues():
    assert len(A.params()) == 49
    assert [c for w, c in A.params() if w == 1] == ["plain"] and "bias_spike" in [c for w, c in A.params() if w == 32]
    assert A.SIZES == ((1, 1, 2), (4, 1, 2), (5, 2, 4), (8, 2, 8), (9, 1, 2), (16, 1, 2), (17, 2, 4), (24, 1, 2), (32, 1, 2))


def test_exact_inputs_are_exact_in_the_contract():
    """The inputs of the GPU file's exact tests do what they are meant to in the contract's f32 arithmetic: the mask table gives every P as exactly 1 or 0 (out the
    mean over the kept keys up to the output rounding, lse the log of their number); scale 0 with a zero table gives the column mean; the one-hot rows have a
    margin at which every other key's P underflows to zero, so the contract returns the selected v row exactly."""
    for ws in (5, 17):
        q, k, v, table, mean, count = A.mask_case(ws, 2)
        assert float(count.min()) >= 1 and float(count.max()) > 1
        c = dict(dtype=AC.BF16, q=q, k=k, v=v, scale=HD_SCALE, table=table, bidx=AC.bias_idxs(ws))
        got = A.tiled_contract(c)
        assert bool(((got["out"] - mean).abs() <= A.half_ulp(mean)).all())
        assert float((got["lse"] - torch.log(count)[None]).abs().max()) <= 1e-6
    for ws in (9, 17):
        N = ws * ws
        q, k, v = A.integer_case(ws, 2)
        got = A.tiled_contract(dict(dtype=AC.BF16, q=q, k=k, v=v, scale=0.0, table=torch.zeros(2, N), bidx=AC.bias_idxs(ws)))
        mean = v.mean(-2, keepdim=True).expand_as(v)
        assert bool(((got["out"] - mean).abs() <= A.half_ulp(mean)).all())
        assert float((got["lse"] - math.log(N)).abs().max()) <= 1e-6
    for ws in (9, 17, 32):
        q, k, v, sel, margin = A.one_hot_case(ws)
        assert margin >= 4 and margin * A.ONE_HOT_SCALE * A.LOG2E >= 150, (ws, margin)
        c = dict(dtype=AC.BF16, q=q, k=k, v=v, scale=A.ONE_HOT_SCALE, table=torch.zeros(2, ws * ws), bidx=AC.bias_idxs(ws))
        assert torch.equal(A.tiled_contract(c)["out"], v[:, :, sel])


HD_SCALE = A.HD ** -0.5
