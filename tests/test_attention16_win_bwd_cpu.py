"""CPU-only checks of the 16-bit-MFMA window attention backward (include/gg_attn16wb.h): the arithmetic contract restated in torch
(tests/attention16_win_bwd_cases.py) against the gates tests/test_gpu_attention16_win_bwd.py holds the kernel to -- which pins those gates to something a correct
kernel can meet -- and against the closed forms of the two exact families, bit for bit (C1); the ``attention16_train`` keyword of the TinyViT classes and its
refusals (C2); the header against the binding (C3); the entry point's refusals, which answer on the host before any launch.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attention16_cases as A
from tests import attention16_win_bwd_cases as WB
from tests import attention_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gg_attention_flash16_win_bwd", "gg_attention_flash16_win_bwd_calls", "gg_attention_flash16_win_dbias_rows", "gg_tinyvit_set_attention16_train"}


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


# ------------------------------------------------------------------------------------------- C1: the restated contract
@pytest.mark.parametrize("ws", [s[0] for s in WB.SIZES])
def test_tiled_contract_meets_the_gpu_gates(ws):
    """The restated contract (per 64-key tile, P from lse with the bias inside, P and dS rounded as operands, dbias from the unrounded dS) against the gates of the
    GPU file on every conditioning case; its out and lse are the restated forward's (attention16_cases.tiled_contract)."""
    worst = 0.0
    for w, cls in WB.params():
        if w != ws:
            continue
        c = WB.get_case(w, cls)
        fwd = A.tiled_contract(c)
        got = WB.tiled_contract_bwd(c, fwd["out"], fwd["lse"])
        bad = WB.check(c, got, f"win bwd contract ws={w}")
        assert not bad, bad
        if w > 1:
            e, g = AC.errors(c, got), AC.gates(c)
            worst = max([worst] + [e[t][k] / g[t][k] for t in WB.TENSORS for k in ("all", "rows") if e[t][k] is not None])
    print(f"\n[win bwd contract ws={ws}] worst error / gate {worst:.2f}")
    assert worst <= 1.0


@pytest.mark.parametrize("ws", WB.ONE_HOT_SIZES)
def test_one_hot_rows_are_exact_in_the_contract(ws):
    c = WB.one_hot_bwd_case(ws)
    assert all(WB.B.is_bf16(t) for t in c["want"].values()) and WB.B.is_bf16(c["dout_c"]) and WB.B.is_bf16(c["v"])
    fwd = A.tiled_contract(c)
    assert torch.equal(fwd["out"], c["out"])
    got = WB.tiled_contract_bwd(c, fwd["out"], fwd["lse"])
    for n in WB.TENSORS:
        assert torch.equal(got[n], c["want"][n]), n


def test_two_hot_rows_are_exact_in_the_contract():
    c = WB.two_hot_case()
    fwd = A.tiled_contract(c)
    assert torch.equal(fwd["out"], c["out"])                                    # the restated forward agrees with the closed form of out
    assert float((fwd["lse"] - c["lse"]).abs().max()) <= 2e-4
    lse = torch.full(c["q"].shape[:-1], c["lse"], dtype=torch.float64)
    got = WB.tiled_contract_bwd(c, c["out"], lse)
    for n in WB.TENSORS:
        assert torch.equal(got[n], c["want"][n]), (n, float((got[n] - c["want"][n]).abs().max()))
    assert float(c["want"]["dbias"].abs().max()) > 0                            # (the family does exercise the bins)


# ------------------------------------------------------------------------------------------- C2: the keyword
def test_keyword_and_its_refusals(L):
    from geoguessr_ai_amd.models.tinyvit import TinyVitBackbone, TinyViTAdapter, check_attention16_train
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    name = "tiny_vit_5m_224"
    makers = {"TinyVitBackbone": lambda **kw: TinyVitBackbone(name, seed=0, **kw),
              "TinyViTAdapter": lambda **kw: TinyViTAdapter(name, pretrained=False, seed=0, **kw),
              "TinyViTClassifier": lambda **kw: TinyViTClassifier(name, num_classes=3, seed=0, **kw)}
    for who, make in makers.items():
        for precision in ("fp32", "fp32_split"):
            with pytest.raises(L.GgError, match=rf"{who}: attention16_train=True .*precision='{precision}'.*attention16_train"):
                make(precision=precision, attention16_train=True)
        mod = make(precision="bf16", attention16_train=True)
        bb = mod if who == "TinyVitBackbone" else mod.backbone
        assert bb.attention16_train is True and bb.attention16 is False          # independent of attention16
        both = make(precision="bf16", attention16_train=True, attention16=True)
        bb = both if who == "TinyVitBackbone" else both.backbone
        assert bb.attention16_train is True and bb.attention16 is True
        off = make(precision="bf16")
        assert (off if who == "TinyVitBackbone" else off.backbone).attention16_train is False
    check_attention16_train(False, "fp32", "x")                                  # off: any precision
    assert "GG_ATTENTION16" not in open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "tinyvit.hip")).read()      # no environment variable


def test_switch_defaults_off_and_returns_the_previous_value(L):
    lib = L.lib()
    n = (lib.gg_attention_flash16_win_bwd_calls(), lib.gg_attention_flash16_win_calls())
    s = lib.gg_tinyvit_set_attention16_train
    assert s(1) == 0 and s(5) == 1 and s(0) == 1 and s(0) == 0
    assert lib.gg_tinyvit_set_attention16(1) == 0 and s(0) == 0 and lib.gg_tinyvit_set_attention16(0) == 1 and s(0) == 0      # two switches, independent
    assert lib.gg_clip_set_attention16_train(1) == 0 and s(0) == 0 and lib.gg_clip_set_attention16_train(0) == 1              # TinyViT's is not CLIP's
    assert (lib.gg_attention_flash16_win_bwd_calls(), lib.gg_attention_flash16_win_calls()) == n                              # a switch flip launches nothing


# ------------------------------------------------------------------------------------------- C3: the header against the binding
def test_attn16wb_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_attn16wb.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.ATTN16WB_SYMBOLS) == SYMBOLS
    assert not (declared & set(L.SYMBOLS))                                       # the extension table, not SYMBOLS
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(L.ATTN16WB_SIGNATURES[n][1]), n
    assert L.ATTN16WB_SIGNATURES["gg_attention_flash16_win_bwd_calls"][0] is C.c_int64
    assert L.ATTN16WB_SIGNATURES["gg_attention_flash16_win_dbias_rows"][0] is C.c_int64
    assert "gg_attn16wb.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "gg_attn16wb.h" in mk.split("attention_flash16_bwd.hip.o ../lib/obj/tinyvit.hip.o:")[1].split("\n")[0]
    for other in ("gg.h", "gg_attn16.h", "gg_attn16w.h", "gg_attn16b.h"):         # the new prototypes live in the new header only
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not (declared & set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", text))), other


def test_dbias_rows_is_the_workgroup_count_plus_the_fold_rows(L):
    rows = L.lib().gg_attention_flash16_win_dbias_rows
    assert rows(64, 1024) == 64 * 8 + 64 and rows(64, 576) == 64 * 5 + 64 and rows(2, 1) == 2 + 64 and rows(4, 289) == 4 * 3 + 64


# ------------------------------------------------------------------------------------------- refusals (K7's list, on the host)
def _args(L, **over):
    a = L.AttnArgs()
    a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = 256, 192, 0, 32, 64, 96, 32
    a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = 2, 4, 289, 17, 34, 34, 0.125
    a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = 512, 64, 768, 1024, 64, 1280
    for k, v in over.items():
        setattr(a, k, v)
    return a


# (overrides of a valid call, dtype, what the message names)
REFUSALS = [
    (dict(), 2, "fp16 storage is inference-only"), (dict(), 1, "dtype must be 0"), (dict(), 3, "dtype must be 0"),
    (dict(head_dim=64), 0, "head_dim must be 32"), (dict(window_size=0), 0, "window_size must be 1 .. 32"),
    (dict(window_size=33, map_h=33, map_w=33, tokens_per_window=1089, num_windows=1), 0, "window_size must be 1 .. 32"),
    (dict(bias=256), 0, "bias (the expanded bf16 table) without bias_table"), (dict(dbias=256), 0, "dbias without bias_table"),
    (dict(window_map=256, num_windows_dev=256), 0, "window_map"), (dict(num_windows_dev=256), 0, "num_windows_dev"),
    (dict(lse=None), 0, "lse"), (dict(out=None), 0, "out"), (dict(dout=None), 0, "dout"), (dict(dqkv=None), 0, "dqkv"),
    (dict(tokens_per_window=0), 0, "token count"), (dict(num_heads=0), 0, "token count"), (dict(qkv=None), 0, "null qkv"),
    (dict(tokens_per_window=288), 0, "window_size^2"), (dict(map_w=35), 0, "map not divisible"), (dict(num_windows=3), 0, "window count"),
    (dict(ld=194), 0, "multiples of 4"), (dict(k_off=34), 0, "multiples of 4"), (dict(ldo=66), 0, "bad out"), (dict(lddo=32), 0, "bad dout"),
    (dict(qkv=264), 0, "16-byte aligned"), (dict(dqkv=1288), 0, "16-byte aligned"), (dict(dout=1032), 0, "bad dout"), (dict(out=520), 0, "bad out"),
    (dict(lse=770), 0, "lse must be 4-byte aligned"), (dict(bias_table=258), 0, "bias_table must be 4-byte aligned"),
]


@pytest.mark.parametrize("over,dtype,msg", REFUSALS)
def test_refusals_answer_on_the_host_by_name(L, over, dtype, msg):
    """Argument validation precedes the launch: every refusal answers without a device, names the entry point and what it refuses; the counter does not move."""
    lib = L.lib()
    before = lib.gg_attention_flash16_win_bwd_calls()
    assert lib.gg_attention_flash16_win_bwd(C.byref(_args(L, **over)), dtype, None) != 0
    err = lib.gg_last_error().decode()
    assert err.startswith("gg_attention_flash16_win_bwd:") and msg in err, err
    assert lib.gg_attention_flash16_win_bwd_calls() == before
    assert lib.gg_attention_flash16_win_bwd(None, 0, None) != 0 and "null" in lib.gg_last_error().decode()
