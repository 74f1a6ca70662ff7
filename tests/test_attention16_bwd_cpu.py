"""CPU-only checks of the long-sequence 16-bit-MFMA attention backward (include/gg_attn16b.h): the header against the binding, the ``attention16_train`` keyword
and its refusals, the entry point's refusals (they answer on the host, before any launch), and the arithmetic contract restated in torch
(tests/attention16_bwd_cases.py) against the gates tests/test_gpu_attention16_bwd.py holds the kernel to -- which pins those gates to something a correct
kernel can meet -- and against the closed forms of the two exact families, bit for bit.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attention16_bwd_cases as B
from tests import attention16_cases as A
from tests import attention_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gg_attention_flash16_bwd", "gg_attention_flash16_bwd_calls", "gg_clip_set_attention16_train"}


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_attn16b_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_attn16b.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.ATTN16B_SYMBOLS) == SYMBOLS
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(L.ATTN16B_SIGNATURES[n][1]), n
    assert L.ATTN16B_SIGNATURES["gg_attention_flash16_bwd_calls"][0] is C.c_int64
    assert "gg_attn16b.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "attention_flash16_bwd.hip" in mk.split("SRCS")[1].split("\n")[0]
    assert "gg_attn16b.h" in mk.split("attention_flash16_bwd.hip.o ../lib/obj/clip.hip.o:")[1].split("\n")[0]
    for other in ("gg.h", "gg_attn16.h", "gg_attn16w.h"):          # the new prototypes live in the new header only
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not (declared & set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", text))), other


def test_switch_defaults_off_and_returns_the_previous_value(L):
    lib = L.lib()
    n, nf = lib.gg_attention_flash16_bwd_calls(), lib.gg_attention_flash16_calls()
    s = lib.gg_clip_set_attention16_train
    assert s(1) == 0 and s(5) == 1 and s(0) == 1 and s(0) == 0
    assert lib.gg_clip_set_attention16(1) == 0 and s(0) == 0 and lib.gg_clip_set_attention16(0) == 1 and s(0) == 0      # two switches, independent
    assert lib.gg_attention_flash16_bwd_calls() == n and lib.gg_attention_flash16_calls() == nf                        # a switch flip launches nothing


def test_keyword_and_its_refusals(L):
    from geoguessr_ai_amd.pretrain import clip_embedder as E
    name = "openai/clip-vit-base-patch32"
    tower = E.CLIPVisionTower(name, precision="bf16", num_layers=1, attention16_train=True)
    assert tower.attention16_train is True and tower.vision_model.attention16_train is True and tower.attention16 is False
    both = E.CLIPVisionTower(name, precision="bf16", num_layers=1, attention16_train=True, attention16=True)
    assert both.attention16_train is True and both.attention16 is True
    plain = E.CLIPVisionTower(name, precision="bf16", num_layers=1, attention16=True)
    assert plain.attention16_train is False and plain.vision_model.attention16_train is False
    for precision in ("fp32", "fp32_split", "fp16", "fp8"):
        with pytest.raises(L.GgError, match=rf"CLIPVisionTower: attention16_train=True .*precision='{precision}'"):
            E.CLIPVisionTower(name, precision=precision, num_layers=1, attention16_train=True)
        assert E.CLIPVisionTower(name, precision=precision, num_layers=1, attention16_train=False).attention16_train is False
    assert "GG_ATTENTION16" not in open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "clip.hip")).read()      # no environment variable


def _args(L, **over):
    a = L.AttnArgs()
    a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = 256, 384, 0, 128, 256, 64, 64
    a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = 2, 1, 300, 0, 0.125
    a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = 512, 128, 768, 1024, 128, 1280
    for k, v in over.items():
        setattr(a, k, v)
    return a


# (overrides of a valid call, dtype, what the message names)
REFUSALS = [
    (dict(), 2, "fp16 storage is inference-only"), (dict(), 1, "dtype must be 0"), (dict(), 3, "dtype must be 0"),
    (dict(head_dim=32), 0, "head_dim must be 64"), (dict(window_size=10, map_h=10, map_w=10, tokens_per_window=100), 0, "window_size must be 0"),
    (dict(bias=256), 0, "bias "), (dict(bias_table=256), 0, "bias_table"), (dict(dbias=256), 0, "dbias"),
    (dict(window_map=256, num_windows_dev=256), 0, "window_map"), (dict(num_windows_dev=256), 0, "num_windows_dev"),
    (dict(lse=None), 0, "lse"), (dict(out=None), 0, "out"), (dict(dout=None), 0, "dout"), (dict(dqkv=None), 0, "dqkv"),
    (dict(tokens_per_window=0), 0, "token count"), (dict(num_heads=0), 0, "token count"), (dict(qkv=None), 0, "null qkv"),
    (dict(ld=386), 0, "multiples of 4"), (dict(k_off=130), 0, "multiples of 4"), (dict(ldo=130), 0, "bad out"), (dict(lddo=64), 0, "bad dout"),
    (dict(qkv=264), 0, "16-byte aligned"), (dict(dqkv=1288), 0, "16-byte aligned"), (dict(dout=1032), 0, "bad dout"),
]


@pytest.mark.parametrize("over,dtype,msg", REFUSALS)
def test_refusals_answer_on_the_host_by_name(L, over, dtype, msg):
    """Argument validation precedes the launch: every refusal answers without a device, names the entry point and what it refuses; the counter does not move."""
    lib = L.lib()
    before = lib.gg_attention_flash16_bwd_calls()
    assert lib.gg_attention_flash16_bwd(C.byref(_args(L, **over)), dtype, None) != 0
    err = lib.gg_last_error().decode()
    assert err.startswith("gg_attention_flash16_bwd:") and msg in err, err
    assert lib.gg_attention_flash16_bwd_calls() == before
    assert lib.gg_attention_flash16_bwd(None, 0, None) != 0 and "null" in lib.gg_last_error().decode()


@pytest.mark.parametrize("N", B.SIZES)
def test_tiled_contract_meets_the_gpu_gates(N):
    """The restated contract (per 64-key tile, P from lse, P and dS rounded as operands) against attention_cases.gates on every case of the GPU file; its out and
    lse are the restated forward's (attention16_cases.tiled_contract)."""
    worst = 0.0
    for n, cls in B.params():
        if n != N:
            continue
        c = B.get_case(n, cls)
        fwd = A.tiled_contract(c)
        got = B.tiled_contract_bwd(c, fwd["out"], fwd["lse"])
        bad = B.check(c, got, f"bwd contract N={n}")
        assert not bad, bad
        e, g = AC.errors(c, got), AC.gates(c)
        worst = max([worst] + [e[t][w] / g[t][w] for t in (("dq", "dk", "dv") if n > 1 else ("dv",)) for w in ("all", "rows") if e[t][w] is not None])
    print(f"\n[bwd contract N={N}] worst error / gate {worst:.2f}")
    assert worst <= 1.0


@pytest.mark.parametrize("N", B.ONE_HOT_SIZES)
def test_one_hot_rows_are_exact_in_the_contract(N):
    c = B.one_hot_bwd_case(N)
    assert c["margin"] >= 13, (N, c["margin"])            # 13 * 8 * log2 e = 150 > 149: exp2 of the difference is 0 in f32
    assert all(B.is_bf16(t) for t in c["want"].values()) and B.is_bf16(c["dout_c"]) and B.is_bf16(c["v"])
    fwd = A.tiled_contract(c)
    assert torch.equal(fwd["out"], c["out"])
    got = B.tiled_contract_bwd(c, fwd["out"], fwd["lse"])
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], c["want"][n]), n


@pytest.mark.parametrize("N", B.TWO_HOT_SIZES)
def test_two_hot_rows_are_exact_in_the_contract(N):
    c = B.two_hot_case(N)
    assert all(B.is_bf16(t) for t in c["want"].values()) and B.is_bf16(c["out"]) and B.is_bf16(c["q"])
    assert float(c["want"]["dq"].abs().max()) <= 64 and float(c["want"]["dk"].abs().max()) <= 128
    fwd = A.tiled_contract(c)
    assert torch.equal(fwd["out"], c["out"])
    print(f"\n[two-hot N={N}] restated lse off by {float((fwd['lse'] - c['lse']).abs().max()):.1e}")
    assert float((fwd["lse"] - c["lse"]).abs().max()) <= 2e-4
    got = B.tiled_contract_bwd(c, fwd["out"], fwd["lse"])
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], c["want"][n]), n
