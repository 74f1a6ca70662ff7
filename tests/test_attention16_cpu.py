"""CPU-only checks of the long-sequence 16-bit-MFMA attention forward (include/gg_attn16.h): the header against the binding, the ``attention16`` keyword and its
refusals, the entry point's refusals (they answer on the host, before any launch), and the arithmetic contract restated in torch (tests/attention16_cases.py) against
the gates tests/test_gpu_attention16.py holds the kernel to -- which pins those gates to something a correct kernel can meet.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attention16_cases as A
from tests import attention_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_attn16_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_attn16.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.ATTN16_SYMBOLS) == {"gg_attention_flash16_fwd", "gg_attention_flash16_calls", "gg_clip_set_attention16"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(L.ATTN16_SIGNATURES[n][1]), n
    assert L.ATTN16_SIGNATURES["gg_attention_flash16_calls"][0] is C.c_int64
    assert "gg_attn16.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "attention_flash16.hip" in mk.split("SRCS")[1].split("\n")[0]
    assert "gg_attn16.h" in mk.split("attention_flash16.hip.o ../lib/obj/clip.hip.o:")[1].split("\n")[0]
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg.h")).read(), flags=re.S)
    assert not (declared & set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", main)))


def test_switch_defaults_off_and_returns_the_previous_value(L):
    lib = L.lib()
    n = lib.gg_attention_flash16_calls()
    assert lib.gg_clip_set_attention16(1) == 0 and lib.gg_clip_set_attention16(5) == 1 and lib.gg_clip_set_attention16(0) == 1 and lib.gg_clip_set_attention16(0) == 0
    assert lib.gg_attention_flash16_calls() == n          # a switch flip launches nothing


def test_keyword_and_its_refusals(L):
    from geoguessr_ai_amd.pretrain import clip_embedder as E
    assert E.tower_precision_code("bf16") == 0 and E.tower_precision_code("fp16") == 2 and E.tower_precision_code("fp8") == 8
    assert E.tower_precision_code("fp32") == 1 and E.tower_precision_code("fp32_split") == 3
    for precision in ("bf16", "fp16", "fp8"):
        tower = E.CLIPVisionTower("openai/clip-vit-base-patch32", precision=precision, num_layers=1, attention16=True)
        assert tower.attention16 is True and tower.vision_model.attention16 is True and tower.precision == precision
    assert E.CLIPVisionTower("openai/clip-vit-base-patch32", precision="bf16", num_layers=1).attention16 is False
    for precision in ("fp32", "fp32_split"):
        with pytest.raises(L.GgError, match=rf"CLIPVisionTower: attention16=True .*precision='{precision}'"):
            E.CLIPVisionTower("openai/clip-vit-base-patch32", precision=precision, num_layers=1, attention16=True)
        with pytest.raises(L.GgError, match=rf"CLIPEmbedding: attention16=True .*precision='{precision}'"):
            E.CLIPEmbedding("openai/clip-vit-base-patch32", device="cpu", precision=precision, num_layers=1, attention16=True)
        E.CLIPVisionTower("openai/clip-vit-base-patch32", precision=precision, num_layers=1, attention16=False)
    assert "GG_ATTENTION16" not in open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "clip.hip")).read()      # no environment variable


def _args(L, **over):
    a = L.AttnArgs()
    a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = 256, 384, 0, 128, 256, 64, 64
    a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = 2, 1, 300, 0, 0.125
    a.out, a.ldo = 512, 128
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(head_dim=32), 2, "head_dim must be 64"), (dict(window_size=10, map_h=10, map_w=10, tokens_per_window=100), 2, "window_size must be 0"),
    (dict(bias=256), 0, "bias "), (dict(bias_table=256), 0, "bias_table"), (dict(window_map=256, num_windows_dev=256), 2, "window_map"),
    (dict(num_windows_dev=256), 2, "num_windows_dev"), (dict(), 1, "dtype must be 0"), (dict(), 3, "dtype must be 0"), (dict(), 8, "dtype must be 0"),
    (dict(tokens_per_window=0), 2, "token count"), (dict(num_heads=0), 0, "token count"), (dict(qkv=None), 2, "null qkv"), (dict(out=None), 2, "bad out"),
    (dict(ld=386), 2, "multiples of 4"), (dict(k_off=130), 0, "multiples of 4"), (dict(ldo=130), 2, "bad out"), (dict(ldo=64), 2, "bad out"),
    (dict(qkv=264), 2, "16-byte aligned"), (dict(out=520), 0, "bad out"),
]


@pytest.mark.parametrize("over,dtype,msg", REFUSALS)
def test_refusals_answer_on_the_host_by_name(L, over, dtype, msg):
    """Argument validation precedes the launch: every refusal answers without a device, names the entry point and what it refuses."""
    lib = L.lib()
    before = lib.gg_attention_flash16_calls()
    assert lib.gg_attention_flash16_fwd(C.byref(_args(L, **over)), dtype, None) != 0
    err = lib.gg_last_error().decode()
    assert err.startswith("gg_attention_flash16_fwd:") and msg in err, err
    assert lib.gg_attention_flash16_calls() == before
    assert lib.gg_attention_flash16_fwd(None, 2, None) != 0 and "null" in lib.gg_last_error().decode()


@pytest.mark.parametrize("storage", A.STORAGES)
@pytest.mark.parametrize("N", A.SIZES)
def test_tiled_contract_meets_the_gpu_gates(storage, N):
    """The restated contract (64-key tiles, running maximum, P rounded per tile) against attention_cases.gates on every case of the GPU file."""
    worst = 0.0
    for s, n, cls in A.params():
        if (s, n) != (storage, N):
            continue
        c = A.get_case(s, n, cls)
        got = A.tiled_contract(c)
        bad = AC.check(c, got, f"contract {s} N={n}", tensors=("out", "lse"))
        assert not bad, bad
        e, g = AC.errors(c, got), AC.gates(c)
        worst = max([worst] + [e[t][w] / g[t][w] for t in ("out", "lse") for w in ("all", "rows") if e[t][w] is not None])
    print(f"\n[contract {storage} N={N}] worst error / gate {worst:.2f}")
    assert worst <= 1.0


def test_integer_and_one_hot_inputs_are_exact_in_the_contract():
    """The inputs of the GPU file's integer tests do what they are meant to in the contract's f32 arithmetic: the one-hot rows have a margin at which every other
    key's P underflows to zero, so the restated contract returns the selected v row exactly; with scale 0 it returns the column mean up to the output rounding."""
    for N in (17, 65, 577):
        q, k, v, sel, margin = A.one_hot_case(N)
        assert margin >= 16, (N, margin)                  # 16 * 8 * log2 e = 184 > 149: exp2 of the difference is 0 in f32
        for st in (AC.F16, AC.BF16):
            c = dict(dtype=st, q=q, k=k, v=v, scale=8.0)
            assert torch.equal(A.tiled_contract(c)["out"], v[:, :, sel])
            q0, k0, v0 = A.integer_case(N, st)
            got = A.tiled_contract(dict(dtype=st, q=q0, k=k0, v=v0, scale=0.0))
            mean = v0.mean(-2, keepdim=True).expand_as(v0)
            assert bool(((got["out"] - mean).abs() <= A.half_ulp(mean, st)).all())
            assert float((got["lse"] - torch.log(torch.tensor(float(N), dtype=torch.float64))).abs().max()) <= 1e-6
