"""CPU-only checks of the fixed-order bias gradient (include/gg_attn_dbias.h): the header against the binding, with a case per prototype (C1); the scratch rows
against what the shapes of the GPU tests and TinyViT's planner reserve (C2); every refusal by its message, answered on the host before any launch (C3); the
process-wide switch (C4); the ``deterministic_bias_grad`` keyword of the three TinyViT classes (C5); and the numpy restatement of the bin walk -- which (q, k)
pairs fall in which bin, in which order -- on an integer-valued dS, where every order of adds gives the same sum exactly (C6).  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import attention_cases as AC
from tests import attention_dbias_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# prototype -> the test of this file that calls it
CASES = {
    "gg_attention_dbias_rows": "test_rows_match_the_shapes_and_the_planner",
    "gg_attention_dbias": "test_every_refusal_by_its_message",
    "gg_attention_dbias_calls": "test_every_refusal_by_its_message",
    "gg_tinyvit_set_deterministic_dbias": "test_switch_defaults_off_and_returns_the_previous_value",
}


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _args(L, ws=7, heads=2, windows=4, map_h=14, map_w=7, es=2):
    """Arguments the entry point accepts, with placeholder pointers (refusals answer before anything is dereferenced or launched)."""
    a = L.AttnArgs()
    a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = 3 * heads * 32, 0, 32, 64, 96, 32
    a.num_heads, a.num_windows, a.tokens_per_window = heads, windows, ws * ws
    a.window_size, a.map_h, a.map_w, a.scale = ws, map_h, map_w, 32 ** -0.5
    a.ldo = a.lddo = heads * 32
    for f in ("qkv", "out", "dout", "lse", "bias_table", "dbias", "dbias_scratch"):
        setattr(a, f, 4096)
    return a


# ------------------------------------------------------------------------------------------- C1
def test_header_symbols_match_the_binding_and_every_prototype_has_a_case(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_attn_dbias.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.ATTN_DBIAS_SYMBOLS) == set(CASES)
    assert not (declared & set(L.SYMBOLS))                                       # the extension table, not SYMBOLS
    lib, src = L.lib(), open(__file__).read()
    for n, test in CASES.items():
        assert hasattr(lib, n), n
        body = src[src.index(f"def {test}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        assert re.search(r"\b" + n + r"\b", body), (n, test)
    # the header is included from nowhere but its two users; the route decision gains nothing
    for f in os.listdir(os.path.join(ROOT, "include")):
        if f != "gg_attn_dbias.h":
            assert not re.search(r'#\s*include\s*[<"][^>"]*gg_attn_dbias\.h', open(os.path.join(ROOT, "include", f)).read()), f
    assert "dbias.h" not in open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "attention_route.h")).read()
    assert L.PROF_CAT_ATTN_DBIAS == 8 and "GG_CAT_ATTN_DBIAS = 8" in open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "prof.h")).read()


# ------------------------------------------------------------------------------------------- C2
def test_rows_match_the_shapes_and_the_planner(L):
    lib = L.lib()
    for name, (ws, heads, windows, map_h, map_w) in DC.SHAPES.items():
        for dtype in (0, 1, 3):
            a = _args(L, ws, heads, windows, map_h, map_w)
            assert lib.gg_attention_dbias_rows(C.byref(a), dtype) == DC.rows(windows) == windows + 64, name
    # more windows than groups; the geometry alone decides: no pointer is looked at
    a = _args(L, 7, 4, 1024 * 16, 28, 28)
    for f in ("qkv", "out", "dout", "lse", "bias_table", "dbias", "dbias_scratch"):
        setattr(a, f, None)
    assert lib.gg_attention_dbias_rows(C.byref(a), 1) == 512 + 64 == DC.rows(1024 * 16)
    # what gg_tinyvit_backward reserves for them: the 128 MiB split-K region of its workspace holds the rows of every stage of every variant at any batch
    from geoguessr_ai_amd.models.tinyvit import VARIANTS
    for name, v in VARIANTS.items():
        for dim, heads_, ws in zip(v["embed_dims"][1:], v["num_heads"][1:], v["window_sizes"][1:]):
            assert dim // heads_ == 32
            assert DC.rows(1 << 20) * heads_ * ws * ws * 4 <= 128 << 20, (name, ws)
    assert lib.gg_attention_dbias_rows(None, 0) < 0 and b"null args" in lib.gg_last_error()


# ------------------------------------------------------------------------------------------- C3
REFUSALS = [
    (dict(dtype=2), "fp16 storage is inference-only"),
    (dict(dtype=4), r"dtype must be 0 \(bf16 storage\), 1 or 3 \(f32 storage\); got 4"),
    (dict(head_dim=64), r"head_dim must be 32 \(got 64\)"),
    (dict(window_size=0), r"window_size must be 1 \.\. 32 \(got 0: without a window geometry"),
    (dict(window_size=33, tokens_per_window=33 * 33, map_h=33, map_w=33, num_windows=1), r"window_size must be 1 \.\. 32 \(got 33\)"),
    (dict(window_map=4096), "window_map / num_windows_dev"),
    (dict(num_windows_dev=4096), "window_map / num_windows_dev"),
    (dict(tokens_per_window=50), r"window_size\^2 != tokens_per_window"),
    (dict(map_w=8), "map not divisible by window"),
    (dict(num_windows=3), "window count"),
    (dict(qkv=None), "missing qkv"), (dict(lse=None), "missing lse"), (dict(out=None), "missing out"), (dict(dout=None), "missing dout"),
    (dict(bias_table=None), "missing bias_table"), (dict(dbias=None), "missing dbias"), (dict(dbias_scratch=None), "missing dbias_scratch"),
    (dict(qkv=4096 + 8), "qkv, out and dout must be 16-byte aligned"), (dict(out=4096 + 2), "16-byte aligned"), (dict(dout=4096 + 4), "16-byte aligned"),
    (dict(ld=3 * 64 + 4), r"multiples of 8 elements \(16 bytes\)"), (dict(dtype=1, ld=3 * 64 + 2), r"multiples of 4 elements \(16 bytes\)"),
    (dict(q_off=4), "multiples of 8 elements"), (dict(dtype=3, head_stride=98), "multiples of 4 elements"),
    (dict(lse=4096 + 2), "lse, bias_table, dbias and dbias_scratch must be 4-byte aligned"), (dict(dbias=4096 + 1), "4-byte aligned"),
    (dict(dbias_scratch=4096 + 2), "4-byte aligned"), (dict(bias_table=4096 + 3), "4-byte aligned"),
]


def test_every_refusal_by_its_message(L):
    """Each refusal answers on the host, by name, before any launch: the call counter does not move (and without a GPU nothing could have been written)."""
    lib = L.lib()
    n0 = lib.gg_attention_dbias_calls()
    for change, msg in REFUSALS:
        a = _args(L)
        dtype = change.pop("dtype", 0) if "dtype" in change else 0
        for k, v in change.items():
            setattr(a, k, v)
        assert lib.gg_attention_dbias(C.byref(a), dtype, 0, None) == -1, change
        err = lib.gg_last_error().decode()
        assert err.startswith("gg_attention_dbias: ") and re.search(msg, err), (change, err)
        change["dtype"] = dtype
    assert lib.gg_attention_dbias(None, 0, 0, None) == -1 and "null args" in lib.gg_last_error().decode()
    assert lib.gg_attention_dbias_calls() == n0


# ------------------------------------------------------------------------------------------- C4
def test_switch_defaults_off_and_returns_the_previous_value(L):
    lib = L.lib()
    s = lib.gg_tinyvit_set_deterministic_dbias
    assert s(1) == 0 and s(7) == 1 and s(0) == 1 and s(0) == 0
    t = lib.gg_tinyvit_set_attention16_train                                      # independent of the other switches
    assert t(1) == 0 and s(0) == 0 and s(1) == 0 and t(0) == 1 and s(0) == 1 and t(0) == 0
    assert "GG_DETERMINISTIC" not in open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "tinyvit.hip")).read()      # no environment variable


# ------------------------------------------------------------------------------------------- C5
def test_keyword_reaches_the_three_classes(L):
    from geoguessr_ai_amd.models.tinyvit import TinyVitBackbone, TinyViTAdapter
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    name = "tiny_vit_5m_224"
    makers = {"TinyVitBackbone": lambda **kw: TinyVitBackbone(name, seed=0, **kw),
              "TinyViTAdapter": lambda **kw: TinyViTAdapter(name, pretrained=False, seed=0, **kw),
              "TinyViTClassifier": lambda **kw: TinyViTClassifier(name, num_classes=3, seed=0, **kw)}
    inner = lambda who, mod: mod if who == "TinyVitBackbone" else mod.backbone
    for (who, make), precision in zip(makers.items(), ("fp32", "fp32_split", "bf16")):      # the keyword reaches every class; every precision takes it
        bb = inner(who, make(precision=precision, deterministic_bias_grad=True))
        assert bb.deterministic_bias_grad is True and bb.attention16_train is False, (who, precision)
        assert inner(who, make(precision=precision)).deterministic_bias_grad is False      # the default is not flipped
    for precision in ("fp32_split", "bf16"):
        assert TinyVitBackbone(name, seed=0, precision=precision, deterministic_bias_grad=True).deterministic_bias_grad is True
    both = makers["TinyViTAdapter"](precision="bf16", deterministic_bias_grad=True, attention16_train=True, grad_checkpointing=True, img_size=160)
    assert both.backbone.deterministic_bias_grad is True and both.backbone.attention16_train is True      # composes with the other switches
    assert L.lib().gg_tinyvit_set_deterministic_dbias(0) == 0                    # constructing a model flips nothing


# ------------------------------------------------------------------------------------------- C6
@pytest.mark.parametrize("ws,windows", [(3, 2), (7, 4), (12, 1), (14, 1), (17, 1), (32, 1), (2, 515)])
def test_bin_walk_sums_an_integer_valued_ds_exactly(ws, windows):
    """Every (query, key) pair of every window is visited exactly once, no two lanes of an instruction meet in one bin of one table, and the walk's sum of an
    integer-valued dS equals the gather-index sum exactly (515 windows of 2 x 2: more windows than window groups, so a group walks two)."""
    N = ws * ws
    ds = np.random.default_rng(ws).integers(-8, 9, size=(windows, N, N)).astype(np.float64)
    table, visits = DC.bin_walk(ds, ws)
    assert (visits == 1).all()
    want = np.zeros(N)
    np.add.at(want, AC.bias_idxs(ws).numpy().reshape(-1), ds.sum(0).reshape(-1))
    assert np.array_equal(table, want)
    assert DC.groups(windows) == min(windows, 512) and DC.rows(windows) == DC.groups(windows) + 64
