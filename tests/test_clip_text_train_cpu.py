"""CPU-only checks of the third header (include/gg_clip_text_train.h: training the CLIP text tower): every prototype exported and bound, the other two headers'
symbol sets untouched and disjoint, the training workspace's size rules and refusals, and the first trained layer under a handful of masks."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _protos(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _table(L, cfg):
    lib = L.lib()
    name = C.create_string_buffer(256)
    out = []
    for i in range(lib.gg_clip_text_num_tensors(C.byref(cfg))):
        L.check(lib.gg_clip_text_tensor_info(C.byref(cfg), i, name, 256, None, None, None, None), "gg_clip_text_tensor_info")
        out.append(name.value.decode())
    return out


def _mask(names, sel):
    return bytes(int(bool(sel(n))) for n in names)


def test_train_header_symbols_exported_and_bound(L):
    hdr = _protos("gg_clip_text_train.h")
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.TEXT_TRAIN_SYMBOLS) and len(declared) == 7
    lib = L.lib()
    for n in L.TEXT_TRAIN_SYMBOLS:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        args = m.group(1)
        cnt = 0 if args.strip() in ("void", "") else len(args.split(","))
        assert cnt == len(L.TEXT_TRAIN_SIGNATURES[n][1]), n


def test_the_other_two_symbol_sets_are_unchanged_and_disjoint(L):
    first = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", _protos("gg.h")))
    second = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", _protos("gg_clip_text.h")))
    assert first == set(L.SYMBOLS) and second == set(L.TEXT_SYMBOLS) and len(second) == 14
    third = set(L.TEXT_TRAIN_SYMBOLS)
    assert not first & third and not second & third


def test_training_workspace_bytes(L):
    lib = L.lib()
    cfg = L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, 1)
    names = _table(L, cfg)
    for code in (0, 1, 3):
        c = L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, code)
        inf = lib.gg_clip_text_workspace_bytes(C.byref(c), 5, 9)
        full = lib.gg_clip_text_train_workspace_bytes(C.byref(c), 5, 9, None)
        assert inf > 0 and full >= inf
        assert lib.gg_clip_text_train_workspace_bytes(C.byref(c), 10, 9, None) > full                     # grows with batch
        assert lib.gg_clip_text_train_workspace_bytes(C.byref(c), 5, 9, bytes(len(names))) == inf         # all frozen: the inference size
        top = lib.gg_clip_text_train_workspace_bytes(C.byref(c), 5, 9, _mask(names, lambda n: ".layers.1." in n))
        assert inf < top < full                                                                           # one kept layer instead of two
    assert lib.gg_clip_text_train_workspace_bytes(C.byref(cfg), 4, 78, None) < 0 and b"position" in lib.gg_last_error()
    assert lib.gg_clip_text_train_workspace_bytes(C.byref(cfg), 4, 77, None) > 0
    bad = L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, 2)
    assert lib.gg_clip_text_train_workspace_bytes(C.byref(bad), 4, 9, None) < 0 and b"act_dtype" in lib.gg_last_error()
    bad = L.ClipTextCfg(128, 256, 2, 4, 64, 77, 1e-5, 1)       # head dim 32
    assert lib.gg_clip_text_train_workspace_bytes(C.byref(bad), 4, 9, None) < 0 and b"head_dim" in lib.gg_last_error()
    assert lib.gg_clip_text_first_trained_layer(C.byref(bad), None) < 0 and b"head_dim" in lib.gg_last_error()
    assert lib.gg_embedding_scatter_add_scratch_bytes(7392) >= 8 * 7392 and lib.gg_embedding_scatter_add_scratch_bytes(0) < 0


def test_first_trained_layer(L):
    lib = L.lib()
    cfg = L.ClipTextCfg(128, 256, 3, 2, 64, 77, 1e-5, 1)
    names = _table(L, cfg)
    ftl = lambda sel: lib.gg_clip_text_first_trained_layer(C.byref(cfg), _mask(names, sel))
    assert lib.gg_clip_text_first_trained_layer(C.byref(cfg), None) == 0
    assert ftl(lambda n: False) == 3                                              # nothing: no layer is kept
    assert ftl(lambda n: n.startswith("final_layer_norm")) == 3                   # the final norm alone keeps no layer
    assert ftl(lambda n: ".layers.2." in n) == 2
    assert ftl(lambda n: n.endswith("layers.1.mlp.fc2.bias") or ".layers.2." in n) == 1
    assert ftl(lambda n: n.endswith("layers.0.layer_norm1.weight")) == 0
    assert ftl(lambda n: n == "embeddings.position_embedding.weight") == 0        # a table trains: every layer back-propagates
    assert ftl(lambda n: n == "embeddings.token_embedding.weight" or ".layers.2." in n) == 0


def test_text_training_is_opt_in(L):
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel
    from tests import clip_text_golden as G
    m = CLIPModel(config=G.tiny_config())
    assert m.train_text is False and m.text_model.wants_training() is False
    assert m.set_text_training(True) is True and m.set_text_training(True) is False and m.train_text is True
    assert m.text_model.wants_training() is True
    for p in m.text_model.parameters():
        p.requires_grad = False
    assert m.text_model.wants_training() is False                                 # every text tensor frozen: the inference forward
    assert CLIPModel(config=G.tiny_config(), train_text=True).train_text is True
