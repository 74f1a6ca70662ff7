"""CPU-only checks of the second header (include/gg_clip_text.h: text tower, contrastive head, gradient norm): every prototype exported and bound, struct
layouts, include/gg.h's own symbol set untouched, the text tensor table against transformers' state dict (the fixture), the EOS pooling rule, the linear
warm-up schedule against transformers' own, and the refusal of host tensors."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import clip_text_golden as G

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


def test_text_header_symbols_exported_and_bound(L):
    hdr = _protos("gg_clip_text.h")
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.TEXT_SYMBOLS) and len(declared) == 14
    lib = L.lib()
    for n in L.TEXT_SYMBOLS:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        args = m.group(1)
        cnt = 0 if args.strip() in ("void", "") else len(args.split(","))
        assert cnt == len(L.TEXT_SIGNATURES[n][1]), n


def test_first_header_symbol_set_is_unchanged(L):
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", _protos("gg.h")))
    assert declared == set(L.SYMBOLS)
    assert not declared & set(L.TEXT_SYMBOLS)


def test_text_struct_layouts_match_header(L):
    src = '#include <stdio.h>\n#include "gg_clip_text.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(GgClipTextCfg),sizeof(GgContrastiveArgs),sizeof(GgAttnArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert [C.sizeof(x) for x in (L.ClipTextCfg, L.ContrastiveArgs, L.AttnArgs)] == sizes


def test_text_tensor_table_matches_the_fixture_state_dict(L):
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel
    sd = G.decode_state_dict()
    m = CLIPModel(config=G.tiny_config())
    want = [(k[len("text_model."):], tuple(v.shape)) for k, v in sd.items() if k.startswith("text_model.")]
    got = [(t["name"], t["shape"]) for t in m.text_model.table]
    assert sorted(got) == sorted(want) and len(got) == 2 + 2 * 16 + 2
    offs = [t["offset"] for t in m.text_model.table]
    assert offs == sorted(offs) and all(o % 8 == 0 for o in offs)
    assert set(m.state_dict()) == set(sd)                      # the whole model carries transformers' keys
    m.load_hf_state_dict(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k].reshape(v.shape)), k
    # the vision sub-dict loads into the stand-alone tower (what the reference's step 6 saves)
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    tower = CLIPVisionTower(**G.TINY["vision"])
    tower.load_hf_state_dict({k: v for k, v in sd.items() if k.startswith("vision_model.")})
    assert torch.equal(tower.vision_model.flat_params, m.vision_model.flat_params)
    # refused configurations, by name
    bad = L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, 2)
    assert L.lib().gg_clip_text_num_tensors(C.byref(bad)) < 0 and b"act_dtype" in L.lib().gg_last_error()
    bad = L.ClipTextCfg(128, 256, 2, 4, 64, 77, 1e-5, 1)       # head dim 32
    assert L.lib().gg_clip_text_num_tensors(C.byref(bad)) < 0 and b"head_dim" in L.lib().gg_last_error()
    ok = L.ClipTextCfg(128, 256, 2, 2, 64, 77, 1e-5, 1)
    assert L.lib().gg_clip_text_workspace_bytes(C.byref(ok), 4, 78) < 0 and b"position" in L.lib().gg_last_error()
    assert L.lib().gg_clip_text_workspace_bytes(C.byref(ok), 4, 77) > 0


def test_freeze_backbone_keep_head_works_unchanged(L):
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel, LOGIT_SCALE_INIT
    m = CLIPModel(config=G.tiny_config())
    for p in m.parameters():                                    # pretrain_idun.py:220-239, verbatim in effect
        p.requires_grad = False
    if hasattr(m, "logit_scale"):
        m.logit_scale.requires_grad = True
    for name, p in m.named_parameters():
        if "visual_projection" in name:
            p.requires_grad = True
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == ["logit_scale", "visual_projection.weight"]
    assert abs(float(m.logit_scale) - np.log(1 / 0.07)) < 1e-6 and LOGIT_SCALE_INIT == np.log(1 / 0.07)
    big = CLIPModel("openai/clip-vit-large-patch14-336").config
    assert (big.text_config.hidden_size, big.text_config.intermediate_size, big.text_config.num_layers, big.text_config.num_heads, big.projection_dim) == (768, 3072, 12, 12, 768)
    assert (big.text_config.vocab_size, big.text_config.max_positions) == (49408, 77)


def test_eos_position_rule():
    from geoguessr_ai_amd.pretrain.clip_model import eos_positions
    z = G.load()
    ids = torch.from_numpy(z["input_ids"])
    assert eos_positions(ids, 63).tolist() == z["eos_pos"].tolist() == [5, 1, 3, 7, 8]
    assert eos_positions(ids, 2).tolist() == z["eos_pos"].tolist()          # argmax rule: 63 is each row's maximum
    two = torch.tensor([[0, 2, 9, 2, 1], [0, 9, 9, 9, 9]])
    assert eos_positions(two, 2).tolist() == [2, 1]                          # eos_token_id == 2: the argmax (first maximum), not the id
    assert eos_positions(two, 9).tolist() == [2, 1]                          # otherwise: the FIRST position equal to the id
    assert eos_positions(torch.tensor([[0, 9, 5, 9]]), 9).tolist() == [1]


def test_linear_warmup_lr_matches_transformers():
    from transformers import get_linear_schedule_with_warmup
    from geoguessr_ai_amd.optim import linear_warmup_lr
    import math
    for total, ratio in ((50, 0.2), (37, 0.2), (10, 0.0)):
        warm = math.ceil(total * ratio)
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=3e-4)
        sch = get_linear_schedule_with_warmup(opt, warm, total)
        want = []
        for _ in range(total + 1):
            want.append(opt.param_groups[0]["lr"])
            opt.step(); sch.step()
        for s in sorted({0, max(warm - 1, 0), warm, total // 2, total - 1, total}):
            assert linear_warmup_lr(s, total, ratio, 3e-4) == pytest.approx(want[s], rel=1e-12, abs=1e-18), (total, s)


def test_host_tensors_are_refused(L):
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel, contrastive
    m = CLIPModel(config=G.tiny_config())
    z = G.load()
    with pytest.raises(L.GgError):
        m(input_ids=torch.from_numpy(z["input_ids"]), pixel_values=torch.from_numpy(z["pixel_values"]), return_loss=True)
    with pytest.raises(L.GgError):
        m.get_text_features(input_ids=torch.from_numpy(z["input_ids"]))
    with pytest.raises(L.GgError):
        m.get_image_features(pixel_values=torch.from_numpy(z["pixel_values"]))
    with pytest.raises(L.GgError):
        contrastive(torch.randn(2, 8), torch.randn(2, 8), torch.tensor(2.0), True)
