"""CPU-only checks of the TinyViT classifier fine-tune (include/gg_cls.h, geoguessr_ai_amd.finetune_tinyvit): the boundary of the new entry points, the
class map with its UNKNOWN quirk, the learning-rate schedule, the rank -> top-k rule and the checkpoint layout.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_cls_header_symbols_and_struct_layout_match_the_binding(L):
    hdr = open(os.path.join(ROOT, "include", "gg_cls.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.CLS_SYMBOLS) == {"gg_cls_head", "gg_tinyvit_last_map_info"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.CLS_SIGNATURES[n][1]), n
    # sizeof and every field offset of GgClsHeadArgs, from the host compiler
    fields = [f[0] for f in L.ClsHeadArgs._fields_]
    body = re.search(r"typedef struct GgClsHeadArgs \{(.*?)\} GgClsHeadArgs;", hdr, re.S).group(1)
    in_header = re.findall(r"[\s\*](\w+)\s*[;,]", body)
    assert in_header == fields                                                     # same names in the same order
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gg_cls.h"\nint main(){printf("%zu", sizeof(GgClsHeadArgs));' + \
          "".join(f'printf(" %zu", offsetof(GgClsHeadArgs, {f}));' for f in fields) + 'printf("\\n");return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert vals == [C.sizeof(L.ClsHeadArgs)] + [getattr(L.ClsHeadArgs, f).offset for f in fields]


def test_cls_head_refuses_bad_arguments_without_a_device(L):
    """Shape and NULL checks come before anything touches the device: they answer on a machine without one."""
    lib = L.lib()
    a = L.ClsHeadArgs()
    assert lib.gg_cls_head(None, None) != 0 and b"null args" in lib.gg_last_error()
    a.N, a.C, a.ldl = 2, 3, 3
    assert lib.gg_cls_head(C.byref(a), None) != 0 and b"null logits" in lib.gg_last_error()
    buf = (C.c_float * 16)()
    a.logits, a.labels = C.addressof(buf), C.addressof(buf)
    for field, val, msg in (("N", 0, b"N=0"), ("C", 0, b"C=0"), ("ldl", 2, b"ldl=2 < C=3")):
        b = L.ClsHeadArgs.from_buffer_copy(a)
        setattr(b, field, val)
        assert lib.gg_cls_head(C.byref(b), None) != 0 and msg in lib.gg_last_error(), field
    b = L.ClsHeadArgs.from_buffer_copy(a)
    b.dlogits, b.ldd = C.addressof(buf), 2
    assert lib.gg_cls_head(C.byref(b), None) != 0 and b"ldd=2 < C=3" in lib.gg_last_error()
    b = L.ClsHeadArgs.from_buffer_copy(a)
    b.loss = C.addressof(buf)
    assert lib.gg_cls_head(C.byref(b), None) != 0 and b"loss_rows" in lib.gg_last_error()
    assert lib.gg_cls_head(C.byref(a), None) != 0                                  # host pointers (or no device at all): refused, nothing launched
    assert all(v == 0.0 for v in buf)


def test_class_map_and_the_unknown_quirk():
    from geoguessr_ai_amd.finetune_tinyvit import build_class_map, class_id
    m = build_class_map(["NO", "SE", "NO", "DK", "FI", "SE"])
    assert m == {"DK": 0, "FI": 1, "NO": 2, "SE": 3} and list(m) == sorted(m)
    assert build_class_map([3, 1, 2]) == {"1": 0, "2": 1, "3": 2}                   # .astype(str) of the reference
    assert class_id(m, "SE") == 3 and "UNKNOWN" not in m
    # an unseen label: setdefault("UNKNOWN", 0) -- aliases class 0 (DK) and grows the map by one key
    assert class_id(m, "XX") == 0 and m["UNKNOWN"] == 0 and len(m) == 5
    assert class_id(m, "YY") == 0 and len(m) == 5
    with_unknown = build_class_map(["UNKNOWN", "AA", "ZZ"])
    assert class_id(with_unknown, "??") == with_unknown["UNKNOWN"] == 1            # a real UNKNOWN class keeps its own id


def test_lr_schedule_equals_torch_cosine_annealing():
    from geoguessr_ai_amd.finetune_tinyvit import cosine_lr
    for epochs, lr in ((5, 5e-4), (3, 1e-3), (1, 5e-4)):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.AdamW([p], lr=lr, weight_decay=0.05)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs)
        for epoch in range(epochs):
            assert abs(cosine_lr(epoch, epochs, lr) - opt.param_groups[0]["lr"]) <= 1e-12 * lr, (epochs, epoch)
            opt.step()
            sched.step()
    assert cosine_lr(0, 5, 5e-4) == 5e-4


def _rank(logits, labels):
    """The kernel's rank rule on the host."""
    zl = logits.gather(1, labels.view(-1, 1))
    idx = torch.arange(logits.shape[1]).view(1, -1)
    return ((logits > zl) | ((logits == zl) & (idx < labels.view(-1, 1)))).sum(1)


@pytest.mark.parametrize("C_", [1, 2, 3, 4, 5, 6, 37])
def test_rank_rule_equals_topk_accuracy(C_):
    g = torch.Generator().manual_seed(C_)
    logits = torch.randn(64, C_, generator=g)
    labels = torch.randint(0, C_, (64,), generator=g)
    assert all(len(set(r.tolist())) == C_ for r in logits)                           # tie-free
    rank = _rank(logits, labels)
    for k in {1, min(5, C_)}:
        top = logits.topk(k, dim=1, largest=True, sorted=True).indices           # timm.utils.accuracy
        hit = (top == labels.view(-1, 1)).any(1)
        assert torch.equal(hit, rank < k), (C_, k)
    assert torch.equal(rank == 0, logits.argmax(1) == labels)


def test_checkpoint_dict_round_trips(tmp_path):
    from geoguessr_ai_amd.finetune_tinyvit import load_model_for_features
    from geoguessr_ai_amd.finetune_tinyvit.train_tinyvit_timm import _plain
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    m = TinyViTClassifier("tiny_vit_5m_224", num_classes=3, seed=5)
    adapter_keys = {k[len("backbone."):] for k in TinyViTAdapter("tiny_vit_5m_224", pretrained=False).state_dict()}
    assert set(m.state_dict()) == adapter_keys | {"head.fc.weight", "head.fc.bias"}
    w = m.head.fc.weight.detach()
    assert w.shape == (3, 320) and float(m.head.fc.bias.detach().abs().max()) == 0.0 and 0.017 < float(w.std()) < 0.023      # trunc_normal(std .02), zero bias
    class_to_id = {"DK": 0, "NO": 1, "SE": 2}
    path = str(tmp_path / "best.pt")
    torch.save({"model": {k: v.detach().cpu() for k, v in m.state_dict().items()}, "class_to_id": class_to_id,
                "args": _plain(dict(epochs=2, lr=5e-4, out_dir=tmp_path))}, path)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"model", "class_to_id", "args"} and ck["class_to_id"] == class_to_id and ck["args"]["out_dir"] == str(tmp_path)
    m2, c2 = load_model_for_features(path)
    assert c2 == class_to_id and m2.num_classes == 3 and not m2.training
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    # the UNKNOWN quirk grew the map after training: the head no longer fits, the encoder still loads
    ck["class_to_id"]["UNKNOWN"] = 0
    torch.save(ck, path)
    m3, _ = load_model_for_features(path)
    assert m3.num_classes == 4 and torch.equal(m3.backbone.flat_params, m.backbone.flat_params)
    with pytest.raises(RuntimeError, match="head.fc.weight"):
        m3.load_state_dict(ck["model"], strict=True)
    from geoguessr_ai_amd import _lib
    with pytest.raises(_lib.GgError):
        m3(torch.zeros(1, 3, 224, 224))                                            # no GPU here: loud, no fallback


def test_last_map_info_lies_inside_the_inference_workspace(L):
    from geoguessr_ai_amd.models.tinyvit import make_cfg
    lib = L.lib()
    for name, prec, res, ch, es in (("tiny_vit_5m_224", "fp32", 7, 320, 4), ("tiny_vit_5m_224", "bf16", 7, 320, 2), ("tiny_vit_21m_384", "fp32_split", 12, 576, 4)):
        cfg, _, _ = make_cfg(name, precision=prec)
        for batch in (1, 2, 5):
            off, nb, r, c = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
            assert lib.gg_tinyvit_last_map_info(C.byref(cfg), batch, C.byref(off), C.byref(nb), C.byref(r), C.byref(c)) == 0, lib.gg_last_error()
            assert (r.value, c.value) == (res, ch) and nb.value == batch * res * res * ch * es
            assert off.value % 256 == 0 and 0 <= off.value and off.value + nb.value <= lib.gg_tinyvit_workspace_bytes(C.byref(cfg), batch, 0)
    assert lib.gg_tinyvit_last_map_info(C.byref(cfg), 0, None, None, None, None) != 0 and b"batch" in lib.gg_last_error()
