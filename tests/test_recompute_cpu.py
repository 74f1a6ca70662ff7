"""Activation recompute (GgTinyVitCfg.recompute, TinyVitBackbone.set_grad_checkpointing) on the host side: the checkpointed workspace plan of the
built libgg.so -- its size against the keep-everything plan, which tensors stay addressable, and that the shared segment region touches nothing
else.  The plan functions are host code: no GPU needed."""
import ctypes as C
import os
import warnings

import pytest

GiB = 2 ** 30
# gg_tinyvit_workspace_bytes_masked of the keep-everything plan before recompute existed: recompute = 0 must keep these to the byte
C2_FREEZE_BYTES = 111256321792          # 21M-224, 1024 images, fp32, freeze_all_but_last_stage (103.6 GiB)
C2_ALL_BYTES = 148095942400             # the same, every tensor trainable (137.9 GiB)


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _cfg_masks(name, precision, recompute):
    """cfg + (freeze_all_but_last_stage mask, all-trainable mask) from the tensor table (the masks TinyVitBackbone.trainable_mask() gives)."""
    from geoguessr_ai_amd.models.tinyvit import make_cfg, _tensor_table
    cfg, _, _ = make_cfg(name, precision=precision, grad_checkpointing=bool(recompute))
    table = _tensor_table(cfg)
    frozen = ("stages.0.", "stages.1.", "stages.2.")
    freeze = bytes(int(t["kind"] == 0 and not t["name"].startswith(frozen)) for t in table)
    full = bytes(int(t["kind"] == 0) for t in table)
    return cfg, freeze, full, table


def _ws(L, cfg, batch, mask, training=1):
    n = L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(cfg), batch, training, mask)
    assert n > 0, L.lib().gg_last_error().decode()
    return n


def _info(L, cfg, batch, name, mask):
    off, nb = C.c_int64(), C.c_int64()
    rc = L.lib().gg_tinyvit_activation_info_masked(C.byref(cfg), batch, name.encode(), mask, C.byref(off), C.byref(nb))
    return (off.value, nb.value) if rc == 0 else L.lib().gg_last_error().decode()


@pytest.mark.parametrize("precision", ["fp32", "fp32_split"])
def test_c2_plan_shrinks(L, precision):
    cfg0, freeze, full, _ = _cfg_masks("tiny_vit_21m_224", precision, 0)
    cfg1, _, _, _ = _cfg_masks("tiny_vit_21m_224", precision, 1)
    off_f, off_a = _ws(L, cfg0, 1024, freeze), _ws(L, cfg0, 1024, full)
    assert (off_f, off_a) == (C2_FREEZE_BYTES, C2_ALL_BYTES)
    on_f, on_a = _ws(L, cfg1, 1024, freeze), _ws(L, cfg1, 1024, full)
    assert on_f <= 0.65 * off_f, on_f / off_f
    assert on_a <= 0.55 * off_a, on_a / off_a


def test_default_512_model_all_trainable_fits_only_with_recompute(L):
    cfg0, _, full, _ = _cfg_masks("tiny_vit_21m_512", "fp32", 0)
    cfg1, _, _, _ = _cfg_masks("tiny_vit_21m_512", "fp32", 1)
    assert _ws(L, cfg0, 512, full) > 288 * GiB
    assert _ws(L, cfg1, 512, full) < 200 * GiB


def test_inference_ignores_the_setting(L):
    cfg0, _, _, _ = _cfg_masks("tiny_vit_21m_224", "fp32", 0)
    cfg1, _, _, _ = _cfg_masks("tiny_vit_21m_224", "fp32", 1)
    for b in (1, 64):
        assert _ws(L, cfg0, b, None, training=0) == _ws(L, cfg1, b, None, training=0)


def _checkpoint_names(cfg):
    names = ["patch_embed.col1", "patch_embed.conv1.y", "patch_embed.conv1.stat", "patch_embed.col2", "patch_embed.conv2.y",
             "patch_embed.conv2.stat", "patch_embed.out", "head.pooled", "head.mean", "head.rstd"]
    for i in range(cfg.depths[0]):
        names += [f"stages.0.blocks.{i}.out"] + [f"stages.0.blocks.{i}.conv{k}.stat" for k in (1, 2, 3)]
    for s in (1, 2, 3):
        names += [f"stages.{s}.downsample.out"] + [f"stages.{s}.downsample.conv{k}.stat" for k in (1, 2, 3)]
        for i in range(cfg.depths[s]):
            names += [f"stages.{s}.blocks.{i}.out", f"stages.{s}.blocks.{i}.local_conv.stat"]
    return names


@pytest.mark.parametrize("name,precision,batch,policy", [("tiny_vit_21m_224", "fp32", 1024, "freeze"), ("tiny_vit_21m_224", "bf16", 64, "all"),
                                                         ("tiny_vit_21m_384", "fp32_split", 4, "all")])
def test_checkpoint_layout(L, name, precision, batch, policy):
    cfg, freeze, full, _ = _cfg_masks(name, precision, 1)
    mask = freeze if policy == "freeze" else full
    total = _ws(L, cfg, batch, mask)
    seg = _info(L, cfg, batch, "scratch.segment", mask)
    assert isinstance(seg, tuple) and seg[1] > 0
    regions = {"scratch.segment": seg}
    for n in _checkpoint_names(cfg) + [f"scratch.G{i}" for i in range(5)]:
        r = _info(L, cfg, batch, n, mask)
        assert isinstance(r, tuple), (n, r)
        regions[n] = r
    for n, (o, b) in regions.items():
        assert 0 <= o and b > 0 and o + b <= total and o % 256 == 0, n
    spans = sorted((o, o + b, n) for n, (o, b) in regions.items())
    for (o0, e0, n0), (o1, e1, n1) in zip(spans, spans[1:]):
        assert e0 <= o1, (n0, n1)                    # pairwise disjoint: the segment region included, the gradient buffers included
    # segment-internal tensors are recomputed, not retained: refused with the recompute message (their names exist in the recompute-off plan)
    cfg0, _, _, _ = _cfg_masks(name, precision, 0)
    internal = ["stages.2.blocks.3.qkv", "stages.0.blocks.0.conv1.y", "stages.0.blocks.1.conv3.y", "stages.1.downsample.conv2.y",
                "stages.3.blocks.1.fc1.pre", "stages.2.blocks.0.mean1", "stages.1.blocks.0.x2", "stages.3.blocks.0.attn.lse"]
    if policy == "all":
        internal += ["stages.1.blocks.1.ln1", "stages.0.blocks.0.act2", "stages.2.downsample.act2"]
    for n in internal:
        assert isinstance(_info(L, cfg0, batch, n, mask), tuple), n
        msg = _info(L, cfg, batch, n, mask)
        assert isinstance(msg, str) and "recompute" in msg and n in msg, (n, msg)
    # the frozen-mask temporaries live in the segment region too: refused with the same message, not the temporary one
    if policy == "freeze":
        for n in ("stages.1.blocks.0.ln1", "stages.2.blocks.5.fc1.act", "stages.0.blocks.1.act2"):
            msg = _info(L, cfg, batch, n, mask)
            assert isinstance(msg, str) and "recompute" in msg, (n, msg)


def test_python_surface_sets_the_field(L):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="fp32")
        m2 = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="fp32", grad_checkpointing=True)
    bb = m.backbone
    assert bb.grad_checkpointing is False and bb.cfg.recompute == 0
    assert bb.set_grad_checkpointing() is bb
    assert bb.grad_checkpointing is True and bb.cfg.recompute == 1
    bb.set_grad_checkpointing(False)
    assert bb.grad_checkpointing is False and bb.cfg.recompute == 0
    assert m2.backbone.grad_checkpointing is True and m2.backbone.cfg.recompute == 1
    # the tensor table does not depend on the setting (same state dict, same flat offsets)
    assert [(t["name"], t["offset"]) for t in bb.table] == [(t["name"], t["offset"]) for t in m2.backbone.table]
