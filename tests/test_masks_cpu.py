"""The trainable-mask family of tests/masks.py and what the workspace plan of the built libgg.so makes of it, on the host (the plan functions are
host code: no GPU needed).  The mask decides the schedule of gg_tinyvit_forward / gg_tinyvit_backward: which activations are retained, which are
temporaries in two alternating ring slots, whether the gradient buffers alias those slots.  Here: the family is well-formed and flips every group of
``tr(tensor)`` sites of csrc/tinyvit.hip both ways; the planned size is positive, monotone in the mask and equal to the all-trainable size for NULL and
all ones; every retained region lies inside the workspace, aligned and disjoint from every other; temporaries are refused by name."""
import ctypes as C
import os
import re

import pytest

from tests import masks as M

MODELS = ("tiny_vit_5m_224", "tiny_vit_21m_224")


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _table(name, precision="fp32", recompute=False):
    from geoguessr_ai_amd.models.tinyvit import make_cfg, _tensor_table
    cfg, _, _ = make_cfg(name, precision=precision, grad_checkpointing=recompute)
    return cfg, _tensor_table(cfg)


@pytest.mark.parametrize("name", MODELS + ("tiny_vit_21m_512",))
def test_family_is_well_formed(L, name):
    _, table = _table(name)
    names = M.param_names(table)
    fam = M.family(table)
    assert tuple(fam) == M.FAMILY_NAMES and set(M.REDUCED) <= set(fam)
    assert len([k for k in fam if k.startswith("random[")]) >= 8
    for key, mask in fam.items():
        assert mask <= set(names), key
        assert 0 < len(mask) < len(names), (key, len(mask))                     # neither empty nor full
        assert not M.pair_violations(names, mask), (key, M.pair_violations(names, mask)[:3])
        assert mask not in (M.policy_mask(table, "all"), M.policy_mask(table, "freeze")), key
    assert len(set(fam.values())) == len(fam)                                   # no two names for one mask
    assert len(fam["head_norm_only"]) == 2
    assert fam["norms"] | fam["matrices"] | fam["attention_biases"] == set(names)
    assert not fam["norms"] & fam["matrices"]


# Groups of tr(...) sites of csrc/tinyvit.hip, as tensor-name patterns of ONE instance of the layer: the site's condition is "none of these trains"
# (plan_build's keep() / alloc_temp per tensor, the fused forms of block_bwd / merge_bwd / mbconv_bwd / patch_embed_bwd per group).  The family must hold a mask that makes it true and one that
# makes it false; the two policies alone leave most of them one-sided inside the frozen stages.
SITE_GROUPS = {
    "plan: ln1 is a temporary (qkv frozen)": [r"^stages\.1\.blocks\.0\.attn\.qkv\.weight$"],
    "plan: x1 is a temporary (local_conv taps frozen)": [r"^stages\.2\.blocks\.0\.local_conv\.conv\.weight$"],
    "plan: ln2 is a temporary (fc1 frozen)": [r"^stages\.2\.blocks\.3\.mlp\.fc1\.weight$"],
    "plan: fc1.act is a temporary (fc2 frozen)": [r"^stages\.3\.blocks\.1\.mlp\.fc2\.weight$"],
    "plan: MBConv act1 temporary / re-formed in backward (conv2 taps)": [r"^stages\.0\.blocks\.0\.conv2\.conv\.weight$"],
    "plan + forward fuse_pro: MBConv act2 (conv3 weight)": [r"^stages\.0\.blocks\.1\.conv3\.conv\.weight$"],
    "plan: PatchMerging act1 (conv2 taps)": [r"^stages\.2\.downsample\.conv2\.conv\.weight$"],
    "plan: PatchMerging act2 (conv3 weight)": [r"^stages\.1\.downsample\.conv3\.conv\.weight$"],
    "backward lncol: local_conv taps + BatchNorm + norm2 all frozen": [r"^stages\.2\.blocks\.2\.local_conv\.", r"^stages\.2\.blocks\.2\.mlp\.norm\."],
    "backward lncol, taps alone": [r"^stages\.2\.blocks\.2\.local_conv\.conv\.weight$"],
    "backward lncol, local_conv BatchNorm alone": [r"^stages\.2\.blocks\.2\.local_conv\.bn\."],
    "backward lncol, norm2 alone": [r"^stages\.2\.blocks\.2\.mlp\.norm\."],
    "backward MBConv fused chain: conv1 and conv2 weights frozen": [r"^stages\.0\.blocks\.1\.conv[12]\.conv\.weight$"],
    "backward MBConv: conv1 BatchNorm inside the chain": [r"^stages\.0\.blocks\.1\.conv1\.bn\."],
    "backward MBConv: conv2 BatchNorm inside the chain": [r"^stages\.0\.blocks\.1\.conv2\.bn\."],
    "backward MBConv: conv3 BatchNorm": [r"^stages\.0\.blocks\.1\.conv3\.bn\."],
    "backward PatchMerging fused chain: conv1 and conv2 weights frozen": [r"^stages\.2\.downsample\.conv[12]\.conv\.weight$"],
    "backward PatchMerging: conv1 BatchNorm": [r"^stages\.2\.downsample\.conv1\.bn\."],
    "backward PatchMerging: conv2 BatchNorm": [r"^stages\.2\.downsample\.conv2\.bn\."],
    "backward PatchMerging: conv3": [r"^stages\.3\.downsample\.conv3\."],
    "backward PatchEmbed need1": [r"^patch_embed\.conv1\."],
    "backward PatchEmbed need2": [r"^patch_embed\."],
    "backward PatchEmbed conv1 weight (convnorm_wgrad_from_dz returns early)": [r"^patch_embed\.conv1\.conv\.weight$"],
    "backward block Linears: qkv": [r"^stages\.1\.blocks\.1\.attn\.qkv\."],
    "backward block Linears: proj": [r"^stages\.1\.blocks\.1\.attn\.proj\."],
    "backward norm1": [r"^stages\.3\.blocks\.0\.attn\.norm\."],
    "backward attention-bias table": [r"^stages\.3\.blocks\.0\.attn\.attention_biases$"],
    "backward head.norm": [r"^head\.norm\."],
}


@pytest.mark.parametrize("name", MODELS)
def test_family_flips_every_site_group_both_ways(L, name):
    _, table = _table(name)
    names = M.param_names(table)
    fam = M.family(table)
    for group, patterns in SITE_GROUPS.items():
        members = [n for n in names if any(re.search(p, n) for p in patterns)]
        assert members, group
        frozen = [k for k, mask in fam.items() if not mask & set(members)]
        trains = [k for k, mask in fam.items() if mask & set(members)]
        assert frozen and trains, (group, len(frozen), len(trains))
    # the PatchEmbed middle case: conv2 needs its gradient although conv1 does not
    pe1 = {n for n in names if n.startswith("patch_embed.conv1.")}
    pe2 = {n for n in names if n.startswith("patch_embed.conv2.")}
    assert any(mask & pe2 and not mask & pe1 for mask in fam.values())
    # lncol's five tensors: frozen together while the block's Linears train (the fused form next to weight gradients)
    five = {n for n in names if re.search(r"^stages\.2\.blocks\.2\.(local_conv|mlp\.norm)\.", n)}
    assert any(not mask & five and "stages.2.blocks.2.mlp.fc1.weight" in mask for mask in fam.values())


def _ws(L, cfg, batch, mask):
    n = L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(cfg), batch, 1, mask)
    assert n > 0, L.lib().gg_last_error().decode()
    return n


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
def test_workspace_size_is_positive_and_monotone_in_the_mask(L, name, precision, recompute):
    cfg, table = _table(name, precision, recompute)
    fam = dict(M.family(table), all=M.policy_mask(table, "all"), freeze=M.policy_mask(table, "freeze"), none=frozenset())
    for batch in (8, 1024):
        size = {k: _ws(L, cfg, batch, M.to_bytes(table, mask)) for k, mask in fam.items()}
        assert _ws(L, cfg, batch, None) == size["all"]                          # NULL = all ones
        keys = list(fam)
        for a in keys:
            for b in keys:
                if fam[a] <= fam[b]:
                    assert size[a] <= size[b], (batch, a, size[a], b, size[b])  # a frozen tensor never costs workspace
        if not recompute:
            assert size["none"] < size["all"]


def _region_names(cfg):
    names = ["patch_embed.col1", "patch_embed.conv1.y", "patch_embed.conv1.stat", "patch_embed.col2", "patch_embed.conv2.y", "patch_embed.conv2.stat",
             "patch_embed.out", "head.pooled", "head.mean", "head.rstd", "scratch.statpart", "scratch.bn", "scratch.ln", "scratch.colsum", "scratch.splitk",
             "scratch.foldw", "scratch.foldb"] + [f"scratch.G{i}" for i in range(5)]
    for i in range(cfg.depths[0]):
        p = f"stages.0.blocks.{i}"
        names += [f"{p}.out", f"{p}.act1", f"{p}.act2"] + [f"{p}.conv{k}.{leaf}" for k in (1, 2, 3) for leaf in ("y", "stat")]
    for s in (1, 2, 3):
        p = f"stages.{s}.downsample"
        names += [f"{p}.out", f"{p}.act1", f"{p}.act2"] + [f"{p}.conv{k}.{leaf}" for k in (1, 2, 3) for leaf in ("y", "stat")]
        for i in range(cfg.depths[s]):
            p = f"stages.{s}.blocks.{i}"
            names += [f"{p}.{leaf}" for leaf in ("ln1", "mean1", "rstd1", "qkv", "attn.out", "attn.lse", "x1", "local_conv.y", "local_conv.stat", "x2", "ln2",
                                                 "mean2", "rstd2", "fc1.pre", "fc1.act", "out")]
    return names


def _expected_temporaries(cfg, mask):
    """What plan_build makes a temporary (or a region the backward re-forms) under the default forward fusions: the input of a frozen Linear /
    depthwise conv, act2 in front of a frozen conv3, and act1 always (the fused depthwise forward never writes it)."""
    temps = set()
    for i in range(cfg.depths[0]):
        p = f"stages.0.blocks.{i}"
        temps.add(f"{p}.act1")
        if f"{p}.conv3.conv.weight" not in mask:
            temps.add(f"{p}.act2")
    for s in (1, 2, 3):
        p = f"stages.{s}.downsample"
        temps.add(f"{p}.act1")
        if f"{p}.conv3.conv.weight" not in mask:
            temps.add(f"{p}.act2")
        for i in range(cfg.depths[s]):
            p = f"stages.{s}.blocks.{i}"
            for leaf, weight in (("ln1", "attn.qkv.weight"), ("x1", "local_conv.conv.weight"), ("ln2", "mlp.fc1.weight"), ("fc1.act", "mlp.fc2.weight")):
                if f"{p}.{weight}" not in mask:
                    temps.add(f"{p}.{leaf}")
    return temps


@pytest.mark.parametrize("key", M.FAMILY_NAMES + ("all", "freeze"))
@pytest.mark.parametrize("name,precision,batch", [("tiny_vit_5m_224", "fp32", 8), ("tiny_vit_21m_224", "bf16", 4)])
def test_retained_regions_are_inside_aligned_and_disjoint(L, name, precision, batch, key):
    cfg, table = _table(name, precision)
    mask = M.mask_of(table, key)
    mb = M.to_bytes(table, mask)
    total = _ws(L, cfg, batch, mb)
    expect_temp = _expected_temporaries(cfg, mask)
    regions = {}
    off, nb = C.c_int64(), C.c_int64()
    for n in _region_names(cfg):
        rc = L.lib().gg_tinyvit_activation_info_masked(C.byref(cfg), batch, n.encode(), mb, C.byref(off), C.byref(nb))
        if rc == 0:
            assert n not in expect_temp, (key, n, "retained although nothing reads it again")
            regions[n] = (off.value, nb.value)
        else:
            msg = L.lib().gg_last_error().decode()
            assert "not retained under this trainable mask" in msg and n in msg, (key, n, msg)
            assert n in expect_temp, (key, n, msg)
    for n, (o, b) in regions.items():
        assert o >= 0 and b > 0 and o % 256 == 0 and o + b <= total, (key, n, o, b, total)
    spans = sorted((o, o + b, n) for n, (o, b) in regions.items())
    for (o0, e0, n0), (o1, e1, n1) in zip(spans, spans[1:]):
        assert e0 <= o1, (key, n0, n1)            # pairwise disjoint, the gradient buffers scratch.G* included (G0 / G1 may alias only temporaries)


# ------------------------------------------------------------------------------------------- CLIP
def _clip(L):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    tower = CLIPVisionTower("openai/clip-vit-tiny-masks", hidden_size=64, intermediate_size=128, num_layers=4, num_heads=1, image_size=64, patch_size=16,
                            precision="fp32")
    return tower


def test_clip_masks_first_trained_layer_and_workspace(L):
    tower = _clip(L)
    vm, lib = tower.vision_model, L.lib()
    names = [t["name"] for t in vm.table]
    nl = tower.cfg.num_layers
    fam = M.clip_family(names, nl)
    assert len(fam) >= 10 and all(0 < len(m) < len(names) for m in fam.values())
    full = bytes(1 for _ in vm.table)
    ws_all = lib.gg_clip_workspace_bytes(C.byref(tower.cfg), 8, 1, full)
    assert ws_all > 0 and lib.gg_clip_workspace_bytes(C.byref(tower.cfg), 8, 1, None) == ws_all
    ws_eval = lib.gg_clip_workspace_bytes(C.byref(tower.cfg), 8, 0, None)
    embed = ("embeddings.", "pre_layrnorm.")
    for key, mask in fam.items():
        mb = bytes(int(t["name"] in mask) for t in vm.table)
        layers = [int(n.split(".")[2]) for n in mask if n.startswith("encoder.layers.")]
        expect = 0 if any(n.startswith(embed) for n in mask) else min(layers)
        assert lib.gg_clip_first_trained_layer(C.byref(tower.cfg), mb) == expect, key
        ws = lib.gg_clip_workspace_bytes(C.byref(tower.cfg), 8, 1, mb)
        assert ws_eval < ws <= ws_all, (key, ws, ws_all)
        if any(n.startswith(embed) for n in mask):
            assert ws == ws_all, key                    # the backward runs through every layer and the embeddings: the all-trainable plan
    # the workspace grows with the number of layers the backward crosses
    sizes = []
    for l0 in range(nl):
        mb = bytes(int(t["name"].startswith(f"encoder.layers.{l0}.mlp.fc2.")) for t in vm.table)
        assert lib.gg_clip_first_trained_layer(C.byref(tower.cfg), mb) == l0
        sizes.append(lib.gg_clip_workspace_bytes(C.byref(tower.cfg), 8, 1, mb))
    assert sizes == sorted(sizes, reverse=True) and len(set(sizes)) == nl
    none = bytes(len(vm.table))
    assert lib.gg_clip_first_trained_layer(C.byref(tower.cfg), none) == nl
    # post_layernorm alone: not on the path, nothing is kept
    post = bytes(int(t["name"].startswith("post_layernorm")) for t in vm.table)
    assert lib.gg_clip_first_trained_layer(C.byref(tower.cfg), post) == nl
