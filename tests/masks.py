"""Trainable masks for the encoder runtimes, built from the tensor table by NAME (so they apply to every model size).

A mask is a frozenset of parameter names that train; everything else is frozen.  ``family(table)`` is the TinyViT family of
tests/test_masks_cpu.py and tests/test_gpu_masks.py: every mask keeps the pair rule of gg_tinyvit_backward (``x.weight`` and ``x.bias`` train or
freeze together) and each is chosen to flip ``tr(tensor)`` branches of csrc/tinyvit.hip that the two policies of the rest of the suite
(freeze_all_but_last_stage, everything trainable) never flip.  ``clip_family(names, num_layers)`` is the CLIP tower's (csrc/clip.hip takes
half pairs: its LayerNorm backward has a dump row for the frozen half)."""
import random as _random
import re

RANDOM_SEEDS = tuple(range(8))


def param_names(table):
    return [t["name"] for t in table if t["kind"] == 0]


def module_of(name):
    """The unit that trains or freezes as one: ``x`` for ``x.weight`` / ``x.bias``, the tensor itself otherwise (attention_biases)."""
    return name.rsplit(".", 1)[0] if name.endswith((".weight", ".bias")) else name


def pair_violations(names, mask):
    """(weight, bias) pairs of which the mask trains exactly one."""
    have = set(names)
    return [(n, n[:-7] + ".bias") for n in names
            if n.endswith(".weight") and n[:-7] + ".bias" in have and ((n in mask) != (n[:-7] + ".bias" in mask))]


def _sel(names, *patterns):
    rx = [re.compile(p) for p in patterns]
    return frozenset(n for n in names if any(r.search(n) for r in rx))


NORM = r"\.bn\.(weight|bias)$|norm\.(weight|bias)$"
MB = r"^stages\.0\.blocks\.\d+\."
MERGE = r"^stages\.\d+\.downsample\."


def family(table):
    """name -> frozenset of trainable parameter names (insertion order = the order the tests list them in)."""
    names = param_names(table)
    F = {}
    F["norms"] = _sel(names, NORM)
    F["attention_biases"] = _sel(names, r"attention_biases$")
    F["matrices"] = frozenset(names) - F["norms"] - F["attention_biases"]
    F["qkv_proj"] = _sel(names, r"\.attn\.(qkv|proj)\.")
    F["mlp"] = _sel(names, r"\.mlp\.fc[12]\.")
    F["fc2_only"] = _sel(names, r"\.mlp\.fc2\.")
    F["fc1_only"] = _sel(names, r"\.mlp\.fc1\.")
    F["attn_norm_only"] = _sel(names, r"\.attn\.norm\.")
    F["mlp_norm_only"] = _sel(names, r"\.mlp\.norm\.")
    F["local_conv_taps"] = _sel(names, r"\.local_conv\.conv\.weight$")
    F["local_conv_bn"] = _sel(names, r"\.local_conv\.bn\.")
    F["local_conv"] = _sel(names, r"\.local_conv\.")
    for tag, prefix in (("mbconv", MB), ("merge", MERGE)):
        for k in (1, 2, 3):
            F[f"{tag}_c{k}"] = _sel(names, prefix + rf"conv{k}\.")
            F[f"{tag}_c{k}_conv"] = _sel(names, prefix + rf"conv{k}\.conv\.weight$")
            F[f"{tag}_c{k}_bn"] = _sel(names, prefix + rf"conv{k}\.bn\.")
    F["pe1"] = _sel(names, r"^patch_embed\.conv1\.")
    F["pe2"] = _sel(names, r"^patch_embed\.conv2\.")
    F["stage0_only"] = _sel(names, r"^stages\.0\.")
    F["stage1_only"] = _sel(names, r"^stages\.1\.")
    F["stage2_only"] = _sel(names, r"^stages\.2\.")
    F["last_two_stages"] = _sel(names, r"^stages\.[23]\.", r"^head\.")
    F["one_middle_block"] = _sel(names, r"^stages\.2\.blocks\.1\.")
    F["head_norm_only"] = _sel(names, r"^head\.norm\.")
    modules = sorted({module_of(n) for n in names})
    for seed in RANDOM_SEEDS:
        rng = _random.Random(1000 + seed)
        on = {m for m in modules if rng.random() < 0.5}
        F[f"random[{seed}]"] = frozenset(n for n in names if module_of(n) in on)
    return F


FAMILY_NAMES = tuple(family([dict(name=n, kind=0) for n in ()]).keys())        # the names alone (the selections are empty without a table)
# the other arithmetic modes (fp32_split with every split route forced, bf16) run this part of the family
REDUCED = ("norms", "matrices", "fc2_only", "local_conv", "mbconv_c2", "merge_c2", "pe2", "stage1_only", "random[0]", "random[1]", "random[2]")


def policy_mask(table, policy):
    """The two masks the suite already trusts, as name sets: "all", "freeze" (TinyViTAdapter.freeze_all_but_last_stage)."""
    names = param_names(table)
    if policy == "all":
        return frozenset(names)
    assert policy == "freeze", policy
    return frozenset(n for n in names if not n.startswith(("stages.0.", "stages.1.", "stages.2.")))


def mask_of(table, policy):
    return policy_mask(table, policy) if policy in ("all", "freeze") else family(table)[policy]


def to_bytes(table, mask):
    """One byte per tensor of the table, as TinyVitBackbone.trainable_mask() / gg_tinyvit_* take it."""
    return bytes(int(t["kind"] == 0 and t["name"] in mask) for t in table)


def apply(bb, mask):
    """Set requires_grad of a FlatStore's parameters to the mask (a family / policy name or a name set); returns the name set."""
    if isinstance(mask, str):
        mask = mask_of(bb.table, mask)
    unknown = set(mask) - set(bb._params)
    assert not unknown, sorted(unknown)[:4]
    for n, p in bb._params.items():
        p.requires_grad_(n in mask)
        if n not in mask:
            p.grad = None
    return mask


# ------------------------------------------------------------------------------------------- CLIP vision tower
CLIP_RANDOM_SEEDS = (0, 1, 2)


def clip_family(names, num_layers):
    """CLIP tower masks over its tensor names (HF names without the ``vision_model.`` prefix).  post_layernorm is not on the path of the
    pooled mean / last hidden state (its gradient is zero): no mask trains it."""
    names = [n for n in names if not n.startswith("post_layernorm")]
    mid = num_layers // 2
    F = {}
    F["biases"] = _sel(names, r"\.bias$")
    F["layernorms"] = _sel(names, r"layer_norm[12]\.", r"^pre_layrnorm\.")
    F["middle_layer"] = _sel(names, rf"^encoder\.layers\.{mid}\.")
    F["position_embedding"] = _sel(names, r"position_embedding")
    F["class_embedding"] = _sel(names, r"class_embedding")
    F["patch_embedding"] = _sel(names, r"patch_embedding")
    F["layernorm_weights"] = _sel(names, r"layer_norm[12]\.weight$", r"^pre_layrnorm\.weight$")       # half pairs: the dump-row path
    for seed in CLIP_RANDOM_SEEDS:
        rng = _random.Random(2000 + seed)
        F[f"random[{seed}]"] = frozenset(n for n in names if rng.random() < 0.5)
    return F
