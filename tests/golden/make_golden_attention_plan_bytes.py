"""Writes tests/golden/attention_plan_bytes_parent.json: every workspace total whose plan depends on the attention routes, at batch 8 --
  * gg_tinyvit_workspace_bytes_masked of the five variants at their own input size and at 224, 256, 384 and 512 (sizes the attention windows do not divide run
    padded), inference and training, in every arithmetic mode, training with the masks None and freeze_all_but_last_stage and activation recompute off and on;
  * gg_clip_workspace_bytes of ViT-B/32, ViT-L/14 and ViT-L/14-336 in every act_dtype, inference and (where the mode trains) training with every tensor and with
    the last two layers trainable, recompute off and on;
  * gg_clip_text_workspace_bytes and gg_clip_text_train_workspace_bytes of the two text towers at 77 and 20 tokens.
Run ONCE with the build of the commit in front of the attention route struct (tests/test_attention_route_cpu.py holds later builds to these totals: the planners now
ask gg_attention_route where they repeated a predicate).  Host code: no GPU."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BATCH = 8
CLIP_TOWERS = {
    "vit_b32": dict(hidden_size=768, intermediate_size=3072, num_layers=12, num_heads=12, image_size=224, patch_size=32),
    "vit_l14": dict(hidden_size=1024, intermediate_size=4096, num_layers=24, num_heads=16, image_size=224, patch_size=14),
    "vit_l14_336": dict(hidden_size=1024, intermediate_size=4096, num_layers=24, num_heads=16, image_size=336, patch_size=14),
}
TEXT_TOWERS = {
    "text_b32": dict(hidden_size=512, intermediate_size=2048, num_layers=12, num_heads=8),
    "text_l14": dict(hidden_size=768, intermediate_size=3072, num_layers=12, num_heads=12),
}
CLIP_DTYPES = {"bf16": 0, "fp32": 1, "fp16": 2, "fp32_split": 3, "fp8": 8}


def _names(L, cfg, count, info):
    lib, out = L.lib(), []
    buf = C.create_string_buffer(256)
    off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int()
    shape = (C.c_int64 * 4)()
    for i in range(count(C.byref(cfg))):
        rc = info(C.byref(cfg), i, buf, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape)
        assert rc == 0, lib.gg_last_error().decode()
        out.append(buf.value.decode())
    return out


def plan_bytes():
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import VARIANTS, make_cfg, _tensor_table
    if not hasattr(C.CDLL(L.LIB_PATH), "gg_attention_route"):
        L.ATTN_ROUTE_SIGNATURES.clear()          # (GG_LIB names the build in front of the route struct: it has no report to bind)
    lib, out = L.lib(), {}

    def put(key, n):
        assert n > 0, (key, lib.gg_last_error().decode())
        out[key] = n

    for name in VARIANTS:
        for size in sorted({VARIANTS[name]["img_size"], 224, 256, 384, 512}):
            for precision in ("bf16", "fp32", "fp32_split"):
                cfg, _, _ = make_cfg(name, precision=precision, img_size=size)
                put(f"tinyvit/{name}/{size}/{precision}/inference", lib.gg_tinyvit_workspace_bytes_masked(C.byref(cfg), BATCH, 0, None))
                for rc in (0, 1):
                    cfg, _, _ = make_cfg(name, precision=precision, img_size=size, grad_checkpointing=bool(rc))
                    table = _tensor_table(cfg)
                    freeze = bytes(int(t["kind"] == 0 and not t["name"].startswith(("stages.0.", "stages.1.", "stages.2."))) for t in table)
                    for label, mask in (("none", None), ("freeze", freeze)):
                        put(f"tinyvit/{name}/{size}/{precision}/{label}/rc{rc}", lib.gg_tinyvit_workspace_bytes_masked(C.byref(cfg), BATCH, 1, mask))
    for tower, kw in CLIP_TOWERS.items():
        for precision, code in CLIP_DTYPES.items():
            c = L.ClipCfg()
            c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads = kw["hidden_size"], kw["intermediate_size"], kw["num_layers"], kw["num_heads"]
            c.image_size, c.patch_size, c.ln_eps, c.act_dtype, c.recompute = kw["image_size"], kw["patch_size"], 1e-5, code, 0
            put(f"clip/{tower}/{precision}/inference", lib.gg_clip_workspace_bytes(C.byref(c), BATCH, 0, None))
            if precision in ("fp16", "fp8"):
                continue          # inference-only modes
            names = _names(L, c, lib.gg_clip_num_tensors, lambda *a: lib.gg_clip_tensor_info(*a[:8]))
            top = tuple(f"encoder.layers.{i}." for i in (kw["num_layers"] - 2, kw["num_layers"] - 1))
            last2 = bytes(int(any(t in n for t in top) or "post_layernorm" in n) for n in names)
            assert 0 < sum(last2) < len(names), names[:8]
            for rc in (0, 1):
                c.recompute = rc
                for label, mask in (("all", None), ("last2", last2)):
                    put(f"clip/{tower}/{precision}/{label}/rc{rc}", lib.gg_clip_workspace_bytes(C.byref(c), BATCH, 1, mask))
    for tower, kw in TEXT_TOWERS.items():
        for precision, code in (("bf16", 0), ("fp32", 1), ("fp32_split", 3)):
            t = L.ClipTextCfg()
            t.hidden_size, t.intermediate_size, t.num_layers, t.num_heads = kw["hidden_size"], kw["intermediate_size"], kw["num_layers"], kw["num_heads"]
            t.vocab_size, t.max_positions, t.ln_eps, t.act_dtype = 49408, 77, 1e-5, code
            n_t = lib.gg_clip_text_num_tensors(C.byref(t))
            assert n_t > 0, lib.gg_last_error().decode()
            for tokens in (77, 20):
                put(f"text/{tower}/{precision}/{tokens}/inference", lib.gg_clip_text_workspace_bytes(C.byref(t), BATCH, tokens))
                put(f"text/{tower}/{precision}/{tokens}/train_all", lib.gg_clip_text_train_workspace_bytes(C.byref(t), BATCH, tokens, bytes([1] * n_t)))
    return out


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "attention_plan_bytes_parent.json")
    values = plan_bytes()
    with open(path, "w") as f:
        json.dump(values, f, indent=1, sort_keys=True)
    print("wrote", path, len(values))
