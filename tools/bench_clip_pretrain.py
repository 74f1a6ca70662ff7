"""One frozen-backbone step of the CLIP contrastive pre-training stage (pretrain_idun.py:205-300 with PRETRAIN_ARGS, config.py:105-136) at ViT-L/14-336 dimensions
with random weights: text tower forward, vision tower forward (both frozen: inference schedules), then the head -- projections, gg_clip_contrastive with its
backward, the visual_projection weight gradient, clip_grad_norm_(1.0) and the AdamW step on visual_projection + logit_scale.

Prints one JSON line per case: wall-clock milliseconds per step (HIP events around the whole step, profiler off) and, from a separate profiled step (gg_prof_*:
HIP events around every launch), the kernel time of each of the three parts split by launch class.  The reference runs 960 pairs per device (gradient
accumulation 8); --batch sets the pairs per step here.
    python tools/bench_clip_pretrain.py --batch 96 --precision fp32_split [--model openai/clip-vit-large-patch14-336] [--steps 5 --warmup 2] [--out FILE.jsonl]

--train-text {top,all}: the fine-tune of both towers instead (CLIPModel(train_text=True)): `top` trains the last encoder layer of each tower, final_layer_norm /
post_layernorm, both projections and logit_scale; `all` trains everything.  The profiled step then also times the two towers' backward passes (text_backward,
vision_backward) and, from separate launches, gg_attention_causal_bwd against the non-causal gg_attention_flash_bwd on the text tower's attention shape."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ["gemm", "attention", "dwconv", "norm", "head", "optimizer", "move"]


def class_ms(lib):
    """{class: ms} of the launches logged since the last reset (split-product GEMMs are counted with the GEMMs)."""
    out = {}
    cat, ms = C.c_int(), C.c_double()
    for i in range(lib.gg_prof_count()):
        lib.gg_prof_record(i, C.byref(cat), C.byref(ms), None, None)
        k = CLASSES[cat.value & 15]
        out[k] = out.get(k, 0.0) + ms.value
    return {k: round(v, 4) for k, v in out.items()}


def attention_bwd_us(L, B, H, T, dtype, iters=20):
    """Microseconds per launch (HIP events around `iters` back-to-back launches after 3 warm-up ones; the buffers, a few MB, stay in the cache in both cases) of
    gg_attention_causal_bwd and of the non-causal gg_attention_flash_bwd on the same (B, H, T, 64) buffers, each behind its own forward."""
    lib = L.lib()
    dt = torch.bfloat16 if dtype == 0 else torch.float32
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * T, 3 * H * 64, generator=g).cuda().to(dt)
    dout = torch.randn(B * T, H * 64, generator=g).cuda().to(dt)
    res = {}
    for name, fwd, bwd in (("causal", lib.gg_attention_causal_fwd, lib.gg_attention_causal_bwd), ("noncausal", lib.gg_attention_flash_fwd, lib.gg_attention_flash_bwd)):
        out, lse, dqkv = torch.empty(B * T, H * 64, dtype=dt, device="cuda"), torch.empty(B * T, H, device="cuda"), torch.empty_like(qkv)
        at = L.AttnArgs()
        at.qkv, at.ld, at.q_off, at.k_off, at.v_off, at.head_stride, at.head_dim = qkv.data_ptr(), 3 * H * 64, 0, H * 64, 2 * H * 64, 64, 64
        at.num_heads, at.num_windows, at.tokens_per_window, at.window_size, at.scale = H, B, T, 0, 0.125
        at.out, at.ldo, at.lse, at.dout, at.lddo, at.dqkv = out.data_ptr(), H * 64, lse.data_ptr(), dout.data_ptr(), H * 64, dqkv.data_ptr()
        L.check(fwd(C.byref(at), dtype, L.stream()), name)
        for _ in range(3):
            L.check(bwd(C.byref(at), dtype, L.stream()), name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            bwd(C.byref(at), dtype, L.stream())
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) / iters * 1e3, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="openai/clip-vit-large-patch14-336")
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--precision", default="fp32_split", choices=["fp32", "fp32_split", "bf16"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train-text", default=None, choices=["top", "all"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.optim import AdamW
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel
    L.require_gpu()
    lib = L.lib()
    m = CLIPModel(a.model, precision=a.precision, train_text=a.train_text is not None).cuda()
    for p in m.parameters():                                   # freeze_backbone_keep_head
        p.requires_grad = False
    m.logit_scale.requires_grad = True
    m.visual_projection.weight.requires_grad = True
    if a.train_text:
        tl, vl = m.config.text_config.num_layers - 1, m.config.vision_config.num_layers - 1
        top = (f"text_model.encoder.layers.{tl}.", f"vision_model.encoder.layers.{vl}.", "text_model.final_layer_norm", "vision_model.post_layernorm", "text_projection")
        for n, p in m.named_parameters():
            if a.train_text == "all" or n.startswith(top):
                p.requires_grad = True
    opt = AdamW(m, lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=1e-3)
    g = torch.Generator().manual_seed(0)
    S = m.config.vision_config.image_size
    ids = torch.randint(0, 49406, (a.batch, a.tokens), generator=g).cuda()
    ids[:, -1] = 49407
    pix = torch.randn(a.batch, 3, S, S, generator=g).cuda()

    def step():
        out = m(input_ids=ids, pixel_values=pix, return_loss=True)
        out.loss.backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad()
        return out.loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    wall = e0.elapsed_time(e1) / a.steps

    # one profiled step, part by part
    parts = {}
    lib.gg_prof_enable(1)
    lib.gg_prof_reset()
    pooled_txt = m._text_pooled(ids)
    torch.cuda.synchronize()
    parts["text_tower"] = class_ms(lib)
    lib.gg_prof_reset()
    pooled_img = m._image_pooled(pix)
    torch.cuda.synchronize()
    parts["vision_tower"] = class_ms(lib)
    lib.gg_prof_reset()
    from geoguessr_ai_amd.pretrain.clip_model import _HeadFn
    if a.train_text:          # the head's backward stops at the pooled outputs; each tower's backward is then timed on its own
        pi, pt = pooled_img.detach().requires_grad_(), pooled_txt.detach().requires_grad_()
        out = _HeadFn.apply(m, pi, pt, m.visual_projection.weight, m.text_projection.weight, m.logit_scale, True, True)
        out[0].backward()
        torch.cuda.synchronize()
        parts["contrastive_head"] = class_ms(lib)
        lib.gg_prof_reset()
        pooled_txt.backward(pt.grad)
        torch.cuda.synchronize()
        parts["text_backward"] = class_ms(lib)
        lib.gg_prof_reset()
        pooled_img.backward(pi.grad)
        torch.cuda.synchronize()
        parts["vision_backward"] = class_ms(lib)
        lib.gg_prof_reset()
        opt.clip_grad_norm_(1.0)
        opt.step()
        torch.cuda.synchronize()
        parts["optimizer"] = class_ms(lib)
    else:
        out = _HeadFn.apply(m, pooled_img, pooled_txt, m.visual_projection.weight, m.text_projection.weight, m.logit_scale, True, True)
        out[0].backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        torch.cuda.synchronize()
        parts["contrastive_head"] = class_ms(lib)
    lib.gg_prof_enable(0)
    lib.gg_prof_reset()
    tot = {k: round(sum(v.values()), 4) for k, v in parts.items()}
    rec = dict(tool="bench_clip_pretrain", model=a.model, precision=a.precision, pairs=a.batch, tokens=a.tokens, steps=a.steps, warmup=a.warmup,
               wall_ms_per_step=round(wall, 3), pairs_per_s=round(a.batch / wall * 1e3, 1), kernel_ms=tot, kernel_ms_by_class=parts,
               text_over_vision=round(tot["text_tower"] / tot["vision_tower"], 4), loss=round(float(loss), 5), device=torch.cuda.get_device_name(0))
    if a.train_text:
        rec["train_text"] = a.train_text
        rec["attention_bwd_us"] = attention_bwd_us(L, a.batch, m.config.text_config.num_heads, a.tokens, {"bf16": 0, "fp32": 1, "fp32_split": 3}[a.precision])
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
