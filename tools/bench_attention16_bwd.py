#!/usr/bin/env python3
"""The long-sequence attention backward on the 16-bit MFMA (gg_attention_flash16_bwd, include/gg_attn16b.h) against the f32-MFMA streaming backward it can replace
(gg_attention_flash_bwd, dtype 0, with the dS scratch exactly as the CLIP tower passes it), in one process on one device, on tools/bench_attention16.py's scheme:
rounds alternate the arms, every round is timed with device events around `--calls` launches after a warm-up of every arm, a case reports the median, the minimum
and every round.

* kernel cases: 64 sequences x 16 heads x 577 tokens (CLIP ViT-L/14-336 at batch 64) and x 257 tokens (just beyond the single-pass kernel), bf16 storage, random
  N(0, 1) q / k / v / dout in the tower's [q | k | v] layout, out and lse from gg_attention_flash16_fwd; the new kernel's fraction of the 16-bit MFMA roof on the
  declared 10 N^2 D flops;
* tower cases: the ViT-L/14-336 fine-tune step of tools/bench_recompute.py (SuperGuessr head, AdamW, every tensor trainable, bf16) at the largest batch of its
  `--cases clip` that fits, library switch off and on (gg_clip_set_attention16_train), without and with recompute; the attention kernels' share of the step from
  one profiled step per arm (gg_prof_read, category 1).

One JSON line per case is appended to profiles/attention16_bwd_bench.jsonl (--out)."""
import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_attention16 import L14, KERNEL_CASES, MFMA16_ROOF_TFLOPS, ab, spread, stats


def kernel_case(L, B, H, N, args):
    st, D = torch.bfloat16, H * 64
    g = torch.Generator("cuda").manual_seed(1)
    qkv = torch.randn(B * N, 3 * D, device="cuda", generator=g).to(st)
    dout = torch.randn(B * N, D, device="cuda", generator=g).to(st)
    out, lse = torch.empty(B * N, D, dtype=st, device="cuda"), torch.empty(B * N, H, device="cuda")
    lib, s = L.lib(), L.stream()
    ds = torch.empty(lib.gg_attention_flash_ds_scratch_floats(B, H, N), device="cuda")
    dq = {k: torch.zeros_like(qkv) for k in ("f32_pipe", "mfma16")}
    a = {}
    for k in dq:
        a[k] = L.AttnArgs()
        a[k].qkv, a[k].ld, a[k].q_off, a[k].k_off, a[k].v_off, a[k].head_stride, a[k].head_dim = qkv.data_ptr(), 3 * D, 0, D, 2 * D, 64, 64
        a[k].num_heads, a[k].num_windows, a[k].tokens_per_window, a[k].window_size, a[k].scale = H, B, N, 0, 0.125
        a[k].out, a[k].ldo, a[k].lse = out.data_ptr(), D, lse.data_ptr()
        a[k].dout, a[k].lddo, a[k].dqkv = dout.data_ptr(), D, dq[k].data_ptr()
    a["f32_pipe"].ds_scratch = ds.data_ptr()
    L.check(lib.gg_attention_flash16_fwd(C.byref(a["mfma16"]), 0, s), "gg_attention_flash16_fwd")
    arms = {"f32_pipe": lambda: L.check(lib.gg_attention_flash_bwd(C.byref(a["f32_pipe"]), 0, s), "gg_attention_flash_bwd"),
            "mfma16": lambda: L.check(lib.gg_attention_flash16_bwd(C.byref(a["mfma16"]), 0, s), "gg_attention_flash16_bwd")}
    ms = ab(arms, args.rounds, args.calls, args.warmup)
    diff = float((dq["mfma16"].double() - dq["f32_pipe"].double()).abs().max())
    med = {k: statistics.median(v) for k, v in ms.items()}
    flop = 10.0 * B * H * N * N * 64
    sp = {k: spread(v) for k, v in ms.items()}
    return dict(case="kernel", storage="bf16", sequences=B, heads=H, tokens=N, ds_scratch_MB=round(ds.numel() * 4 / 2 ** 20, 1), ms=stats(ms),
                f32_pipe_over_mfma16_median=round(med["f32_pipe"] / med["mfma16"], 4), spread={k: round(v, 4) for k, v in sp.items()},
                faster_by_more_than_the_spread=bool(min(ms["f32_pipe"]) > max(ms["mfma16"])),
                tflops_declared={k: round(flop / (med[k] * 1e-3) / 1e12, 1) for k in med},
                mfma16_frac_of_roof=round(flop / (med["mfma16"] * 1e-3) / 1e12 / MFMA16_ROOF_TFLOPS, 4), max_abs_diff_between_arms=diff)


def tower_case(L, recompute, images, args):
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.optim import AdamW
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    lib = L.lib()
    gc.collect(); torch.cuda.empty_cache()
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = CLIPVisionTower(L14, precision="bf16", gradient_checkpointing=recompute)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True, serving=False).cuda().train()
    opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(images // 4, 4, 3, 336, 336, device="cuda", generator=g)
    lab = torch.stack([torch.rand(images // 4, device="cuda", generator=g) * 360 - 180, torch.rand(images // 4, device="cuda", generator=g) * 180 - 90], 1)

    def arm(on):
        def run():
            prev = lib.gg_clip_set_attention16_train(on)          # the library switch: read when the forward and the backward are enqueued
            try:
                out = model(pixel_values=x, labels=lab)
                out.loss.backward()
            finally:
                lib.gg_clip_set_attention16_train(prev)
            opt.step()
            opt.zero_grad()
        return run
    arms = {"off": arm(0), "on": arm(1)}
    ms = ab(arms, args.tower_rounds, 1, 1)
    med = {k: statistics.median(v) for k, v in ms.items()}
    attn, calls = {}, {}
    for k, fn in arms.items():          # one profiled step per arm: the attention category's share of the kernels' time
        n = (lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls())
        lib.gg_prof_reset(); lib.gg_prof_enable(1)
        fn()
        torch.cuda.synchronize()
        lib.gg_prof_enable(0)
        cat = {}
        for c in range(8):
            t, nl, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            L.check(lib.gg_prof_read(c, C.byref(t), C.byref(nl), C.byref(fl), C.byref(by)), "gg_prof_read")
            cat[c] = t.value
        lib.gg_prof_reset()
        attn[k] = dict(attention_ms=round(cat[1], 2), all_categories_ms=round(sum(cat.values()), 2), attention_share_of_kernels=round(cat[1] / sum(cat.values()), 4),
                       attention_share_of_step=round(cat[1] / med[k], 4))
        calls[k] = (lib.gg_attention_flash16_calls() - n[0], lib.gg_attention_flash16_bwd_calls() - n[1])
    res = dict(case="tower", model=L14, precision="bf16", policy="all", recompute=int(recompute), images=images, ms_per_step=stats(ms),
               off_over_on_median=round(med["off"] / med["on"], 4), spread={k: round(spread(v), 4) for k, v in ms.items()}, attention=attn,
               flash16_fwd_and_bwd_calls_per_step=calls)
    del model, base, opt, x
    gc.collect(); torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tower-rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=0, help="tower batch (a multiple of 4); 0: the largest of tools/bench_recompute.py --cases clip that fits")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--tower-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention16_bwd_bench.jsonl"))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(dict(line, rounds=args.rounds, calls_per_round=args.calls, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:16])) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for B, H, N in (() if args.tower_only else KERNEL_CASES):
        emit(kernel_case(L, B, H, N, args))
        torch.cuda.empty_cache()
    if not args.kernel_only:
        images = args.images
        if not images:
            from tools.bench_recompute import clip_largest_panoramas
            images = 4 * clip_largest_panoramas("bf16")
        for recompute in (False, True):
            emit(tower_case(L, recompute, images, args))


if __name__ == "__main__":
    main()
