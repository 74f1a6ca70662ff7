#!/usr/bin/env python3
"""The long-sequence attention forward on the 16-bit MFMA (gg_attention_flash16_fwd, include/gg_attn16.h) against the f32-MFMA online-softmax kernel it can
replace (gg_attention_flash_fwd, dtype 2 / 0), in one process on one device, on tools/bench_clip_fp8.py's scheme: rounds alternate the arms, every round is timed
with device events around `--calls` launches after a warm-up of every arm, a case reports the median, the minimum and every round.

* kernel cases: 64 sequences x 16 heads x 577 tokens (CLIP ViT-L/14-336 at batch 64) and x 257 tokens (just beyond the register-resident kernels), fp16 and bf16
  storage, random N(0, 1) q / k / v in the tower's [q | k | v] layout;
* tower cases: the frozen ViT-L/14-336 tower at 64 images in fp16, fp8 and bf16, library switch off and on (gg_clip_set_attention16).

One JSON line per case is appended to profiles/attention16_bench.jsonl (--out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

L14 = "openai/clip-vit-large-patch14-336"
KERNEL_CASES = [(64, 16, 577), (64, 16, 257)]
TOWER_BATCH = 64
MFMA16_ROOF_TFLOPS = 2500.0


def events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def ab(arms, rounds, calls, warmup):
    """{arm: [ms per call, one figure per round]}: warm every arm, then alternate them round by round."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(events(fn, calls))
    return ms


def stats(ms):
    return {k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), rounds=[round(x, 4) for x in v]) for k, v in ms.items()}


def spread(v):
    """(max - min) / median of one arm's rounds."""
    return (max(v) - min(v)) / statistics.median(v)


def kernel_case(L, B, H, N, dtype, args):
    st = torch.float16 if dtype == 2 else torch.bfloat16
    D = H * 64
    qkv = torch.randn(B * N, 3 * D, device="cuda", generator=torch.Generator("cuda").manual_seed(1)).to(st)
    outs = {k: torch.empty(B * N, D, dtype=st, device="cuda") for k in ("f32_pipe", "mfma16")}
    a = {}
    for k in outs:
        a[k] = L.AttnArgs()
        a[k].qkv, a[k].ld, a[k].q_off, a[k].k_off, a[k].v_off, a[k].head_stride, a[k].head_dim = qkv.data_ptr(), 3 * D, 0, D, 2 * D, 64, 64
        a[k].num_heads, a[k].num_windows, a[k].tokens_per_window, a[k].window_size, a[k].scale = H, B, N, 0, 0.125
        a[k].out, a[k].ldo = outs[k].data_ptr(), D
    lib, s = L.lib(), L.stream()
    arms = {"f32_pipe": lambda: L.check(lib.gg_attention_flash_fwd(C.byref(a["f32_pipe"]), dtype, s), "gg_attention_flash_fwd"),
            "mfma16": lambda: L.check(lib.gg_attention_flash16_fwd(C.byref(a["mfma16"]), dtype, s), "gg_attention_flash16_fwd")}
    ms = ab(arms, args.rounds, args.calls, args.warmup)
    diff = float((outs["mfma16"].double() - outs["f32_pipe"].double()).abs().max())
    med = {k: statistics.median(v) for k, v in ms.items()}
    flop = 4.0 * B * H * N * N * 64
    return dict(case="kernel", storage="fp16" if dtype == 2 else "bf16", sequences=B, heads=H, tokens=N, ms=stats(ms),
                f32_pipe_over_mfma16_median=round(med["f32_pipe"] / med["mfma16"], 4), spread={k: round(spread(v), 4) for k, v in ms.items()},
                tflops={k: round(flop / (med[k] * 1e-3) / 1e12, 1) for k in med}, mfma16_frac_of_roof=round(flop / (med["mfma16"] * 1e-3) / 1e12 / MFMA16_ROOF_TFLOPS, 4),
                max_abs_diff_between_arms=diff)


def tower_case(L, precision, batch, args):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    t = CLIPVisionTower(L14, seed=0, precision=precision).cuda().eval()
    for p in t.parameters():
        p.requires_grad = False
    x = torch.randn(batch, 3, 336, 336, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    lib = L.lib()

    def arm(on):
        def run():
            lib.gg_clip_set_attention16(on)
            return t(pixel_values=x, return_last_hidden=False).pooled_mean
        return run
    arms = {"off": arm(0), "on": arm(1)}
    with torch.no_grad():
        pooled = {k: fn().double() for k, fn in arms.items()}
        n = lib.gg_attention_flash16_calls()
        arms["on"]()
        per_forward = lib.gg_attention_flash16_calls() - n
        ms = ab(arms, args.rounds, args.calls, args.warmup)
    lib.gg_clip_set_attention16(0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    cos = torch.nn.functional.cosine_similarity(pooled["on"], pooled["off"], dim=-1)
    return dict(case="tower", model=L14, precision=precision, batch=batch, flash16_launches_per_forward=per_forward, ms=stats(ms),
                off_over_on_median=round(med["off"] / med["on"], 4), spread={k: round(spread(v), 4) for k, v in ms.items()}, pooled_cos_on_vs_off_min=round(float(cos.min()), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="the kernel cases alone (re-measuring the kernel beside a change that leaves the tower as it is)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention16_bench.jsonl"))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    lines = []
    for B, H, N in KERNEL_CASES:
        for dtype in (2, 0):
            lines.append(kernel_case(L, B, H, N, dtype, args))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    for precision in (() if args.kernel_only else ("fp16", "fp8", "bf16")):
        lines.append(tower_case(L, precision, TOWER_BATCH, args))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(dict(line, rounds=args.rounds, calls_per_round=args.calls, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:16])) + "\n")


if __name__ == "__main__":
    main()
