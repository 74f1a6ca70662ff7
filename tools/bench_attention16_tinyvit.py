#!/usr/bin/env python3
"""The 16-bit-MFMA window attention forward beyond 256 tokens (gg_attention_flash16_win_fwd, include/gg_attn16w.h) against the f32-MFMA online-softmax kernel it
can replace (gg_attention_flash_fwd, dtype 0), in one process on one device, on tools/bench_attention16.py's scheme: rounds alternate the arms, every round is
timed with device events around `--calls` launches after a warm-up of every arm, a case reports the median, the minimum and every round.

* kernel cases: 64 images x 12 heads, head dim 32, with the relative-position bias, one window per image of 1024 tokens (ws 32: tiny_vit_21m_512 stage 2) and of
  576 tokens (ws 24: tiny_vit_21m_384), bf16 storage, random N(0, 1) q / k / v in TinyViT's per-head [q | k | v] layout, table N(0, 0.5);
* model cases: the bf16 eval forward of tiny_vit_21m_512 and tiny_vit_21m_384, library switch off and on (gg_tinyvit_set_attention16), at batch 64 (eager) and at
  batch 4 (one serving panorama: launch-bound, the captured graph of each setting is replayed).

Gates, each against the other arm of the same case: the new kernel is no slower than flash_fwd_kernel at both shapes (medians); the batch-64 forward with the
switch on is no slower than with it off.  One JSON line per case is appended to profiles/attention16_tinyvit_bench.jsonl (--out); the exit status is 1 when a
gate failed (the records are written either way)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
import torch

from bench_attention16 import MFMA16_ROOF_TFLOPS, ab, spread, stats

KERNEL_CASES = [(64, 12, 32), (64, 12, 24)]          # images (one window each), heads, window side
MODEL_CASES = [("tiny_vit_21m_512", 64), ("tiny_vit_21m_512", 4), ("tiny_vit_21m_384", 64), ("tiny_vit_21m_384", 4)]


def kernel_case(L, B, H, ws, args):
    N, D = ws * ws, 32
    g = torch.Generator("cuda").manual_seed(1)
    qkv = torch.randn(B * N, 3 * H * D, device="cuda", generator=g).to(torch.bfloat16)
    table = (0.5 * torch.randn(H, N, device="cuda", generator=g)).contiguous()
    outs = {k: torch.empty(B * N, H * D, dtype=torch.bfloat16, device="cuda") for k in ("f32_pipe", "mfma16")}
    a = {}
    for k in outs:
        a[k] = L.AttnArgs()
        a[k].qkv, a[k].ld, a[k].q_off, a[k].k_off, a[k].v_off, a[k].head_stride, a[k].head_dim = qkv.data_ptr(), 3 * H * D, 0, D, 2 * D, 3 * D, D
        a[k].num_heads, a[k].num_windows, a[k].tokens_per_window, a[k].window_size, a[k].map_h, a[k].map_w = H, B, N, ws, ws, ws
        a[k].scale, a[k].bias_table = D ** -0.5, table.data_ptr()
        a[k].out, a[k].ldo = outs[k].data_ptr(), H * D
    lib, s = L.lib(), L.stream()
    arms = {"f32_pipe": lambda: L.check(lib.gg_attention_flash_fwd(C.byref(a["f32_pipe"]), 0, s), "gg_attention_flash_fwd"),
            "mfma16": lambda: L.check(lib.gg_attention_flash16_win_fwd(C.byref(a["mfma16"]), 0, s), "gg_attention_flash16_win_fwd")}
    ms = ab(arms, args.rounds, args.calls, args.warmup)
    diff = float((outs["mfma16"].double() - outs["f32_pipe"].double()).abs().max())
    med = {k: statistics.median(v) for k, v in ms.items()}
    flop = 4.0 * B * H * N * N * D
    return dict(case="kernel", storage="bf16", images=B, heads=H, head_dim=D, window=ws, tokens=N, bias=True, ms=stats(ms),
                f32_pipe_over_mfma16_median=round(med["f32_pipe"] / med["mfma16"], 4), spread={k: round(spread(v), 4) for k, v in ms.items()},
                tflops={k: round(flop / (med[k] * 1e-3) / 1e12, 1) for k in med}, mfma16_frac_of_roof=round(flop / (med["mfma16"] * 1e-3) / 1e12 / MFMA16_ROOF_TFLOPS, 4),
                max_abs_diff_between_arms=diff, gate="mfma16 <= f32_pipe (median)", gate_ok=bool(med["mfma16"] <= med["f32_pipe"]))


def graph_stats(L):
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    L.lib().gg_graph_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value


def model_case(L, name, batch, args):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    torch.manual_seed(0)
    m = TinyViTAdapter(name, pretrained=False, precision="bf16", drop_path_rate=0.0, seed=0).cuda().eval()
    bb = m.backbone
    x = torch.randn(batch, 3, bb.img_size, bb.img_size, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    lib = L.lib()
    lib.gg_graph_clear()

    def arm(on):
        def run():
            lib.gg_tinyvit_set_attention16(on)
            return bb.forward_hip(x, False)          # (the result is dropped by the caller: the next call gets the same address, so a captured graph replays)
        return run
    arms = {"off": arm(0), "on": arm(1)}
    with torch.no_grad():
        pooled = {k: fn().double() for k, fn in arms.items()}
        n = lib.gg_attention_flash16_win_calls()
        arms["on"]()
        per_forward = lib.gg_attention_flash16_win_calls() - n          # (counted on an eager or capturing call; a replay enqueues the captured launches)
        r0 = graph_stats(L)[1]
        ms = ab(arms, args.rounds, args.model_calls, args.warmup)
        replays = graph_stats(L)[1] - r0
    lib.gg_tinyvit_set_attention16(0)
    lib.gg_graph_clear()
    med = {k: statistics.median(v) for k, v in ms.items()}
    cos = torch.nn.functional.cosine_similarity(pooled["on"], pooled["off"], dim=-1)
    rec = dict(case="model", model=name, precision="bf16", batch=batch, img_size=bb.img_size, flash16_win_launches_per_forward=per_forward, graph_replays=replays, ms=stats(ms),
               off_over_on_median=round(med["off"] / med["on"], 4), spread={k: round(spread(v), 4) for k, v in ms.items()}, pooled_cos_on_vs_off_min=round(float(cos.min()), 6))
    if batch == 64:
        rec.update(gate="on <= off (median)", gate_ok=bool(med["on"] <= med["off"]))
    del m, bb
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--model-calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention16_tinyvit_bench.jsonl"))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    lines = []
    for B, H, ws in KERNEL_CASES:
        lines.append(kernel_case(L, B, H, ws, args))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    for name, batch in ([] if args.kernel_only else MODEL_CASES):
        lines.append(model_case(L, name, batch, args))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            calls = args.calls if line["case"] == "kernel" else args.model_calls
            f.write(json.dumps(dict(line, rounds=args.rounds, calls_per_round=calls, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:16])) + "\n")
    failed = [l for l in lines if l.get("gate_ok") is False]
    for l in failed:
        print(f"GATE FAILED: {l['case']} {l.get('model', '')} {l.get('tokens', l.get('batch'))}: {l['gate']}", flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
