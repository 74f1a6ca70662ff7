#!/usr/bin/env python3
"""fp16 against fp8 (e4m3) inference of the frozen CLIP vision tower, in one process on one device: the c4 shape (ViT-B/32, 1024 images) and ViT-L/14-336 at
batch 64.  Both towers hold the same seeded weights and see the same batch; rounds alternate the two precisions, every round is timed with device events around
`--calls` forwards after a warm-up of every shape, and a case reports the median and the minimum over the rounds.  One JSON line per case is appended to
profiles/clip_fp8_bench.jsonl (--out).

--trace CASE runs the fp8 tower of one case alone for a few calls and writes nothing: the program to put behind `rocprofv3 --kernel-trace --stats --` for the
per-kernel split (the share of the stand-alone quantisation passes, quant_rows_kernel)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

CASES = {"c4": ("openai/clip-vit-base-patch32", 1024), "l14": ("openai/clip-vit-large-patch14-336", 64)}


def tower_of(name, precision, seed=0):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    t = CLIPVisionTower(name, seed=seed, precision=precision).cuda().eval()
    for p in t.parameters():
        p.requires_grad = False
    return t


def timed(tower, x, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        tower(pixel_values=x, return_last_hidden=False)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c4,l14")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "clip_fp8_bench.jsonl"))
    ap.add_argument("--trace", default=None, choices=sorted(CASES))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    if args.trace:
        name, batch = CASES[args.trace]
        t = tower_of(name, "fp8")
        x = torch.randn(batch, 3, t.cfg.image_size, t.cfg.image_size, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        with torch.no_grad():
            for _ in range(4):
                t(pixel_values=x, return_last_hidden=False)
        torch.cuda.synchronize()
        return
    for case in args.cases.split(","):
        name, batch = CASES[case]
        towers = {p: tower_of(name, p) for p in ("fp16", "fp8")}
        S = towers["fp16"].cfg.image_size
        x = torch.randn(batch, 3, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        ms = {p: [] for p in towers}
        with torch.no_grad():
            out = {p: t(pixel_values=x, return_last_hidden=False).pooled_mean.double() for p, t in towers.items()}
            for p, t in towers.items():
                for _ in range(args.warmup):
                    t(pixel_values=x, return_last_hidden=False)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for p, t in towers.items():
                    ms[p].append(timed(t, x, args.calls))
        cos = torch.nn.functional.cosine_similarity(out["fp8"], out["fp16"], dim=-1)
        med = {p: statistics.median(v) for p, v in ms.items()}
        line = dict(case=case, model=name, batch=batch, rounds=args.rounds, calls_per_round=args.calls,
                    fp16_ms_median=round(med["fp16"], 4), fp16_ms_min=round(min(ms["fp16"]), 4), fp8_ms_median=round(med["fp8"], 4), fp8_ms_min=round(min(ms["fp8"]), 4),
                    fp16_over_fp8_median=round(med["fp16"] / med["fp8"], 4), fp16_over_fp8_min=round(min(ms["fp16"]) / min(ms["fp8"]), 4),
                    fp16_ms_rounds=[round(v, 3) for v in ms["fp16"]], fp8_ms_rounds=[round(v, 3) for v in ms["fp8"]],
                    pooled_cos_fp8_vs_fp16_min=round(float(cos.min()), 6), device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:16])
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del towers, x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
