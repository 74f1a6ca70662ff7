#!/usr/bin/env python3
"""The two-pass (streaming) attention backward of csrc/attention_flash.hip -- flash_bwd_dq_kernel + flash_bwd_dkv_kernel, and with a dS scratch
flash_bwd_dkv_kernel<.., STORE_DS> + flash_bwd_dq_ds_kernel -- at the shapes that take it: 24 x 24 windows of head dim 32 with bias and dbias (tiny_vit_21m_384
stage 2, 16 images x 12 heads), 577 tokens of head dim 64 (CLIP ViT-L/14-336, 16 images x 16 heads) and 1024 linear tokens of head dim 32 without a bias table
(no model's shape: the one at which LDS leaves the dQ kernel's register count to decide its occupancy), f32 and bf16 storage.  Every round is timed with device
events around `--calls` backward calls after a warm-up; a case reports the median, the minimum and every round.  One process times one library (GG_LIB): to
compare two builds, run the tool once per build, alternating, and compare the medians against the spread between runs of the same build.

One JSON line per case is appended to --out (default profiles/attention_bwd_streaming_bench.jsonl), tagged with --tag."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

# (name, layout, tokens, head dim, ws, map side, windows, heads)
CASES = [("win24_hd32", "tinyvit", 576, 32, 24, 24, 16, 12), ("lin577_hd64", "clip", 577, 64, 0, 0, 16, 16), ("lin1024_hd32", "clip", 1024, 32, 0, 0, 16, 12)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention_bwd_streaming_bench.jsonl"))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L, ops
    from tests import attention_cases as A
    L.require_gpu()
    for name, layout, N, hd, ws, map_hw, W, H in CASES:
        for storage in ("f32", "bf16"):
            for handoff in ((False, True) if storage == "f32" else (False,)):
                st = A.STORAGE[storage]
                g = torch.Generator().manual_seed(N + hd)
                q_off, k_off, v_off, hs = A.columns(layout, H, hd)
                qkv = torch.randn(W * N, 3 * H * hd, generator=g).to(st).cuda()
                dout = torch.randn(W * N, H * hd, generator=g).to(st).cuda()
                table = (0.5 * torch.randn(H, ws * ws, generator=g)).cuda() if ws else None
                kw = dict(num_windows=W, tokens_per_window=N, num_heads=H, head_dim=hd, q_off=q_off, k_off=k_off, v_off=v_off, head_stride=hs, window_size=ws,
                          map_h=map_hw, map_w=map_hw, bias_table=table)
                out, lse = ops.attention_flash(qkv, want_lse=True, **kw)
                fn = lambda: ops.attention_flash(qkv, dout=dout, out=out, lse=lse, want_dbias=table is not None, ds_handoff=handoff, **kw)
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                ms = []
                for _ in range(args.rounds):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.calls):
                        fn()
                    b.record()
                    b.synchronize()
                    ms.append(a.elapsed_time(b) / args.calls)
                rec = dict(case=name, storage=storage, ds_handoff=handoff, windows=W, heads=H, tokens=N, head_dim=hd, tag=args.tag,
                           ms=dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4), rounds=[round(x, 4) for x in ms]))
                print(json.dumps(rec), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
