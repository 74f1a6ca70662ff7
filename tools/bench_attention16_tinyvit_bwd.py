#!/usr/bin/env python3
"""The window attention backward on the 16-bit MFMA (gg_attention_flash16_win_bwd, include/gg_attn16wb.h) against the f32-MFMA streaming backward it can replace
(gg_attention_bwd, which beyond 256 tokens is gg_attention_flash_bwd, dtype 0) on identical arguments, in one process on one device, on tools/bench_attention16.py's
scheme: rounds alternate the arms, every round is timed with device events around `--calls` launches after a warm-up of every arm, a case reports the median, the
minimum and every round.

* kernel cases: 64 windows x 12 heads x 1024 tokens (tiny_vit_21m_512 stage 2 at batch 64) and x 576 tokens (tiny_vit_21m_384), bf16 storage, random N(0, 1)
  q / k / v / dout in TinyViT's per-head [q | k | v] layout, a random table, out and lse from gg_attention_flash16_win_fwd; without and with the bias gradient
  (each arm with the partial-row scratch its own rows function asks for); the new kernels' fraction of the 16-bit MFMA roof on the declared 10 N^2 D flops;
* step cases: the bf16 tiny_vit_21m_512 fully-trainable training step of tools/bench_recompute.py (SuperGuessr head, AdamW), library switch off and on
  (gg_tinyvit_set_attention16_train), without and with recompute; the attention kernels' share of the step from one profiled step per arm (gg_prof_read,
  category 1).

Gates, printed (no ratio is fixed in advance; the margin is the reference arm's own round spread, (max - min) / median, as this run measures it): the new kernel
pair is no slower than the f32-pipe arm at either shape, the step is no slower with the switch on.

One JSON line per case is appended to profiles/attention16_tinyvit_bwd_bench.jsonl (--out)."""
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

from tools.bench_attention16 import MFMA16_ROOF_TFLOPS, ab, spread, stats

KERNEL_CASES = [(64, 12, 32), (64, 12, 24)]          # windows, heads, window side
MODEL = "tiny_vit_21m_512"


def gate(ms, ref, new):
    """new's median <= ref's median * (1 + ref's own round spread)."""
    med = {k: statistics.median(v) for k, v in ms.items()}
    margin = spread(ms[ref])
    return dict(reference=ref, margin=round(margin, 4), ratio_new_over_reference=round(med[new] / med[ref], 4), ok=bool(med[new] <= med[ref] * (1.0 + margin)))


def kernel_case(L, W, H, ws, dbias, args):
    st, N, D = torch.bfloat16, ws * ws, 32
    g = torch.Generator("cuda").manual_seed(1)
    qkv = torch.randn(W * N, 3 * H * D, device="cuda", generator=g).to(st)
    dout = torch.randn(W * N, H * D, device="cuda", generator=g).to(st)
    table = 0.5 * torch.randn(H, N, device="cuda", generator=g)
    out, lse = torch.empty(W * N, H * D, dtype=st, device="cuda"), torch.empty(W * N, H, device="cuda")
    lib, s = L.lib(), L.stream()
    rows = {"f32_pipe": lib.gg_attention_flash_dbias_rows(W, N), "mfma16": lib.gg_attention_flash16_win_dbias_rows(W, N)}
    dq = {k: torch.zeros_like(qkv) for k in rows}
    db = {k: torch.zeros_like(table) for k in rows}
    scratch = {k: torch.empty(r * H * N, device="cuda") for k, r in rows.items()}
    a = {}
    for k in rows:
        a[k] = L.AttnArgs()
        a[k].qkv, a[k].ld, a[k].q_off, a[k].k_off, a[k].v_off, a[k].head_stride, a[k].head_dim = qkv.data_ptr(), 3 * H * D, 0, 32, 64, 96, D
        a[k].num_heads, a[k].num_windows, a[k].tokens_per_window, a[k].window_size, a[k].map_h, a[k].map_w, a[k].scale = H, W, N, ws, ws, ws, D ** -0.5
        a[k].bias_table, a[k].out, a[k].ldo, a[k].lse = table.data_ptr(), out.data_ptr(), H * D, lse.data_ptr()
        a[k].dout, a[k].lddo, a[k].dqkv = dout.data_ptr(), H * D, dq[k].data_ptr()
    L.check(lib.gg_attention_flash16_win_fwd(C.byref(a["mfma16"]), 0, s), "gg_attention_flash16_win_fwd")
    if dbias:
        for k in rows:
            a[k].dbias, a[k].dbias_scratch = db[k].data_ptr(), scratch[k].data_ptr()
    arms = {"f32_pipe": lambda: L.check(lib.gg_attention_bwd(C.byref(a["f32_pipe"]), s), "gg_attention_bwd"),
            "mfma16": lambda: L.check(lib.gg_attention_flash16_win_bwd(C.byref(a["mfma16"]), 0, s), "gg_attention_flash16_win_bwd")}
    ms = ab(arms, args.rounds, args.calls, args.warmup)
    diff = float((dq["mfma16"].double() - dq["f32_pipe"].double()).abs().max())
    med = {k: statistics.median(v) for k, v in ms.items()}
    flop = 10.0 * W * H * N * N * D
    return dict(case="kernel", storage="bf16", windows=W, heads=H, tokens=N, dbias=int(dbias), ms=stats(ms),
                f32_pipe_over_mfma16_median=round(med["f32_pipe"] / med["mfma16"], 4), spread={k: round(spread(v), 4) for k, v in ms.items()},
                gate_no_slower_than_f32_pipe=gate(ms, "f32_pipe", "mfma16"),
                tflops_declared={k: round(flop / (med[k] * 1e-3) / 1e12, 1) for k in med},
                mfma16_frac_of_roof=round(flop / (med["mfma16"] * 1e-3) / 1e12 / MFMA16_ROOF_TFLOPS, 4), max_abs_diff_between_arms=diff)


def step_case(L, recompute, images, args):
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.optim import AdamW
    lib = L.lib()
    gc.collect(); torch.cuda.empty_cache()
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(MODEL, pretrained=False, precision="bf16", grad_checkpointing=recompute)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True, serving=False).cuda().train()
    base.unfreeze_all()
    opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
    g = torch.Generator(device="cuda").manual_seed(1)
    S = base.backbone.cfg.img_size
    x = torch.randn(images // 4, 4, 3, S, S, device="cuda", generator=g)
    lab = torch.stack([torch.rand(images // 4, device="cuda", generator=g) * 360 - 180, torch.rand(images // 4, device="cuda", generator=g) * 180 - 90], 1)

    def arm(on):
        def run():
            prev = lib.gg_tinyvit_set_attention16_train(on)          # the library switch: read when the forward and the backward are enqueued
            try:
                out = model(pixel_values=x, labels=lab)
                out.loss.backward()
            finally:
                lib.gg_tinyvit_set_attention16_train(prev)
            opt.step()
            opt.zero_grad()
        return run
    arms = {"off": arm(0), "on": arm(1)}
    ms = ab(arms, args.step_rounds, 1, 1)
    med = {k: statistics.median(v) for k, v in ms.items()}
    attn, calls = {}, {}
    for k, fn in arms.items():          # one profiled step per arm: the attention category's share of the kernels' time
        n = (lib.gg_attention_flash16_win_calls(), lib.gg_attention_flash16_win_bwd_calls())
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
        calls[k] = (lib.gg_attention_flash16_win_calls() - n[0], lib.gg_attention_flash16_win_bwd_calls() - n[1])
    res = dict(case="step", model=MODEL, precision="bf16", policy="all", recompute=int(recompute), images=images, ms_per_step=stats(ms),
               off_over_on_median=round(med["off"] / med["on"], 4), spread={k: round(spread(v), 4) for k, v in ms.items()},
               gate_no_slower_with_the_switch_on=gate(ms, "off", "on"), attention=attn, flash16_win_fwd_and_bwd_calls_per_step=calls)
    del model, base, opt, x
    gc.collect(); torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=128, help="step batch (a multiple of 4): tools/bench_recompute.py's default512 case runs 128")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention16_tinyvit_bwd_bench.jsonl"))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    gates = []

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(dict(line, rounds=args.rounds, calls_per_round=args.calls, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:16])) + "\n")
        for k, v in line.items():
            if k.startswith("gate_"):
                gates.append((f"{line['case']} {line.get('tokens', line.get('model'))} dbias={line.get('dbias', '-')} recompute={line.get('recompute', '-')}", k, v))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.step_only:
        for W, H, ws in KERNEL_CASES:
            for dbias in (False, True):
                emit(kernel_case(L, W, H, ws, dbias, args))
                torch.cuda.empty_cache()
    if not args.kernel_only:
        for recompute in (False, True):
            emit(step_case(L, recompute, args.images, args))
    for what, name, g in gates:
        print(f"GATE {'ok  ' if g['ok'] else 'MISS'} {what}: {name}: new / reference {g['ratio_new_over_reference']} (margin: the reference arm's spread {g['margin']})")
    return 0 if all(g["ok"] for _, _, g in gates) else 1


if __name__ == "__main__":
    sys.exit(main())
