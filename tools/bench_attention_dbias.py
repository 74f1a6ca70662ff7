#!/usr/bin/env python3
"""The fixed-order bias gradient (gg_attention_dbias, include/gg_attn_dbias.h) against the float atomics it replaces, in one process on one device, on
tools/bench_attention16.py's scheme: rounds alternate the arms, every round is timed with device events around `--calls` launches after a warm-up of every arm, a
case reports the median, the minimum and every round.

* layer cases (`atomics`: the existing backward with dbias, the baseline; `fixed`: the existing backward without dbias plus gg_attention_dbias; `bwd_only` and
  `dbias_only`: the two halves of `fixed` on their own): 7 x 7 x 18 heads at 1024 images (tiny_vit_21m_224 stage 3), 14 x 14 x 12 heads at 1024 images (stage 2),
  1024 tokens x 12 heads at 64 images (tiny_vit_21m_512 stage 2; bf16 also through the 16-bit-MFMA window pair: `attention16_train`), f32 and bf16 storage,
  random N(0, 1) q / k / v / dout in TinyViT's per-head [q | k | v] layout, a random table, out and lse from the forward of the same route;
* step cases: the bench.py headline configuration (tiny_vit_21m_224, 256 panoramas = 1024 images, the reference freeze policy, SuperGuessr head, AdamW) in the
  three precisions, and the fully trainable bf16 tiny_vit_21m_512 step at 128 images with attention16_train; library switch off / on
  (gg_tinyvit_set_deterministic_dbias), the off arm TWICE (`off`, `off_again`) so that the run-to-run spread is on record; the new launches' time from one
  profiled step (gg_prof_read, the class of its own).

There is no speed gate: the switch is an opt-in whose purpose is reproducibility.  One JSON line per case is appended to profiles/attention_dbias_bench.jsonl."""
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

from tools.bench_attention16 import ab, spread, stats

# (name, window side, heads, images, windows per image)
LAYER_CASES = [("7x7x18@1024", 7, 18, 1024, 1), ("14x14x12@1024", 14, 12, 1024, 1), ("32x32x12@64", 32, 12, 64, 1)]


def layer_case(L, name, ws, H, W, storage, attn16, args):
    st, N, D = (torch.bfloat16 if storage == "bf16" else torch.float32), ws * ws, 32
    dt = int(storage == "f32")
    g = torch.Generator("cuda").manual_seed(1)
    qkv = torch.randn(W * N, 3 * H * D, device="cuda", generator=g).to(st)
    dout = torch.randn(W * N, H * D, device="cuda", generator=g).to(st)
    table = 0.5 * torch.randn(H, N, device="cuda", generator=g)
    out, lse = torch.empty(W * N, H * D, dtype=st, device="cuda"), torch.empty(W * N, H, device="cuda")
    dqkv = torch.zeros_like(qkv)
    lib, s = L.lib(), L.stream()

    def make(dbias):
        a = L.AttnArgs()
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), 3 * H * D, 0, 32, 64, 96, D
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = H, W, N, ws, ws, ws, D ** -0.5
        a.bias_table, a.out, a.ldo, a.lse = table.data_ptr(), out.data_ptr(), H * D, lse.data_ptr()
        a.dout, a.lddo, a.dqkv = dout.data_ptr(), H * D, dqkv.data_ptr()
        return a
    full = None
    if storage == "bf16" and not attn16 and N <= 256:      # gg_attention_fwd / _bwd read the expanded table as well
        Np = lib.gg_attention_padded_tokens(N)
        full = torch.empty(H, Np, Np, dtype=torch.bfloat16, device="cuda")
        L.check(lib.gg_attention_expand_bias(table.data_ptr(), H, ws, L.f32(D ** -0.5), full.data_ptr(), s), "gg_attention_expand_bias")
    if attn16:
        entry, fwd, bwd = "FLASH16_WIN_BWD", (lambda a: lib.gg_attention_flash16_win_fwd(C.byref(a), 0, s)), (lambda a: lib.gg_attention_flash16_win_bwd(C.byref(a), 0, s))
    elif storage == "bf16":
        entry, fwd, bwd = "BWD", (lambda a: lib.gg_attention_fwd(C.byref(a), s)), (lambda a: lib.gg_attention_bwd(C.byref(a), s))
    else:
        entry, fwd, bwd = "FLASH_BWD", (lambda a: lib.gg_attention_flash_fwd(C.byref(a), dt, s)), (lambda a: lib.gg_attention_flash_bwd(C.byref(a), dt, s))
    a_with, a_without, a_new = make(True), make(False), make(False)
    for a in (a_with, a_without, a_new):
        a.bias = None if full is None else full.data_ptr()
    L.check(fwd(a_without), "forward")
    db_old, db_new = torch.zeros_like(table), torch.zeros_like(table)
    a_with.dbias = db_old.data_ptr()
    route = L.attention_route(a_with, entry, dt)
    scratch_old = torch.empty(route.dbias_rows * H * N, device="cuda")
    a_with.dbias_scratch = scratch_old.data_ptr()
    a_new.dbias = db_new.data_ptr()
    rows = lib.gg_attention_dbias_rows(C.byref(a_new), dt)
    scratch_new = torch.empty(rows * H * N, device="cuda")
    a_new.dbias_scratch = scratch_new.data_ptr()
    r0 = L.attention_route(a_without, entry, dt)
    rounded = int(bool(r0.rounded_bias) or L.ATTN_KERNELS[r0.kernel] in ("BWD", "BWD_GROUPED"))
    new = lambda: L.check(lib.gg_attention_dbias(C.byref(a_new), dt, rounded, s), "gg_attention_dbias")
    old = lambda a: (lambda: L.check(bwd(a), "backward"))

    def fixed():
        old(a_without)(); new()
    arms = {"atomics": old(a_with), "fixed": fixed, "bwd_only": old(a_without), "dbias_only": new}
    db_old.zero_(); db_new.zero_()
    arms["atomics"](); new()
    torch.cuda.synchronize()
    diff = float((db_old - db_new).abs().max() / db_old.abs().max())
    ms = ab(arms, args.rounds, args.calls, args.warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(case="layer", shape=name, storage=storage, attention16_train=int(attn16), backward_kernel=L.ATTN_KERNELS[route.kernel], round_bias=rounded,
                windows=W, heads=H, tokens=N, ms=stats(ms), spread={k: round(spread(v), 4) for k, v in ms.items()},
                fixed_over_atomics_median=round(med["fixed"] / med["atomics"], 4), dbias_rel_diff_between_arms=diff)


def step_case(L, model_name, precision, images, unfrozen, attn16, args):
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.optim import AdamW
    lib = L.lib()
    gc.collect(); torch.cuda.empty_cache()
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(model_name, pretrained=False, precision=precision, attention16_train=attn16)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True, serving=False).cuda().train()
    if unfrozen:
        base.unfreeze_all()
    opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
    g = torch.Generator(device="cuda").manual_seed(1)
    S = base.backbone.cfg.img_size
    x = torch.randn(images // 4, 4, 3, S, S, device="cuda", generator=g)
    lab = torch.stack([torch.rand(images // 4, device="cuda", generator=g) * 360 - 180, torch.rand(images // 4, device="cuda", generator=g) * 180 - 90], 1)

    def arm(on):
        def run():
            prev = lib.gg_tinyvit_set_deterministic_dbias(on)          # the library switch: read when the backward is enqueued
            try:
                out = model(pixel_values=x, labels=lab)
                out.loss.backward()
            finally:
                lib.gg_tinyvit_set_deterministic_dbias(prev)
            opt.step()
            opt.zero_grad()
        return run
    arms = {"off": arm(0), "on": arm(1), "off_again": arm(0)}
    ms = ab(arms, args.step_rounds, 1, 1)
    med = {k: statistics.median(v) for k, v in ms.items()}
    prof = {}
    for k in ("off", "on"):          # one profiled step per arm: the attention class and the new launches' class of their own
        n = lib.gg_attention_dbias_calls()
        lib.gg_prof_reset(); lib.gg_prof_enable(1)
        arms[k]()
        torch.cuda.synchronize()
        lib.gg_prof_enable(0)
        cat = {}
        for c in (1, L.PROF_CAT_ATTN_DBIAS):
            t, nl, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            L.check(lib.gg_prof_read(c, C.byref(t), C.byref(nl), C.byref(fl), C.byref(by)), "gg_prof_read")
            cat[c] = (round(t.value, 3), nl.value)
        lib.gg_prof_reset()
        prof[k] = dict(attention_ms=cat[1][0], attention_launches=cat[1][1], dbias_ms=cat[L.PROF_CAT_ATTN_DBIAS][0], dbias_launches=cat[L.PROF_CAT_ATTN_DBIAS][1],
                       gg_attention_dbias_calls=lib.gg_attention_dbias_calls() - n)
    res = dict(case="step", model=model_name, precision=precision, policy="all" if unfrozen else "reference freeze", attention16_train=int(attn16), images=images,
               ms_per_step=stats(ms), spread={k: round(spread(v), 4) for k, v in ms.items()}, on_over_off_median=round(med["on"] / med["off"], 4),
               off_again_over_off_median=round(med["off_again"] / med["off"], 4), profile=prof)
    del model, base, opt, x
    gc.collect(); torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--layer-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention_dbias_bench.jsonl"))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(dict(line, rounds=args.rounds, calls_per_round=args.calls, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:16])) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.step_only:
        for name, ws, H, images, per in LAYER_CASES:
            for storage in ("f32", "bf16"):
                for attn16 in ((False, True) if (storage == "bf16" and ws == 32) else (False,)):
                    emit(layer_case(L, name, ws, H, images * per, storage, attn16, args))
                    gc.collect(); torch.cuda.empty_cache()
    if not args.layer_only:
        for precision in ("fp32", "fp32_split", "bf16"):
            emit(step_case(L, "tiny_vit_21m_224", precision, 1024, False, False, args))
        emit(step_case(L, "tiny_vit_21m_512", "bf16", 128, True, True, args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
