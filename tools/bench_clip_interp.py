#!/usr/bin/env python3
"""The CLIP vision tower at foreign input sizes (`CLIPVisionTower(..., interpolate_pos_encoding=True)`, include/gg_clip_interp.h) at ViT-L/14-336 dimensions with
random weights, timed on tools/bench_attention16.py's scheme (device events around `--calls` launches per round, rounds alternate the arms, medians reported):

* the frozen bf16 forward at 64 images: 336 px with the flag off and on (the same launch list: asserted), 224 px, 448 px with `attention16` off and on;
* the last-layer fine-tune step (SuperGuessr on the tower, encoder layers [:-1] frozen as models/super_guessr.py does with a pretrained head; forward + backward +
  AdamW) at 336 px and at 448 px with `attention16_train` off and on;
* next to every row: the two resampling kernels alone at that row's geometry and the whole weight-cache refresh (`gg_clip_refresh_weights`, which rebuilds the
  resampled table with everything else; a training step pays it once per optimizer step, a frozen tower pays the forward kernel alone per change of size).

One JSON line per row is appended to profiles/clip_interp_bench.jsonl (--out)."""
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

from tools.bench_attention16 import ab, events, spread, stats

L14 = "openai/clip-vit-large-patch14-336"
PATCH, NATIVE = 14, 336


def launch_list(L, fn):
    lib = L.lib()
    lib.gg_prof_reset(); lib.gg_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    cat, cats = C.c_int(), []
    for i in range(lib.gg_prof_count()):
        L.check(lib.gg_prof_record(i, C.byref(cat), None, None, None), "gg_prof_record")
        cats.append(cat.value)
    lib.gg_prof_reset()
    return cats


def resampling(L, tower, size, args):
    """ms of gg_clip_pos_interp_fwd, gg_clip_pos_interp_bwd (alone, at this size's geometry) and of the whole cache refresh at this size."""
    from geoguessr_ai_amd import ops
    vm = tower.vision_model
    g = size // PATCH
    if g == NATIVE // PATCH:
        return dict(interp_fwd_ms=0.0, interp_bwd_ms=0.0, note="native grid: neither kernel runs, the cache holds no resampled table",
                    refresh_ms=round(events(lambda: vm._refresh(None), args.calls), 4))
    pos = vm._params["embeddings.position_embedding.weight"].data
    out = ops.clip_pos_interp(pos, (g, g))
    d_pos = torch.zeros_like(pos)
    f = events(lambda: ops.clip_pos_interp(pos, (g, g), out=out), args.calls)
    b = events(lambda: ops.clip_pos_interp_bwd(out, pos.shape[0], (g, g), accumulate_into=d_pos), args.calls)
    r = events(lambda: vm._refresh(None), args.calls)
    return dict(interp_fwd_ms=round(f, 4), interp_bwd_ms=round(b, 4), interp_sum_ms=round(f + b, 4), refresh_ms=round(r, 4))


def forward_rows(L, args, emit):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    lib = L.lib()
    t = CLIPVisionTower(L14, seed=0, precision="bf16").cuda().eval()
    for p in t.parameters():
        p.requires_grad = False
    gen = torch.Generator("cuda").manual_seed(1)
    xs = {s: torch.randn(args.batch, 3, s, s, device="cuda", generator=gen) for s in (336, 224, 448)}

    def arm(size, flag, a16):
        def run():
            prev = lib.gg_clip_set_attention16(a16)
            try:
                return t(pixel_values=xs[size], return_last_hidden=False, interpolate_pos_encoding=flag).pooled_mean
            finally:
                lib.gg_clip_set_attention16(prev)
        return run
    with torch.no_grad():
        lists = {flag: launch_list(L, arm(336, flag, 0)) for flag in (False, True)}
        assert lists[False] == lists[True] and lists[False], "336 px: the flag changed the launch list"
        assert torch.equal(arm(336, False, 0)(), arm(336, True, 0)())
        for name, arms in (("336", {"flag_off": arm(336, False, 0), "flag_on": arm(336, True, 0)}), ("224", {"flag_on": arm(224, True, 0)}),
                           ("448", {"attention16_off": arm(448, True, 0), "attention16_on": arm(448, True, 1)})):
            ms = ab(arms, args.rounds, args.calls, args.warmup)
            size = int(name)
            emit(dict(case="forward", model=L14, precision="bf16", batch=args.batch, size=size, tokens=(size // PATCH) ** 2 + 1, ms=stats(ms),
                      spread={k: round(spread(v), 4) for k, v in ms.items()}, launches=len(launch_list(L, next(iter(arms.values())))),
                      same_launch_list_flag_on_off=True if size == 336 else None, resampling=resampling(L, t, size, args)))
    del t, xs
    gc.collect(); torch.cuda.empty_cache()


def finetune_rows(L, args, emit):
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.optim import AdamW
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    lib = L.lib()
    for size in (336, 448):
        gc.collect(); torch.cuda.empty_cache()
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            base = CLIPVisionTower(L14, precision="bf16", interpolate_pos_encoding=True)
            model = SuperGuessr(base, panorama=True, should_smooth_labels=True, serving=False)
        for layer in list(base.vision_model.encoder.layers)[:-1]:
            for p in layer.parameters():
                p.requires_grad = False
        model = model.cuda().train()
        opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
        g = torch.Generator(device="cuda").manual_seed(1)
        n = args.batch // 4
        x = torch.randn(n, 4, 3, size, size, device="cuda", generator=g)
        lab = torch.stack([torch.rand(n, device="cuda", generator=g) * 360 - 180, torch.rand(n, device="cuda", generator=g) * 180 - 90], 1)

        def arm(on):
            def run():
                prev = lib.gg_clip_set_attention16_train(on)
                try:
                    out = model(pixel_values=x, labels=lab)
                    out.loss.backward()
                finally:
                    lib.gg_clip_set_attention16_train(prev)
                opt.step()
                opt.zero_grad()
            return run
        arms = {"attention16_train_off": arm(0)} if size == 336 else {"attention16_train_off": arm(0), "attention16_train_on": arm(1)}
        ms = ab(arms, args.tower_rounds, 1, 1)
        emit(dict(case="finetune_last_layer", model=L14, precision="bf16", images=4 * n, size=size, tokens=(size // PATCH) ** 2 + 1, ms_per_step=stats(ms),
                  spread={k: round(spread(v), 4) for k, v in ms.items()}, resampling_per_step=resampling(L, base, size, args)),
             rounds=args.tower_rounds, calls_per_round=1)
        del model, base, opt, x
    gc.collect(); torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tower-rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="images per forward / per step (a multiple of 4)")
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "clip_interp_bench.jsonl"))
    args = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line, rounds=args.rounds, calls_per_round=args.calls):      # (the kernel / refresh figures next to a row are always args.calls calls)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(dict(line, rounds=rounds, calls_per_round=calls_per_round, resampling_calls=args.calls, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:16])) + "\n")
    forward_rows(L, args, emit)
    if not args.forward_only:
        finetune_rows(L, args, emit)


if __name__ == "__main__":
    main()
