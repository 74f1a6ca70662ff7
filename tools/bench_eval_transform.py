"""The batched eval transform (gg_eval_batch, include/gg_eval.h) next to the per-image path it stands beside: 256 raw 640 x 640 images -> timm's eval transform at 224
(crop_pct 0.95: Pillow bicubic resize to 235 x 235, centre crop, /255, ImageNet mean / std).

Prints one JSON line per row and appends them to --out:
  per_image        ms per batch of B ops.preprocess_pil calls (today's path with the images already on the device: per image one workspace and one output allocation
                   and four launches), images / s
  batched          ms per gg_eval_batch call (packed sources and workspace set up outside the window; the call includes the host-side validation and the table
                   upload), images / s, the algorithmic bytes of a call (what the three stages declare to the launch profiler: weights and windows, the source rows
                   the crop reads, the intermediate written and read, the outputs), achieved bytes / s against them, and the ratio to per_image.  THE GATE:
                   batched takes no longer than per_image (exit status 1 otherwise)
  batched_stages   one profiled call (gg_prof_*: HIP events around every stage, in launch order): ms per stage
  aug_zero_layers  gg_aug_batch on the same images with records of the whole image as the box and no layers: the closest existing batch kernel, informational
  end_to_end       host uint8 images -> TinyViTEmbedding('tiny_vit_5m_224') embeddings, per-image transform against batch_transform=True (host packing, the
                   copy, the transform and the encoder), ms per batch
Timing: HIP events around --calls back-to-back calls after --warmup, the profiler off; the variants alternate within one process, --repeats times, and every row
reports the median and the spread (min, max) over the repeats.
    python tools/bench_eval_transform.py [--batch 256 --src 640 --size 224 --pipeline timm --crop-pct 0.95] [--out profiles/eval_transform_bench.jsonl]
The sources are tools/bench_augment.py's photograph-like generator."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def spread(v):
    return dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), repeats=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--src", type=int, default=640)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--pipeline", default="timm")
    ap.add_argument("--crop-pct", type=float, default=0.95)
    ap.add_argument("--calls", type=int, default=50, help="timed gg_eval_batch / gg_aug_batch calls per repeat")
    ap.add_argument("--per-image-calls", type=int, default=5, help="timed batches of B per-image calls per repeat")
    ap.add_argument("--e2e-calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bench_augment import make_sources
    from geoguessr_ai_amd import _lib as L, ops
    from geoguessr_ai_amd.finetune_tinyvit import augment as A
    from geoguessr_ai_amd.training import preprocess as P
    L.require_gpu()
    lib = L.lib()
    B, S, H = a.batch, a.size, a.src
    mean, std = (P.CLIP_MEAN, P.CLIP_STD) if a.pipeline == "clip" else (P.TINYVIT_MEAN, P.TINYVIT_STD)
    flt, (hr, wr), (top, left) = P.raw_image_geometry(H, H, a.pipeline, S, a.crop_pct)
    common = dict(tool="bench_eval_transform", batch=B, src=f"{H}x{H}", size=S, pipeline=a.pipeline, crop_pct=a.crop_pct, resized=f"{hr}x{wr}", crop_origin=[top, left],
                  seed=a.seed, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:12])
    src = make_sources(B, H, H, a.seed)

    # per image: today's loop of images_to_pixel_values, the images already on the device
    def per_image():
        return torch.stack([ops.preprocess_pil(src[b], flt, (hr, wr), (top, left), (S, S), mean, std, mul_rescale=a.pipeline == "clip") for b in range(B)], 0)

    # batched: one call, everything set up outside the window
    offsets = np.arange(B, dtype=np.int64) * 3 * H * H
    heights = widths = np.full(B, H, np.int32)
    geom = np.zeros(B, P.GEOM_DTYPE)
    geom[:] = (hr, wr, top, left)
    dst = torch.empty(B, 3, S, S, device="cuda")
    e = L.EvalArgs()
    e.src, e.src_bytes = src.data_ptr(), src.numel()
    e.offsets, e.heights, e.widths, e.geom = offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, geom.ctypes.data
    e.B, e.Hc, e.Wc, e.filter, e.mul_rescale, e.normalize = B, S, S, flt, int(a.pipeline == "clip"), 1
    e.mean, e.std = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    need = lib.gg_eval_workspace_bytes(C.byref(e))
    assert need > 0, lib.gg_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    e.dst, e.workspace, e.workspace_bytes = dst.data_ptr(), ws.data_ptr(), need

    def batched():
        L.check(lib.gg_eval_batch(C.byref(e), L.stream()), "gg_eval_batch")

    # the training transform with nothing to do but the resize: the whole image as the box (640 -> S, another reduction than the eval transform's 640 -> 235)
    recs = np.zeros(B, A.RECORD_DTYPE)
    recs["h"], recs["w"] = H, H
    dst_aug = torch.empty(B, 3, S, S, device="cuda")
    g = L.AugArgs()
    g.src, g.src_bytes = src.data_ptr(), src.numel()
    g.offsets, g.heights, g.widths = offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data
    g.B, g.S, g.filter = B, S, flt
    g.mean, g.std = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    g.records = recs.ctypes.data
    need_aug = lib.gg_aug_workspace_bytes(C.byref(g))
    assert need_aug > 0, lib.gg_last_error()
    ws_aug = torch.empty(need_aug, dtype=torch.uint8, device="cuda")
    g.dst, g.workspace, g.workspace_bytes = dst_aug.data_ptr(), ws_aug.data_ptr(), need_aug

    def aug():
        L.check(lib.gg_aug_batch(C.byref(g), L.stream()), "gg_aug_batch")

    # the two paths compute the same pixel_values
    ref = per_image()
    batched()
    torch.cuda.synchronize()
    max_diff = float((ref - dst).abs().max())
    assert max_diff <= 1e-6, max_diff
    del ref

    for _ in range(a.warmup):
        per_image(); batched(); aug()
    torch.cuda.synchronize()
    t = {"per_image": [], "batched": [], "aug": []}
    for _ in range(a.repeats):                                            # the variants alternate: a drift of the machine reaches all of them
        t["per_image"].append(timed(per_image, a.per_image_calls))
        t["batched"].append(timed(batched, a.calls))
        t["aug"].append(timed(aug, a.calls))

    # one profiled call: a scope per stage, in launch order
    names = ["coefficients", "horizontal", "vertical"]
    lib.gg_prof_reset()
    lib.gg_prof_enable(1)
    batched()
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    assert lib.gg_prof_count() == len(names), (lib.gg_prof_count(), names)
    stages, stage_bytes, ms, by = {}, {}, C.c_double(), C.c_double()
    for i, n in enumerate(names):
        L.check(lib.gg_prof_record(i, None, C.byref(ms), None, C.byref(by)), "gg_prof_record")
        stages[n], stage_bytes[n] = ms.value, by.value
    lib.gg_prof_reset()
    alg_bytes = sum(stage_bytes.values())

    rows = []
    pi, ba, au = spread(t["per_image"]), spread(t["batched"]), spread(t["aug"])
    rows.append(dict(common, row="per_image", **pi, images_per_s=round(B / pi["ms"] * 1e3, 1), calls=a.per_image_calls, warmup=a.warmup, launches_per_batch=4 * B))
    rows.append(dict(common, row="batched", **ba, images_per_s=round(B / ba["ms"] * 1e3, 1), calls=a.calls, warmup=a.warmup, launches_per_batch=3 + (B + 15) // 16,
                     workspace_mib=round(need / 2 ** 20, 1), algorithmic_mib=round(alg_bytes / 2 ** 20, 2), achieved_gb_per_s=round(alg_bytes / (ba["ms"] * 1e-3) / 1e9, 1),
                     speedup_over_per_image=round(pi["ms"] / ba["ms"], 2), max_abs_diff_to_per_image=max_diff, gate_batched_no_slower=bool(ba["ms"] <= pi["ms"])))
    rows.append(dict(common, row="batched_stages", stage_ms={k: round(v, 4) for k, v in stages.items()}, stage_mib={k: round(v / 2 ** 20, 2) for k, v in stage_bytes.items()},
                     stage_gb_per_s={k: round(stage_bytes[k] / (v * 1e-3) / 1e9, 1) for k, v in stages.items() if v > 0}, stage_sum_ms=round(sum(stages.values()), 4),
                     dominant_stage=max(stages, key=stages.get)))
    rows.append(dict(common, row="aug_zero_layers", **au, images_per_s=round(B / au["ms"] * 1e3, 1), calls=a.calls,
                     note="gg_aug_batch, whole image as the box, no layers: 640 -> size on both axes, separate pack pass; informational"))

    # end to end: host uint8 images -> embeddings
    import warnings
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    torch.manual_seed(0)
    host = [im.numpy() for im in src.cpu()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        emb = TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", **({"img_size": S} if S != 224 else {}))

    def embed(batch_transform):                                           # one model, the keyword's attribute switched between the two paths
        emb.batch_transform = batch_transform
        return emb(host)
    outs = {k: embed(k == "batch_transform") for k in ("per_image", "batch_transform")}
    torch.cuda.synchronize()
    e2e_rel = float((outs["per_image"] - outs["batch_transform"]).norm() / outs["per_image"].norm())
    te = {"per_image": [], "batch_transform": []}
    for _ in range(a.repeats):
        for k in te:
            te[k].append(timed(lambda: embed(k == "batch_transform"), a.e2e_calls))
    rows.append(dict(common, row="end_to_end", model="tiny_vit_5m_224", per_image=spread(te["per_image"]), batch_transform=spread(te["batch_transform"]),
                     speedup=round(statistics.median(te["per_image"]) / statistics.median(te["batch_transform"]), 2), embedding_rel_l2_between_paths=e2e_rel,
                     calls=a.e2e_calls))

    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not ba["ms"] <= pi["ms"]:
        print(f"GATE FAILED: batched {ba['ms']} ms > per_image {pi['ms']} ms", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
