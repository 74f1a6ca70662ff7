"""The device-side training transform (gg_aug_batch, include/gg_aug.h) next to the step it feeds: 256 raw 640 x 640 images -> 224 x 224 with two RandAugment layers,
seeded records (finetune_tinyvit/augment.py::sample_params, 'rand-m9-mstd0.5-inc1', bicubic).

Prints one JSON line per row and appends them to --out:
  transform        ms per gg_aug_batch call (HIP events around --aug-steps back-to-back calls after --warmup, profiler off; the packed sources, the records and the
                   workspace are set up outside the window -- the call itself includes the host-side validation and the record upload) and images / s
  transform_stages one profiled call (gg_prof_*: HIP events around every stage, in launch order): ms per stage, the statistics passes and the apply passes summed over
                   the layers, and the name of the largest
  train_step       ms per TinyViTClassifier('tiny_vit_5m_224') train() step (forward, loss, backward, AdamW) on the 256 transformed images, which this transform
                   does not touch, and the ratio transform / step
  pillow_host      where Pillow is importable: images / s of the host pipeline on ONE core for the same records (img.crop(box).resize, transpose, the ops through
                   ImageOps / ImageEnhance / Image.transform), over --pillow-images images
    python tools/bench_augment.py [--batch 256 --src 640 --size 224 --layers 2 --aug-steps 300 --steps 20 --warmup 3] [--out profiles/augment_bench.jsonl]
The sources are a seeded smooth gradient plus low-amplitude noise: photograph-like histograms (neighbouring pixels share bins, which is what the LDS histogram atomics
contend on), not white noise."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_sources(B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy = torch.arange(H, device="cuda").view(1, H, 1, 1).float()
    xx = torch.arange(W, device="cuda").view(1, 1, W, 1).float()
    ph = torch.rand(B, 1, 1, 3, generator=g, device="cuda") * 255
    base = (ph + yy * (200.0 / H) + xx * (120.0 / W)) % 256
    noise = torch.randint(0, 24, (B, H, W, 3), generator=g, device="cuda")
    return (base + noise).clamp_(0, 255).to(torch.uint8).contiguous()


def pillow_apply(im, rec, S, flt):
    """One record through Pillow itself, as timm's transform calls it."""
    from PIL import Image, ImageEnhance, ImageOps
    t, l, h, w = int(rec["top"]), int(rec["left"]), int(rec["h"]), int(rec["w"])
    im = im.crop((l, t, l + w, t + h)).resize((S, S), flt)
    if rec["flip"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    for k in range(int(rec["num_layers"])):
        o = rec["ops"][k]
        if not o["applied"]:
            continue
        op, iarg, f = int(o["op"]), int(o["iarg"]), float(o["factor"])
        if op == 0:
            im = ImageOps.autocontrast(im)
        elif op == 1:
            im = ImageOps.equalize(im)
        elif op == 2:
            im = ImageOps.invert(im)
        elif op == 4:
            im = im if iarg >= 8 else ImageOps.posterize(im, iarg)
        elif op == 5:
            im = ImageOps.solarize(im, iarg)
        elif op == 6:
            lut = [min(255, i + iarg) if i < 128 else i for i in range(256)]
            im = im.point(lut + lut + lut)
        elif op in (7, 8, 9, 10):
            im = {7: ImageEnhance.Color, 8: ImageEnhance.Contrast, 9: ImageEnhance.Brightness, 10: ImageEnhance.Sharpness}[op](im).enhance(f)
        else:                             # Rotate too: Image.rotate is Image.transform with the matrix the record holds
            im = im.transform(im.size, Image.AFFINE, tuple(float(v) for v in o["m"]), resample=int(o["resample"]), fillcolor=tuple(int(v) for v in o["fill"]))
    return im


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--src", type=int, default=640)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20, help="timed training steps")
    ap.add_argument("--aug-steps", type=int, default=300, help="timed gg_aug_batch calls (a call takes about a millisecond: enough of them to fill a fraction of a second)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--classes", type=int, default=200)
    ap.add_argument("--precision", default="fp32_split")
    ap.add_argument("--pillow-images", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.finetune_tinyvit import augment as A
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    from geoguessr_ai_amd.optim import AdamW
    L.require_gpu()
    lib = L.lib()
    B, S, H = a.batch, a.size, a.src
    rows = []
    common = dict(tool="bench_augment", batch=B, src=f"{H}x{H}", size=S, layers=a.layers, seed=a.seed, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:12])

    src = make_sources(B, H, H, a.seed)
    recs = A.sample_params([(H, H)] * B, S, f"rand-m9-mstd0.5-inc1-n{a.layers}", np.random.default_rng(a.seed), interpolation="bicubic")
    offsets = (np.arange(B, dtype=np.int64) * 3 * H * H)
    heights = widths = np.full(B, H, np.int32)
    dst = torch.empty(B, 3, S, S, device="cuda")
    args = L.AugArgs()
    args.src, args.src_bytes = src.data_ptr(), src.numel()
    args.offsets, args.heights, args.widths = offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data
    args.B, args.S, args.filter = B, S, 3
    args.mean, args.std = (C.c_float * 3)(*A.TINYVIT_MEAN), (C.c_float * 3)(*A.TINYVIT_STD)
    args.records = recs.ctypes.data
    need = lib.gg_aug_workspace_bytes(C.byref(args))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    args.dst, args.workspace, args.workspace_bytes = dst.data_ptr(), ws.data_ptr(), need

    def call():
        L.check(lib.gg_aug_batch(C.byref(args), L.stream()), "gg_aug_batch")

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.aug_steps):
        call()
    e1.record()
    torch.cuda.synchronize()
    t_ms = e0.elapsed_time(e1) / a.aug_steps
    applied = recs["ops"]["applied"][:, :a.layers]
    rows.append(dict(common, row="transform", ms_per_batch=round(t_ms, 4), images_per_s=round(B / t_ms * 1e3, 1), steps=a.aug_steps, warmup=a.warmup,
                     workspace_mib=round(need / 2 ** 20, 1), mean_crop_area_fraction=round(float((recs["h"] * recs["w"]).mean()) / (H * H), 4),
                     applied_slots=int(applied.sum()), slots=int(applied.size)))

    # one profiled call: a scope per stage, in launch order
    needs_stats = [bool((applied[:, l].astype(bool) & np.isin(recs["ops"]["op"][:, l], (0, 1, 8))).any()) for l in range(a.layers)]
    names = ["coefficients", "horizontal", "vertical"]
    for l in range(int(recs["num_layers"].max())):
        names += (["statistics"] if needs_stats[l] else []) + ["apply"]
    names.append("pack")
    lib.gg_prof_reset()
    lib.gg_prof_enable(1)
    call()
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    assert lib.gg_prof_count() == len(names), (lib.gg_prof_count(), names)
    stages, ms = {}, C.c_double()
    for i, n in enumerate(names):
        L.check(lib.gg_prof_record(i, None, C.byref(ms), None, None), "gg_prof_record")
        stages[n] = stages.get(n, 0.0) + ms.value
    lib.gg_prof_reset()
    rows.append(dict(common, row="transform_stages", stage_ms={k: round(v, 4) for k, v in stages.items()}, stage_sum_ms=round(sum(stages.values()), 4),
                     dominant_stage=max(stages, key=stages.get)))

    # the step the transform feeds: train()'s body on the same 256 images
    model = TinyViTClassifier("tiny_vit_5m_224", num_classes=a.classes, precision=a.precision, seed=1, **({"img_size": S} if S != 224 else {})).cuda().train()
    opt = AdamW(model, lr=5e-4, weight_decay=0.05)
    y = torch.randint(0, a.classes, (B,), generator=torch.Generator().manual_seed(1)).cuda()

    def step():
        opt.zero_grad(set_to_none=True)
        loss, _ = model.loss_and_metrics(model(dst), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    s_ms = e0.elapsed_time(e1) / a.steps
    rows.append(dict(common, row="train_step", model="tiny_vit_5m_224", precision=a.precision, classes=a.classes, ms_per_step=round(s_ms, 3), steps=a.steps,
                     images_per_s=round(B / s_ms * 1e3, 1), loss=round(float(loss.detach()), 4), transform_over_step=round(t_ms / s_ms, 4)))

    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None and a.pillow_images > 0:
        torch.set_num_threads(1)
        n = min(a.pillow_images, B)
        host = [Image.fromarray(src[b].cpu().numpy()) for b in range(n)]
        mean, std = np.asarray(A.TINYVIT_MEAN, np.float32).reshape(3, 1, 1), np.asarray(A.TINYVIT_STD, np.float32).reshape(3, 1, 1)
        t0 = time.perf_counter()
        for b in range(n):
            im = pillow_apply(host[b], recs[b], S, 3)
            x = (np.asarray(im).astype(np.float32).transpose(2, 0, 1) / np.float32(255) - mean) / std      # ToTensor + Normalize
        dt = time.perf_counter() - t0
        u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
        args.dst_u8 = u8.data_ptr()
        call()
        torch.cuda.synchronize()
        same = bool(np.array_equal(u8[n - 1].cpu().numpy(), np.asarray(im)))
        rows.append(dict(common, row="pillow_host", pillow=Image.__version__, images=n, cores=1, images_per_s=round(n / dt, 1),
                         device_over_host_core=round((B / t_ms * 1e3) / (n / dt), 1), last_image_byte_identical_to_device=same))
    else:
        rows.append(dict(common, row="pillow_host", pillow=None, note="Pillow is not importable here: not measured"))

    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
