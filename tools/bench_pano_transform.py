"""The panorama fine-tune's input path on the device (gg_pano_batch, include/gg_pano.h; training/preprocess.py::DevicePanoramaTransform) next to what it replaces:
--panoramas panoramas x 4 views of 640 x 640 4:2:0 quality-90 files without restart markers (tools/bench_jpeg_decode.py's files), required_size 336, to the
reference's default target (512, 512) and to the c2 target (224, 224).

Prints one JSON line per row and appends them to --out; per target:
  pano_batch         HIP-event ms per DevicePanoramaTransform call on the decoded packed batch (ONE gg_pano_batch), --calls calls back to back; GB/s against the call's
                     algorithmic bytes (sources read, intermediate and resized images written and read, the result written)
  composed           the same batch through the entry points the library had before: gg_eval_batch with the torchvision geometry, the whole resized image as the crop
                     and dst_u8 (DeviceEvalTransform), a permute to (B, 3, 336, 336), gg_preprocess_bilinear (prepare_batch).  GATE (a): pano_batch takes no longer
  pano_stages        one profiled call (gg_prof_*: HIP events around every stage, in launch order): coefficients, horizontal, vertical, interpolation
  host_pool          file bytes -> pixel_values, wall clock: a pool of --threads threads runs the dataset's statements per view (Image.open(...).convert("RGB"),
                     Resize(336) = Image.resize(BILINEAR), ToTensor), torch.stack, then the upload and prepare_batch
  device_e2e         file bytes -> pixel_values through DevicePanoramaTransform with jpeg_split_bytes 0 and 512, wall clock, synchronised.  GATE (b): neither takes
                     longer than host_pool
  c2_step            (224 only, unless --skip-step) one bf16 training step of SuperGuessr on TinyViT-21M over the same pixel_values, forward + backward + AdamW, HIP events:
                     the time the transform has to hide behind
Timing: the variants alternate within one process after --warmup calls, --repeats times; every row reports the median and the spread (min, max).
    python tools/bench_pano_transform.py [--panoramas 256] [--out profiles/pano_transform_bench.jsonl]"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def spread(v):
    return dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), repeats=len(v))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def events(fn, calls):
    """HIP-event ms per call over `calls` calls back to back."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panoramas", type=int, default=256)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--src", type=int, default=640)
    ap.add_argument("--required-size", type=int, default=336)
    ap.add_argument("--targets", type=int, nargs="+", default=[512, 224])
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--e2e-repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-step", action="store_true", help="leave out the c2_step row (and the model it needs)")
    ap.add_argument("--skip-e2e", action="store_true", help="leave out host_pool / device_e2e")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image
    from bench_augment import make_sources
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    from geoguessr_ai_amd.training.preprocess import DeviceEvalTransform, DevicePanoramaTransform, prepare_batch, raw_image_geometry
    L.require_gpu()
    lib = L.lib()
    N, V, H, rs = a.panoramas, a.views, a.src, a.required_size
    B = N * V
    common = dict(tool="bench_pano_transform", panoramas=N, views=V, src=f"{H}x{H}", required_size=rs, quality=a.quality, subsampling="4:2:0", restart="none",
                  unique=a.unique, seed=a.seed, threads=a.threads, device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:12])
    files = []
    for im in make_sources(a.unique, H, H, a.seed).cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, "JPEG", quality=a.quality, subsampling="4:2:0")
        files.append(buf.getvalue())
    files = [files[b % a.unique] for b in range(B)]
    panoramas = [files[n * V:(n + 1) * V] for n in range(N)]
    decoded = DeviceJpegDecoder("cuda").decode(files)
    decoded = decoded._replace(slots=np.arange(B, dtype=np.int32).reshape(N, V))
    hr, wr = raw_image_geometry(H, H, "torchvision", rs)[1]
    pool = ThreadPoolExecutor(a.threads)
    rows, gate_ok = [], True

    def host_view(f):                                          # LocalGeoMapDataset's statements for one view
        im = Image.open(io.BytesIO(f)).convert("RGB").resize((wr, hr), Image.BILINEAR)
        # ToTensor in numpy (the same float32 division): sixteen threads of torch CPU ops, each with a thread pool of its own, oversubscribe the cores and cost the
        # pool a factor of ten, which a DataLoader's worker processes do not pay
        return torch.from_numpy(np.ascontiguousarray(np.asarray(im, np.uint8).transpose(2, 0, 1)).astype(np.float32) / np.float32(255))

    for T in a.targets:
        target = (T, T)
        cfg = dict(common, target=f"{T}x{T}")
        pano = DevicePanoramaTransform(target, MEAN, STD, required_size=rs)
        ev = DeviceEvalTransform(rs, MEAN, STD, "torchvision")

        def new():
            return pano(decoded)

        def old():
            _, u8 = ev(decoded, return_u8=True)
            return prepare_batch(u8.permute(0, 3, 1, 2).contiguous().view(N, V, 3, hr, wr), target, MEAN, STD)
        x, y = new(), old()
        diff = float((x - y).abs().max())
        del x, y
        for _ in range(a.warmup):
            new(); old()
        tn, to = [], []
        for _ in range(a.repeats):                             # the variants alternate: a drift of the machine reaches both
            tn.append(events(new, a.calls)); to.append(events(old, a.calls))
        sn, so = spread(tn), spread(to)
        tstride = (3 * wr + 3) // 4 * 4
        algo = B * (3.0 * H * H + 2.0 * H * tstride + 2.0 * hr * tstride + 12.0 * T * T)
        ok = bool(sn["ms"] <= so["ms"])
        rows.append(dict(cfg, row="pano_batch", **sn, unit="ms per call, HIP events", calls=a.calls, images_per_s=round(B / sn["ms"] * 1e3, 1), algorithmic_gb=round(algo / 1e9, 3),
                         gb_per_s=round(algo / sn["ms"] / 1e6, 1), composed_over_pano=round(so["ms"] / sn["ms"], 3), max_abs_diff_to_composed=diff, gate="a", pano_no_slower=ok))
        rows.append(dict(cfg, row="composed", **so, unit="ms per call, HIP events", calls=a.calls, images_per_s=round(B / so["ms"] * 1e3, 1)))
        gate_ok = gate_ok and ok
        names = ["coefficients", "horizontal", "vertical", "interpolation"]
        lib.gg_prof_reset()
        lib.gg_prof_enable(1)
        new()
        torch.cuda.synchronize()
        lib.gg_prof_enable(0)
        assert lib.gg_prof_count() == len(names), lib.gg_prof_count()
        stages, ms = {}, C.c_double()
        for i, n in enumerate(names):
            L.check(lib.gg_prof_record(i, None, C.byref(ms), None, None), "gg_prof_record")
            stages[n] = round(ms.value, 4)
        lib.gg_prof_reset()
        rows.append(dict(cfg, row="pano_stages", stage_ms=stages, stage_sum_ms=round(sum(stages.values()), 4), dominant_stage=max(stages, key=stages.get)))

        if not a.skip_e2e:
            def host():
                views = list(pool.map(host_view, files))
                batch = torch.stack([torch.stack(views[n * V:(n + 1) * V]) for n in range(N)])
                return prepare_batch(batch.to("cuda", non_blocking=True), target, MEAN, STD)
            devs = {S: DevicePanoramaTransform(target, MEAN, STD, required_size=rs, jpeg_split_bytes=S) for S in (0, 512)}
            want = host()
            diffs = {S: float((d(panoramas) - want).abs().max()) for S, d in devs.items()}
            del want
            th, td = [], {S: [] for S in devs}
            for _ in range(a.e2e_repeats):
                th.append(wall(host))
                for S, d in devs.items():
                    td[S].append(wall(lambda: d(panoramas)))
            sh = spread(th)
            rows.append(dict(cfg, row="host_pool", **sh, unit="ms per batch, wall clock, synchronised", images_per_s=round(B / sh["ms"] * 1e3, 1)))
            for S in devs:
                sd = spread(td[S])
                ok = bool(sd["ms"] <= sh["ms"])
                rows.append(dict(cfg, row="device_e2e", jpeg_split_bytes=S, **sd, unit="ms per batch, wall clock, synchronised", images_per_s=round(B / sd["ms"] * 1e3, 1),
                                 host_pool_over_device=round(sh["ms"] / sd["ms"], 2), max_abs_diff_to_host=diffs[S], gate="b", device_no_slower=ok))
                gate_ok = gate_ok and ok
        if T == 224 and not a.skip_step:
            import warnings
            from geoguessr_ai_amd.models.super_guessr import SuperGuessr
            from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
            from geoguessr_ai_amd.optim import AdamW
            torch.manual_seed(0)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                base = TinyViTAdapter("tiny_vit_21m_224", pretrained=False, drop_path_rate=0.0, precision="bf16")
            model = SuperGuessr(base, panorama=True, should_smooth_labels=True).cuda().train()
            opt = AdamW(model, lr=5e-5)
            pv = new()
            g = torch.Generator().manual_seed(1)
            labels = torch.stack([torch.rand(N, generator=g) * 360 - 180, torch.rand(N, generator=g) * 140 - 70], 1).cuda()

            def step():
                opt.zero_grad()
                model(pixel_values=pv, labels=labels).loss.backward()
                opt.step()
            for _ in range(a.warmup):
                step()
            ss = spread([events(step, 1) for _ in range(a.repeats)])
            rows.append(dict(cfg, row="c2_step", model="tiny_vit_21m_224", precision="bf16", **ss, unit="ms per step, HIP events",
                             pano_batch_share_of_step=round(sn["ms"] / ss["ms"], 4)))
            del model, base, opt, pv
            torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not gate_ok:
        print("GATE FAILED: gg_pano_batch is slower than the composed calls (gate a), or the device path from file bytes is slower than the host pool (gate b)",
              file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
