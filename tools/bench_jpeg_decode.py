"""The device JPEG decoder (gg_jpeg_decode, include/gg_jpeg.h) next to the host path it replaces, PIL.Image.open(...).convert("RGB"): batches of 640 x 640 4:2:0
quality-90 files, B = 256 and B = 1024, each without restart markers (what real camera files look like) and with one restart interval per MCU row.

Prints one JSON line per row and appends them to --out; per (B, restart) configuration:
  pillow_1_thread    ms per image, decoded one after the other on one core (at most --one-thread-files of the batch)
  pillow_16_threads  ms per batch in a pool of 16 threads (Pillow releases the GIL while it decodes): the only way before this decoder, the thing being replaced
  device             wall-clock ms per DeviceJpegDecoder.decode(files) call, synchronised: the host plan, filling the pinned buffer, the upload, the four kernels and the
                     status read-back; images / s, the ratio to pillow_16_threads, and whether every decoded byte equals Pillow's.  THE GATE (B = 1024 without
                     restart markers): device takes no longer than pillow_16_threads (exit status 1 otherwise)
  device_stages      one profiled call (gg_prof_*: HIP events around every stage, in launch order): entropy, inverse DCT, status + upsample + colour + pack
  end_to_end         file bytes -> TinyViTEmbedding('tiny_vit_5m_224', batch_transform=True) embeddings: host decode (the 16-thread pool) against device decode
  device_split       with --split-bytes S [S ...], per value: the same call through DeviceJpegDecoder(split_bytes=S) (gg_jscan_decode, include/gg_jscan.h: many
                     lanes inside one scan), timed in the same repeats as the rows above; the sub-segments and speculative lanes of the batch, the share of
                     sub-segments that took the resolve pass's slow path, the ratios to device (split_bytes = 0) and to pillow_16_threads.  THE GATES (without
                     restart markers): at B = 256 the best split takes no longer than pillow_16_threads, at B = 1024 no longer than device
  device_split_stages  one profiled call per value: speculate, resolve, write, DC, inverse DCT, status + upsample + colour + pack
  split_summary      per configuration: the split_bytes that wins
Timing: the variants alternate within one process after --warmup calls, --repeats times; every row reports the median and the spread (min, max).
    python tools/bench_jpeg_decode.py [--batches 256 1024 --src 640 --quality 90] [--out profiles/jpeg_decode_bench.jsonl]
    python tools/bench_jpeg_decode.py --batches 64 256 1024 --split-bytes 256 512 1024 2048 --skip-e2e --out profiles/jpeg_split_bench.jsonl
    python tools/bench_jpeg_decode.py --progressive [--batches 256 1024] [--out profiles/jpeg_progressive_bench.jsonl]
--progressive: the same source images saved with progressive=True, through DeviceJpegDecoder(progressive=True) (gg_jprog_decode, include/gg_jprog.h); three things
alternate in one process: the device decode of the progressive files (row device_progressive), the 16-thread Pillow pool on those same files (pillow_16_threads)
and the device baseline decode of the baseline twins (device_baseline_twins; the ratio is recorded, not gated), then one profiled call (device_progressive_stages).
THE GATE is this path's usual one: at B = 1024 without restart markers device_progressive takes no longer than pillow_16_threads, and every byte equals Pillow's.
The files: --unique seeded synthetic images (smooth structure plus noise, tools/bench_augment.py's generator), encoded once and repeated to fill the batch; every
copy is decoded on its own."""
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


def spread(v):
    return dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), repeats=len(v))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def pil_decode(f):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def progressive_main(a):
    from PIL import Image
    from bench_augment import make_sources
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder, JpegPlan
    L.require_gpu()
    lib = L.lib()
    H = a.src
    out_path = a.out or os.path.join(ROOT, "profiles", "jpeg_progressive_bench.jsonl")
    common = dict(tool="bench_jpeg_decode --progressive", src=f"{H}x{H}", quality=a.quality, subsampling="4:2:0", unique=a.unique, seed=a.seed, threads=a.threads,
                  device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:12])
    src = make_sources(a.unique, H, H, a.seed).cpu().numpy()

    def save(im, **kw):
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, "JPEG", quality=a.quality, subsampling="4:2:0", **kw)
        return buf.getvalue()
    encoded = {False: ([save(im, progressive=True) for im in src], [save(im) for im in src])}
    try:
        encoded[True] = ([save(im, progressive=True, restart_marker_rows=1) for im in src], [save(im, restart_marker_rows=1) for im in src])
    except OSError as e:                                                 # Pillow's progressive encoder can run out of buffer when restart markers are asked for
        print(json.dumps(dict(common, row="note", note=f"Pillow could not write the progressive files with restart markers: {e}")))
    pool = ThreadPoolExecutor(a.threads)
    pdec, bdec = DeviceJpegDecoder("cuda", progressive=True), DeviceJpegDecoder("cuda")
    rows, gate_ok = [], True
    for B in a.batches:
        for restart, (prog, twins) in encoded.items():
            files, base = [prog[b % a.unique] for b in range(B)], [twins[b % a.unique] for b in range(B)]
            plan = JpegPlan(files, progressive=True)
            cfg = dict(common, batch=B, restart="one interval per MCU row" if restart else "none", file_kib=round(sum(len(f) for f in files) / B / 1024, 1),
                       twin_file_kib=round(sum(len(f) for f in base) / B / 1024, 1), scans_per_file=plan.scans[0], rounds=plan.rounds,
                       lanes=int(sum(i.segments for i in plan.info)))
            plan.close()
            ref = [pil_decode(f) for f in prog]
            got = pdec.unpack(pdec.decode(files))
            identical = all(np.array_equal(got[b].cpu().numpy(), ref[b % a.unique]) for b in range(B))
            del got

            def host16():
                return list(pool.map(pil_decode, files))
            for _ in range(a.warmup):
                host16(); pdec.decode(files); bdec.decode(base)
            t16, tp, tb = [], [], []
            for _ in range(a.repeats):                                    # the three alternate: a drift of the machine reaches all of them
                t = time.perf_counter()
                host16()
                t16.append((time.perf_counter() - t) * 1e3)
                tp.append(wall(lambda: pdec.decode(files)))
                tb.append(wall(lambda: bdec.decode(base)))
            s16, sp, sb = spread(t16), spread(tp), spread(tb)
            gated = B == 1024 and not restart
            ok = bool(sp["ms"] <= s16["ms"])
            rows.append(dict(cfg, row="pillow_16_threads", **s16, unit="ms per batch", images_per_s=round(B / s16["ms"] * 1e3, 1)))
            rows.append(dict(cfg, row="device_progressive", **sp, unit="ms per batch, wall clock, synchronised", images_per_s=round(B / sp["ms"] * 1e3, 1),
                             pillow_16_threads_over_device=round(s16["ms"] / sp["ms"], 2), byte_identical_to_pillow=identical, gated=gated, device_no_slower=ok))
            rows.append(dict(cfg, row="device_baseline_twins", **sb, unit="ms per batch, wall clock, synchronised", images_per_s=round(B / sb["ms"] * 1e3, 1),
                             progressive_over_baseline=round(sp["ms"] / sb["ms"], 2)))
            gate_ok = gate_ok and identical and (ok or not gated)
            names = ["fill_and_entropy_rounds", "idct", "status_upsample_colour_pack"]
            lib.gg_prof_reset()
            lib.gg_prof_enable(1)
            pdec.decode(files)
            torch.cuda.synchronize()
            lib.gg_prof_enable(0)
            assert lib.gg_prof_count() == len(names), lib.gg_prof_count()
            stages, ms = {}, C.c_double()
            for i, n in enumerate(names):
                L.check(lib.gg_prof_record(i, None, C.byref(ms), None, None), "gg_prof_record")
                stages[n] = round(ms.value, 4)
            lib.gg_prof_reset()
            rows.append(dict(cfg, row="device_progressive_stages", stage_ms=stages, stage_sum_ms=round(sum(stages.values()), 4), dominant_stage=max(stages, key=stages.get)))
    for r in rows:
        print(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    if not gate_ok:
        print("GATE MISSED: the progressive device decode is slower than the 16-thread Pillow pool at B = 1024 without restart markers, or bytes differ", file=sys.stderr)
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--src", type=int, default=640)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--one-thread-files", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-bytes", type=int, nargs="*", default=[], help="also time DeviceJpegDecoder(split_bytes=S) for every S given")
    ap.add_argument("--skip-e2e", action="store_true", help="leave out the end_to_end rows (and the embedder they need)")
    ap.add_argument("--progressive", action="store_true", help="time the progressive decode (gg_jprog_decode) instead; rows go to profiles/jpeg_progressive_bench.jsonl")
    a = ap.parse_args()
    if a.progressive:
        return progressive_main(a)
    import warnings
    from PIL import Image
    from bench_augment import make_sources
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder, JpegPlan
    L.require_gpu()
    lib = L.lib()
    H = a.src
    common = dict(tool="bench_jpeg_decode", src=f"{H}x{H}", quality=a.quality, subsampling="4:2:0", unique=a.unique, seed=a.seed, threads=a.threads,
                  device=torch.cuda.get_device_name(0), source_hash=L.source_hash()[:12])
    src = make_sources(a.unique, H, H, a.seed).cpu().numpy()
    encoded = {}
    for restart in (False, True):
        out = []
        for im in src:
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, "JPEG", quality=a.quality, subsampling="4:2:0", **({"restart_marker_rows": 1} if restart else {}))
            out.append(buf.getvalue())
        encoded[restart] = out
    pool = ThreadPoolExecutor(a.threads)
    dec = DeviceJpegDecoder("cuda")
    split_decs = {S: DeviceJpegDecoder("cuda", split_bytes=S) for S in a.split_bytes}
    torch.manual_seed(0)
    emb = None
    if not a.skip_e2e:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            emb = TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", batch_transform=True)
    rows, gate_ok = [], True
    for B in a.batches:
        for restart in (False, True):
            files = [encoded[restart][b % a.unique] for b in range(B)]
            cfg = dict(common, batch=B, restart="one interval per MCU row" if restart else "none", file_kib=round(sum(len(f) for f in files) / B / 1024, 1))
            ref = [pil_decode(f) for f in encoded[restart]]
            p = dec.decode(files)
            got = dec.unpack(p)
            identical = all(np.array_equal(got[b].cpu().numpy(), ref[b % a.unique]) for b in range(B))
            del got, p
            split_info = {}
            for S, sdec in split_decs.items():                           # the same bytes, the slow-path share and the lane counts, before anything is timed
                p = sdec.decode(files)
                got = sdec.unpack(p)
                same = all(np.array_equal(got[b].cpu().numpy(), ref[b % a.unique]) for b in range(B))
                plan = JpegPlan(files, split_bytes=S)
                lanes = sum(n * (6 if i.components == 3 and i.hs * i.vs == 4 else (4 if i.components == 3 and i.hs * i.vs == 2 else i.components)) for n, i in zip(plan.subsegments, plan.info))
                split_info[S] = dict(byte_identical_to_pillow=same, sub_segments=int(plan.total_subsegments), speculate_lanes_at_most=int(lanes),
                                     slow_sub_segments=int(p.slow.sum()), slow_share=round(float(p.slow.sum()) / plan.total_subsegments, 5))
                plan.close()
                del got, p
            one = files[:min(B, a.one_thread_files)]

            def host16():
                return list(pool.map(pil_decode, files))

            def device():
                return dec.decode(files)
            for _ in range(a.warmup):
                host16(); device()
                for sdec in split_decs.values():
                    sdec.decode(files)
            t1, t16, td, ts = [], [], [], {S: [] for S in split_decs}
            for _ in range(a.repeats):                                    # the variants alternate: a drift of the machine reaches all of them
                t = time.perf_counter()
                for f in one:
                    pil_decode(f)
                t1.append((time.perf_counter() - t) * 1e3 / len(one))
                t = time.perf_counter()
                host16()
                t16.append((time.perf_counter() - t) * 1e3)
                td.append(wall(device))
                for S, sdec in split_decs.items():
                    ts[S].append(wall(lambda: sdec.decode(files)))
            s1, s16, sd = spread(t1), spread(t16), spread(td)
            rows.append(dict(cfg, row="pillow_1_thread", **s1, unit="ms per image", files=len(one), images_per_s=round(1e3 / s1["ms"], 1)))
            rows.append(dict(cfg, row="pillow_16_threads", **s16, unit="ms per batch", images_per_s=round(B / s16["ms"] * 1e3, 1)))
            gated = B == 1024 and not restart
            ok = bool(sd["ms"] <= s16["ms"])
            rows.append(dict(cfg, row="device", **sd, unit="ms per batch, wall clock, synchronised", images_per_s=round(B / sd["ms"] * 1e3, 1),
                             pillow_16_threads_over_device=round(s16["ms"] / sd["ms"], 2), byte_identical_to_pillow=identical, gated=gated, device_no_slower=ok))
            gate_ok = gate_ok and identical and (ok or not gated)
            best = None
            for S in split_decs:
                ss = spread(ts[S])
                rows.append(dict(cfg, row="device_split", split_bytes=S, **ss, unit="ms per batch, wall clock, synchronised", images_per_s=round(B / ss["ms"] * 1e3, 1),
                                 device_over_split=round(sd["ms"] / ss["ms"], 2), pillow_16_threads_over_split=round(s16["ms"] / ss["ms"], 2), **split_info[S]))
                gate_ok = gate_ok and split_info[S]["byte_identical_to_pillow"]
                if best is None or ss["ms"] < best[1]["ms"]:
                    best = (S, ss)
            if best is not None:
                gate = None
                if not restart and B == 256:
                    gate = dict(gate="split no slower than pillow_16_threads", passed=bool(best[1]["ms"] <= s16["ms"]))
                if not restart and B == 1024:
                    gate = dict(gate="split no slower than device (split_bytes = 0)", passed=bool(best[1]["ms"] <= sd["ms"]))
                rows.append(dict(cfg, row="split_summary", winning_split_bytes=best[0], winning_ms=best[1]["ms"], device_ms=sd["ms"], pillow_16_threads_ms=s16["ms"],
                                 **(gate or {})))
                gate_ok = gate_ok and (gate is None or gate["passed"])
            # one profiled call: a scope per stage, in launch order
            names = ["entropy", "idct", "status_upsample_colour_pack"]
            lib.gg_prof_reset()
            lib.gg_prof_enable(1)
            device()
            torch.cuda.synchronize()
            lib.gg_prof_enable(0)
            assert lib.gg_prof_count() == len(names), lib.gg_prof_count()
            stages, ms = {}, C.c_double()
            for i, n in enumerate(names):
                L.check(lib.gg_prof_record(i, None, C.byref(ms), None, None), "gg_prof_record")
                stages[n] = round(ms.value, 4)
            lib.gg_prof_reset()
            rows.append(dict(cfg, row="device_stages", stage_ms=stages, stage_sum_ms=round(sum(stages.values()), 4), dominant_stage=max(stages, key=stages.get)))

            for S, sdec in split_decs.items():
                snames = ["speculate", "resolve", "write", "dc", "idct", "status_upsample_colour_pack"]
                lib.gg_prof_reset()
                lib.gg_prof_enable(1)
                sdec.decode(files)
                torch.cuda.synchronize()
                lib.gg_prof_enable(0)
                assert lib.gg_prof_count() == len(snames), lib.gg_prof_count()
                stages = {}
                for i, n in enumerate(snames):
                    L.check(lib.gg_prof_record(i, None, C.byref(ms), None, None), "gg_prof_record")
                    stages[n] = round(ms.value, 4)
                lib.gg_prof_reset()
                rows.append(dict(cfg, row="device_split_stages", split_bytes=S, stage_ms=stages, stage_sum_ms=round(sum(stages.values()), 4),
                                 dominant_stage=max(stages, key=stages.get)))
            if emb is None:
                continue

            # end to end: file bytes -> embeddings
            def e2e_host():
                return emb(host16())

            def e2e_device():
                return emb(files)
            x, y = e2e_host(), e2e_device()
            same = bool(torch.equal(x, y))
            th, tdv = [], []
            for _ in range(a.e2e_repeats):
                th.append(wall(e2e_host)); tdv.append(wall(e2e_device))
            rows.append(dict(cfg, row="end_to_end", model="tiny_vit_5m_224", host_decode=spread(th), device_decode=spread(tdv),
                             speedup=round(statistics.median(th) / statistics.median(tdv), 2), embeddings_identical=same))
            del x, y
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not gate_ok:
        print("GATE FAILED: the device decode is slower than the 16-thread Pillow pool at B = 1024 without restart markers, a split decode misses its gate "
              "(split_summary rows), or bytes differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
