#!/usr/bin/env python3
"""Headline benchmark: images/sec of the TinyViT-21M-224 4-heading fine-tune step (BASELINE.json configs[1]:
256 panoramas = 1024 images per GPU per step; forward + backward + AdamW, haversine-smoothed soft-CE over 12 647
geocells, reference freeze policy ``freeze_all_but_last_stage``, DropPath 0.2, batch-stat BatchNorm) on N MI355X.

    python bench.py --gpus 1 --steps 10 --warmup 3 [--dump-outputs DIR]      (the headline only)
    python bench.py --gpus 1 --steps 10 --warmup 3 --full                    (+ everything below: other modes, roofline, secondary, CPU baseline)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    python bench.py --gpus N ...        (no launcher: starts the line above as a child process and relays its JSON line; exits non-zero
                                         when the machine has fewer than N GPUs -- it never reports an N-GPU number from fewer ranks)

One process per GPU; ranks shard the global batch (weak scaling: 256 panoramas per GPU), start from rank 0's parameters (broadcast) and
exchange only gradients (sum all-reduce over RCCL, launched bucket by bucket while the backward pass is still running; the average
is folded into the AdamW kernel).  Inputs are synthetic and resident in HBM before the timed region.  Rank 0 prints ONE JSON line.

PRECISION.  The reference computes this path in fp32 (torch defaults), so the headline ``value`` / ``dtype`` of the line
are measured in the fp32 reference-precision mode (f32 activations, ``v_mfma_f32_16x16x4_f32``, erf GELU through a 1.2-ulp fp32 Phi).  The bf16 mode (bf16
activations / MFMA operands, fp32 accumulation and master weights -- the mode a production run would use) is measured under ``--full`` in the same
invocation with the same protocol (W warm-up steps, exactly K timed steps between barrier + synchronize) and reported under
``"bf16"``.  ``--precision fp32|bf16`` runs one mode only (then ``value`` is that mode's).

``--full`` adds the figures below (a plain run reports them as null).
``roofline`` (dominant kernel class = the MFMA GEMMs: every Linear / 1x1 conv / im2col'd conv and their dgrad / wgrad).  Every launch is
timed with HIP events recorded on the launch stream inside libgg (``gg_prof_*``) over an instrumented replay of the timed steps and
declares its algorithmic FLOPs (2MNK) and algorithmic bytes (A, B, C once each plus every second tensor its epilogue reads or writes).
fp32: 157.3 TFLOP/s / 8 TB/s = 20 flop/B ridge, every GEMM of the model is above it -> bound "mfma", achieved = sum flops / sum time
against 157.3 TFLOP/s.  bf16: ridge 312 flop/B, the average launch sits near 136 flop/B -> bound "hbm", achieved = algorithmic bytes /
time against 8 TB/s (the MFMA-side numbers ride along).  ``per_launch_frac`` = sum_i max(flops_i / peak_flops, bytes_i / 8 TB/s) /
sum_i t_i: the roofline evaluated per launch instead of on the aggregate (the per-shape table is committed under profiles/).
``traffic`` = measured HBM bytes per GEMM launch (rocprofv3 PMC passes of this command, profiles/).
``cpu_baseline``: the CPU oracle's identical step (torch fp32, host cores) on a bounded sample, rank 0 / N=1 only.
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CATS = ["gemm", "attention", "dwconv", "norm_elementwise", "head_loss", "optimizer", "data_movement"]
GFLOP_PER_IMAGE = 18.2          # fwd 8.50 + dgrad 8.50 + wgrad(patch_embed + stage 3) 1.20
MFMA_PEAK_TF = {"fp32": 157.3, "bf16": 2500.0, "fp32_split": 157.3}      # MI355X_MICROARCH.md: dense f32 / bf16 matrix peaks (fp32_split: whole-step figures priced as f32 work)
DTYPE_LABEL = {"fp32_split": "fp32 (bf16x3 split MFMA)", "fp32": "fp32 (f32 MFMA GEMMs)"}
SPLIT_PEAK_TF = 2500.0 / 6.0        # an f32-accurate split product is six bf16 MFMA products: the roof of the split GEMM kernels in f32-equivalent TFLOP/s
HBM_PEAK_GBS = 8000.0


def host_cpu():
    """(logical CPUs the process may use, CPU model string) of this host -- read from /proc, no subprocess."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        usable = os.cpu_count() or 1
    return usable, model


def cpu_baseline(seconds_budget: float = 14.0):
    """BASELINE.md section 3, the c2-shaped micro-batch: the CPU oracle's identical step (TinyViT-21M-224 + 12 647-cell head, 8 panoramas =
    32 images, forward + backward + AdamW, smooth-label loss, reference freeze policy, seed 1234) on the host cores: a multi-thread figure
    (the headline `value`) and a 1-thread figure on a quarter of the micro-batch, both bounded in wall time.  `cores` = worker threads used
    (torch intra-op pool); `host_cpus` / `cpu_model` say what the box offers."""
    import torch
    from oracle import step_ref as S, tinyvit_ref as R, geo_ref as G
    import numpy as np
    usable, cpu_model = host_cpu()
    # torch's intra-op pool degrades badly when oversubscribed with the many small ops of a 224-px ViT step
    # (measured on a 256-CPU GPU-box host: 256 threads 169 s/step; 8/16/32/64 threads: 10.7/11.3/8.3/4.4 images/s): 16 worker threads, stated next
    # to the number of CPUs the box has
    cores = max(1, min(usable, int(os.environ.get("GG_CPU_THREADS", "16"))))
    cfg = R.config_for("tiny_vit_21m_224", drop_path_rate=0.0)
    st = R.init_state(cfg, 0)
    cent = torch.from_numpy(np.load(os.path.join(ROOT, "geoguessr-ai_amd", "data", "centroids_12647x2_f32.npy")))
    g = torch.Generator().manual_seed(1234)
    n = 8
    x = torch.randn(n, 4, 3, 224, 224, generator=g)
    labels = torch.stack([torch.rand(n, generator=g) * 360 - 180, torch.rand(n, generator=g) * 180 - 90], 1)
    W, b = torch.randn(12647, 576, generator=g) * 0.02, torch.zeros(12647)
    trainable = [k for k in st if k.startswith(("patch_embed", "stages.3", "head")) and "running" not in k and "num_batches" not in k]
    params = {k: st[k] for k in trainable}
    params["cell_layer.weight"], params["cell_layer.bias"] = W, b
    mom = {k: (torch.zeros_like(t), torch.zeros_like(t)) for k, t in params.items()}
    count = [0]

    def step(nn):
        out = S.train_step(cfg, st, W, b, cent, x[:nn], labels[:nn], trainable=trainable)
        count[0] += 1
        with torch.no_grad():            # AdamW (main_coordinator_idun_s3.py:286-291): lr 5e-5, betas (.9, .999), wd .01 -- oracle/geo_ref.adamw_step
            for k, t in params.items():
                gk = out["grads"].get(k)
                if gk is None:
                    continue
                m, v = mom[k]
                pn, mn_, vn = G.adamw_step(t.numpy(), gk.numpy(), m.numpy(), v.numpy(), count[0], 5e-5)
                t.copy_(torch.from_numpy(np.ascontiguousarray(pn))); m.copy_(torch.from_numpy(np.ascontiguousarray(mn_))); v.copy_(torch.from_numpy(np.ascontiguousarray(vn)))

    def timed(nn, budget, min_steps):
        step(nn)                                                             # warm-up
        ts = []
        t0 = time.time()
        while len(ts) < min_steps or (time.time() - t0) < budget:
            t1 = time.time(); step(nn); ts.append(time.time() - t1)
        return float(np.median(ts)), len(ts), time.time() - t0

    torch.set_num_threads(cores)
    med, steps, dt = timed(n, seconds_budget, 2)
    n1 = 1
    torch.set_num_threads(1)
    med1, steps1, dt1 = timed(n1, 0.0, 3)
    torch.set_num_threads(cores)
    return dict(value=round(n * 4 / med, 3), unit="images/s", cores=cores, kind="port", host_cpus=os.cpu_count(), usable_cpus=usable, cpu_model=cpu_model,
                one_thread=dict(value=round(n1 * 4 / med1, 3), unit="images/s", cores=1,
                                sample=f"1 warm-up + {steps1} timed steps (median) of {n1} panorama = {n1 * 4} images, {dt1:.1f} s"),
                sample=f"1 warm-up + {steps} timed oracle train steps (fwd+bwd+AdamW, torch fp32, median) of {n} panoramas = {n * 4} images, "
                       f"TinyViT-21M-224 + 12647-cell head, reference freeze policy, {cores} threads on a host with {os.cpu_count()} CPUs ({cpu_model}), {dt:.1f} s")


def clock_under_gemm_load(dev):
    """Shader clock while the fp32 GEMMs run: traced launches of the five heaviest GEMM forms of the fp32 step (gg_gemm_f32_set_trace: every workgroup
    records s_memtime, which ticks at the shader clock, and the constant 100 MHz wall clock over its life).  MI355X lowers its clock under sustained fp32
    MFMA load, so the matrix peak that can be reached is 157.3 TFLOP/s x (clock / 2.4 GHz).  -> (flop-weighted mean MHz, {form: MHz})."""
    import numpy as np
    import torch
    from geoguessr_ai_amd import ops, _lib as L
    forms = [("stage2.qkv 200704x1152x384", 200704, 1152, 384), ("stage2.fc1 200704x1536x384", 200704, 1536, 384), ("stage2.fc2 200704x384x1536", 200704, 384, 1536),
             ("stage1.fc1 802816x768x192", 802816, 768, 192), ("stage0.conv3 3211264x96x384", 3211264, 96, 384)]
    per, wsum, w = {}, 0.0, 0.0
    for name, M, N, K in forms:
        A = torch.randn(M, K, device=dev); B = torch.randn(N, K, device=dev) * 0.05; out = torch.empty(M, N, device=dev)
        tiles = ((M + 63) // 64) * ((N + 63) // 64)                  # (at least as many records as any tile form launches workgroups)
        buf = torch.zeros(tiles, 8, dtype=torch.int64, device=dev)
        for _ in range(3):
            ops.gemm_nt(A, B, out=out)
        L.lib().gg_gemm_f32_set_trace(buf.data_ptr())
        try:
            ops.gemm_nt(A, B, out=out)
            torch.cuda.synchronize(dev)
        finally:
            L.lib().gg_gemm_f32_set_trace(None)
        t = buf.cpu().numpy().astype("float64")
        life_us = (t[:, 5] - t[:, 2]) * 0.01
        ok = life_us > 1.0
        if ok.any():
            mhz = float(np.median(t[ok, 1] / life_us[ok]))
            per[name] = round(mhz, 0)
            wsum += mhz * M * N * K; w += float(M) * N * K
        del A, B, out, buf
    return (wsum / w if w else None), per


def pmc_traffic(precision):
    """HBM bytes per GEMM launch from the committed rocprofv3 PMC passes of this command (FETCH_SIZE x2 on gfx950 + WRITE_SIZE, separate
    runs; tools/profile_round.sh + tools/pmc_traffic.py).  PMC collection cannot run inside the timed process, so this is the offline
    measurement of the same workload.  The file records the sha256 of the kernel sources it was measured on: when the running tree differs the
    figure is still reported but marked ``stale``.  -> (bytes or None, info dict, per-class table or None)."""
    from geoguessr_ai_amd import _lib as L
    names = [f"r{r:02d}_hbm_traffic_pmc_{precision}.json" for r in (6, 5, 4, 3, 2)] + (["r01_hbm_traffic_pmc.json"] if precision == "bf16" else [])
    for name in names:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                d = json.load(f)
            val = d["per_kernel_class"]["gemm_nt"]["traffic_bytes_per_launch"]
        except (OSError, KeyError, ValueError):
            continue
        prof_hash = d.get("source_hash")
        return val, dict(file="profiles/" + name, git_head=d.get("git_head"), source_hash=prof_hash,
                         stale=(prof_hash is None or prof_hash != L.source_hash())), d["per_kernel_class"]
    return None, None, None


# kernel class of the bench line -> rocprofv3 kernel classes of tools/pmc_traffic.py that make it up
PMC_CLASSES = {"attention": ("attn",), "dwconv": ("dwconv",), "norm_elementwise": ("bn", "ln"), "data_movement": ("im2col", "col2im")}


def class_rooflines(breakdown_raw, steps, precision, pmc_classes, pmc_info):
    """One roofline-shaped object per non-GEMM kernel class (the GEMM class is the line's `roofline`): attention against the MFMA peak of the mode
    on its ALGORITHMIC flops (4 N^2 D forward, 10 N^2 D backward per window and head), the streaming classes against 8 TB/s on their algorithmic
    bytes; `traffic` = PMC HBM bytes per step of the class (same hash-checked file as `roofline.traffic`), `traffic_ratio` = traffic / algorithmic."""
    out = {}
    for name, (ms_, n_, fl_, by_) in breakdown_raw.items():
        if name not in PMC_CLASSES or ms_ <= 0:
            continue
        traffic = None
        if pmc_classes:
            traffic = sum((pmc_classes.get(k, {}).get("fetch_GB_per_step", 0.0) + pmc_classes.get(k, {}).get("write_GB_per_step", 0.0)) for k in PMC_CLASSES[name]) * 1e9
        alg_bytes_step = by_ / steps
        if name == "attention":
            # the window attention of both f32-storage modes runs on split products (csrc/attention_split.h: six bf16 MFMAs per f32 product), so its matrix roof is the
            # bf16 peak / 6, as for the split GEMMs -- not the f32 MFMA peak, a pipe these kernels do not use.  The class is priced against whichever roof bounds it:
            # max(flops / matrix roof, algorithmic bytes / 8 TB/s); the other fraction is reported beside it
            peak = SPLIT_PEAK_TF if precision in ("fp32", "fp32_split") else MFMA_PEAK_TF[precision]
            ach, ach_gb = fl_ / ms_ / 1e9, by_ / ms_ / 1e6
            t_mfma, t_hbm = fl_ / (peak * 1e9), by_ / (HBM_PEAK_GBS * 1e6)
            if t_mfma >= t_hbm:
                o = dict(bound="mfma", achieved=round(ach, 2), peak=round(peak, 1), unit="TFLOP/s", frac=round(ach / peak, 4), hbm_frac=round(ach_gb / HBM_PEAK_GBS, 4))
            else:
                o = dict(bound="hbm", achieved=round(ach_gb, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach_gb / HBM_PEAK_GBS, 4), mfma_frac=round(ach / peak, 4))
            o["algorithmic_gflop_per_step"] = round(fl_ / steps / 1e9, 1)
        else:
            ach = by_ / ms_ / 1e6
            o = dict(bound="hbm", achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach / HBM_PEAK_GBS, 4))
        o.update(ms_per_step=round(ms_ / steps, 3), launches_per_step=n_ // steps, algorithmic_bytes_per_step=int(alg_bytes_step),
                 traffic=(int(traffic) if traffic else None), traffic_ratio=(round(traffic / alg_bytes_step, 3) if traffic and alg_bytes_step else None),
                 traffic_stale=(pmc_info or {}).get("stale"))
        out[name] = o
    return out


def class_profile(fn, steps, wall_ms, peak_tf):
    """Roofline-shaped objects for one secondary workload: `steps` instrumented calls (the library's per-launch HIP-event log: class, ms, algorithmic flops and
    bytes; HIP graphs are off while it is on), summed per kernel class.  A class is priced against the roof that bounds it -- max(flops / MFMA peak of the
    mode, bytes / 8 TB/s) -- and the workload as a whole reports its launches per step and the share of the un-instrumented wall time its kernels fill
    (`gpu_busy_frac`: what is left is launch latency -- the launch-bound configs)."""
    import torch
    import ctypes as C
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    lib.gg_prof_reset(); lib.gg_prof_enable(1)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    tot = {c: [0.0, 0, 0.0, 0.0] for c in range(len(CATS))}
    cat, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    for i in range(lib.gg_prof_count()):
        L.check(lib.gg_prof_record(i, C.byref(cat), C.byref(ms), C.byref(fl), C.byref(by)), "gg_prof_record")
        t = tot[cat.value & 15]
        t[0] += ms.value; t[1] += 1; t[2] += fl.value; t[3] += by.value
    lib.gg_prof_reset()
    classes = {}
    for c, name in enumerate(CATS):
        ms_, n_, fl_, by_ = tot[c]
        if n_ == 0 or ms_ <= 0:
            continue
        t_mfma, t_hbm = fl_ / (peak_tf * 1e9), by_ / (HBM_PEAK_GBS * 1e6)            # ms at either roof
        if t_mfma >= t_hbm:
            ach = fl_ / ms_ / 1e9
            o = dict(bound="mfma", achieved=round(ach, 2), peak=peak_tf, unit="TFLOP/s", frac=round(ach / peak_tf, 4))
        else:
            ach = by_ / ms_ / 1e6
            o = dict(bound="hbm", achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach / HBM_PEAK_GBS, 4))
        o.update(ms_per_step=round(ms_ / steps, 4), launches_per_step=n_ // steps, algorithmic_gflop_per_step=round(fl_ / steps / 1e9, 3),
                 algorithmic_bytes_per_step=int(by_ / steps), traffic=None)
        classes[name] = o
    busy = sum(t[0] for t in tot.values()) / steps
    return dict(class_rooflines=classes, launches_per_step=sum(t[1] for t in tot.values()) // steps, gpu_busy_ms_per_step=round(busy, 4),
                gpu_busy_frac=round(min(1.0, busy / max(wall_ms, 1e-9)), 4))


def secondary_cases(dev, budget_s=15.0):
    """BASELINE.json configs other than the headline, timed in the same process on the same device with the protocol of tools/bench_secondary.py
    (W warm-up calls, K timed calls between synchronisations), bounded to ~`budget_s` seconds in total:
      c1  TinyViT-5M-224, batch 8 single images, forward + geocell hard-CE + backward + AdamW (fp32)
      c4  CLIP ViT-B/32 vision tower inference, batch 1024, fp32 (the reference's precision) and fp16 (BASELINE's), mean over all 50 tokens
      c5  SuperGuessr serving head + ProtoRefiner on precomputed (4096, 4, 576) embeddings (this rank's shard of the 8-GPU config: no exchange)"""
    import numpy as np
    import torch
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.models.proto_refiner import ProtoRefiner
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    from geoguessr_ai_amd.optim import AdamW
    t_start = time.perf_counter()
    out = {}

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    def cleanup():
        gc.collect(); torch.cuda.empty_cache()

    try:
        torch.manual_seed(0)
        base = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="fp32")
        model = SuperGuessr(base, panorama=False, should_smooth_labels=False, serving=False).to(dev).train()
        opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
        g = torch.Generator(device=dev).manual_seed(330)
        x = torch.randn(8, 3, 224, 224, device=dev, generator=g)
        lab = torch.stack([torch.rand(8, device=dev, generator=g) * 360 - 180, torch.rand(8, device=dev, generator=g) * 180 - 90], 1)
        clf = torch.randint(0, model.num_cells, (8,), device=dev, generator=g)

        def c1():
            o = model(pixel_values=x, labels=lab, labels_clf=clf)
            o.loss.backward(); opt.step(); opt.zero_grad()
        dt = timed(c1, 15, 4)
        out["c1"] = dict(workload="tiny_vit_5m_224, batch 8 single images, fwd + hard-CE + bwd + AdamW", dtype="fp32", ms_per_step=round(dt * 1e3, 3), images_per_s=round(8 / dt, 1),
                         **class_profile(c1, 3, dt * 1e3, 157.3))
        del model, base, opt, x
        cleanup()
        # the serving call of the reference's inference.py:162-170 on ONE panorama (4 headings through TinyViT-21M + the geocell head): latency with the GPU drained
        # after every call -- the launch-bound end of the path (64 x 64 small-M GEMM tiles, split-K, captured HIP graph)
        base = TinyViTAdapter("tiny_vit_21m_224", pretrained=False, precision="fp32")
        model = SuperGuessr(base, panorama=True, serving=True).to(dev).eval()
        xs = torch.randn(1, 4, 3, 224, 224, device=dev)
        dummy = torch.zeros(1, dtype=torch.long, device=dev)
        with torch.no_grad():
            for _ in range(5):
                model(pixel_values=xs, labels_clf=dummy)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(30):
                model(pixel_values=xs, labels_clf=dummy)
                torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 30
        def serve():
            with torch.no_grad():
                model(pixel_values=xs, labels_clf=dummy)
        out["serve_1_panorama"] = dict(workload="tiny_vit_21m_224 + geocell head, serving call on 1 panorama (4 images), synchronised after every call", dtype="fp32",
                                       latency_ms=round(dt * 1e3, 3), panoramas_per_s=round(1 / dt, 1), **class_profile(serve, 3, dt * 1e3, 157.3))
        del model, base, xs
        cleanup()
        for prec in ("fp32", "fp16"):
            tower = CLIPVisionTower("openai/clip-vit-base-patch32", precision=prec).to(dev).eval()
            for p_ in tower.parameters():
                p_.requires_grad = False
            xc = torch.randn(1024, 3, 224, 224, device=dev)
            with torch.no_grad():
                dt = timed(lambda: tower(pixel_values=xc, return_last_hidden=False), 3 if prec == "fp32" else 10, 1 if prec == "fp32" else 2)
            peak = 157.3 if prec == "fp32" else 2500.0
            tf = 1024 / dt * 8.82e9 / 1e12
            def c4():
                with torch.no_grad():
                    tower(pixel_values=xc, return_last_hidden=False)
            out["c4_" + prec] = dict(workload="CLIP ViT-B/32 vision tower inference (random weights), batch 1024", dtype=prec, ms_per_step=round(dt * 1e3, 3),
                                     images_per_s=round(1024 / dt, 1), tflops=round(tf, 1), frac_of_mfma_peak=round(tf / peak, 4), **class_profile(c4, 2, dt * 1e3, peak))
            del tower, xc
            cleanup()
        Bq, D = 4096, 576
        head = SuperGuessr(None, panorama=True, serving=True, embed_dim=D, precision="fp32_split").to(dev).eval()      # (the headline mode: the geocell Linear as a split product)
        K = head.num_cells
        rng = np.random.default_rng(0)
        counts = rng.poisson(4.0, K)
        gi = np.repeat(np.arange(K), counts)
        refiner = ProtoRefiner.from_clusters(gi, rng.standard_normal((len(gi), D), dtype=np.float32), rng.uniform(-180, 180, len(gi)).astype(np.float32),
                                             rng.uniform(-90, 90, len(gi)).astype(np.float32), K, topk=5).to(dev).eval()
        emb = torch.randn(Bq, 4, D, device=dev)

        def c5():
            with torch.no_grad():
                llh, topk, e = head(embedding=emb)
                refiner(e, llh, topk.indices, topk.values)
        dt = timed(c5, 10, 3)
        out["c5"] = dict(workload="SuperGuessr serving head (576 -> 12647, softmax, top-5) + ProtoRefiner on precomputed embeddings, batch 4096 per GPU", dtype=DTYPE_LABEL["fp32_split"],
                         prototypes=int(len(gi)), ms_per_step=round(dt * 1e3, 3), samples_per_s=round(Bq / dt, 1), **class_profile(c5, 3, dt * 1e3, SPLIT_PEAK_TF))      # (the head GEMM is a split product: priced against the bf16 matrix peak / 6)
        del head, refiner, emb
        cleanup()
    except Exception as e:           # the secondary block must never cost the headline line
        out["error"] = f"{type(e).__name__}: {e}"
    out["seconds"] = round(time.perf_counter() - t_start, 1)
    return out


def count_gpus_without_runtime():
    """GPUs this process would see, counted WITHOUT loading the HIP / HSA runtime (torch.cuda.device_count() falls back to hipGetDeviceCount on
    builds without amdsmi): readable KFD topology nodes with a non-zero simd_count; HIP_/ROCR_VISIBLE_DEVICES
    narrow the set.  None = unknown."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    if not os.path.isdir(base):
        return 0                                  # no amdgpu compute driver on this host
    n, unknown = 0, False
    try:
        nodes = os.listdir(base)
    except OSError:
        nodes, unknown = [], True
    for node in nodes:
        try:
            with open(os.path.join(base, node, "properties")) as f:
                props = dict(ln.split(None, 1) for ln in f if " " in ln)
            if int(props.get("simd_count", "0").strip() or 0) <= 0:
                continue                          # a CPU node
            n += 1
        except PermissionError:
            continue                              # a GPU of the host this container was not given (its topology node is unreadable)
        except (OSError, ValueError):
            unknown = True                        # cannot tell
    vis = None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            k = len([t for t in v.split(",") if t.strip() != ""])
            vis = k if vis is None else min(vis, k)
    if unknown and n == 0:
        return vis                                # None when nothing narrows it either
    return n if vis is None else min(n, vis)


def self_launch(args) -> int:
    """``python bench.py --gpus N`` (N > 1) without a launcher in front: start the driver's own launch line
    (``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...``) as a CHILD
    process group, relay rank 0's JSON line and return the child's exit code.  This process never loads the HIP runtime (devices are counted
    from the KFD topology in sysfs), and the launch is a spawn + wait, never an exec.  Fails loudly when the box has fewer than N GPUs -- an
    N-GPU number must come from N devices -- and when the ranks have not finished within GG_BENCH_LAUNCH_TIMEOUT seconds (default 480: a
    hung RCCL bootstrap must not sit silently until the caller's own limit): the child's process group is then killed and the tail of its
    stderr printed."""
    import collections
    import signal
    import socket
    import subprocess
    import threading
    have = count_gpus_without_runtime()
    if have is not None and have < args.gpus and not os.environ.get("GG_BENCH_ONE_DEVICE"):
        print(f"bench.py: --gpus {args.gpus} requested but this machine exposes {have} GPU(s); refusing to report an {args.gpus}-GPU number "
              f"from fewer devices (GG_BENCH_ONE_DEVICE=1 GG_DIST_BACKEND=gloo rehearses the multi-rank path on one GPU)", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    # multi-process GPU work on this image: the host driver only supports dmabuf IPC, and without this RCCL's peer-memory registration
    # fails with `hipIpcGetMemHandle: invalid argument` (already exported on the driver's boxes; set here for a bare shell)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    limit = float(os.environ.get("GG_BENCH_LAUNCH_TIMEOUT", "480"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: starting " + " ".join(cmd), file=sys.stderr)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, start_new_session=True)
    err_tail = collections.deque(maxlen=40)
    lines = [0]

    def pump_err():
        for ln in proc.stderr:
            err_tail.append(ln); sys.stderr.write(ln)

    def pump_out():
        for ln in proc.stdout:                 # rank 0 prints exactly one JSON line; anything else on stdout goes to our stderr
            if ln.startswith("{") and '"metric"' in ln:
                sys.stdout.write(ln); sys.stdout.flush(); lines[0] += 1
            else:
                sys.stderr.write(ln)

    threads = [threading.Thread(target=pump_err, daemon=True), threading.Thread(target=pump_out, daemon=True)]
    for t in threads:
        t.start()
    try:
        rc = proc.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGTERM)          # the session we started: torchrun + its ranks, nothing else
            try:
                proc.wait(timeout=10)
            except subprocess.TimeoutExpired:
                os.killpg(proc.pid, signal.SIGKILL)
                proc.wait()
        except ProcessLookupError:
            pass
        for t in threads:
            t.join(timeout=2)
        print(f"bench.py: the {args.gpus}-rank run did not finish within {limit:.0f} s (GG_BENCH_LAUNCH_TIMEOUT) and was killed; last stderr lines of the ranks:\n"
              + "".join(err_tail), file=sys.stderr)
        return 4
    for t in threads:
        t.join(timeout=5)
    if rc == 0 and lines[0] != 1:
        print(f"bench.py: the {args.gpus}-rank run printed {lines[0]} result lines instead of 1", file=sys.stderr)
        return 3
    return rc


def allreduce_cost(opt, dev, world, reps=5):
    """What the step's gradient exchange costs when nothing hides it: the same buckets (flat trainable ranges + the head's weight / bias),
    summed in place ``reps`` times between device synchronisations on scratch copies.  In the timed step these all-reduces ride under the
    backward pass (bucket launch from the stage callback), so this is an upper bound of their exposed share."""
    import torch
    import torch.distributed as dist
    shapes = [bb.flat_grads()[s:e] for bb in opt.backbones for s, e in bb.trainable_ranges()] + [p.data for p in opt.loose]   # (the head's .grad is None after zero_grad)
    bufs = [torch.zeros_like(t) for t in shapes]
    nbytes = sum(b.numel() * b.element_size() for b in bufs)
    for b in bufs:
        dist.all_reduce(b)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        for b in bufs:
            dist.all_reduce(b)
    torch.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0) / reps
    t = torch.tensor([ms], device=dev, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ms = float(t.item())
    # ring all-reduce moves 2 (n-1)/n of the payload per rank
    return dict(allreduce_ms_per_step=round(ms, 3), allreduce_bytes_per_step=nbytes, allreduce_buckets=len(bufs),
                allreduce_bucket_bytes=[b.numel() * b.element_size() for b in bufs],
                allreduce_busbw_gbps=round(2 * (world - 1) / world * nbytes / max(ms, 1e-9) / 1e6, 1))


def dump_outputs(dump_dir, model, out):
    """What the last timed step handed its caller -- the ModelOutput fields and the parameters AdamW wrote -- as float32 / float64 .npy files
    under `dump_dir` (about 7 MB at the default size), so that two builds can be compared output for output on the same seeded inputs.
    Integer outputs go out as float64 (exact).  Of the ~16 M trainable parameters a fixed seeded sample of 2^20 is kept, and any output above
    2^22 elements (larger --panoramas) is sampled the same way, which keeps the total under 64 MB."""
    import numpy as np

    def sample(a, n):
        if a.size <= n:
            return a
        return a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, size=n, replace=False))]

    os.makedirs(dump_dir, exist_ok=True)
    f32 = lambda t: t.detach().float().cpu().numpy()
    f64 = lambda t: t.detach().double().cpu().numpy()
    arrays = dict(loss=f32(out.loss), preds_LLH=f32(out.preds_LLH), preds_geocell=f64(out.preds_geocell),
                  top5_values=f32(out.top5_geocells.values), top5_indices=f64(out.top5_geocells.indices), embedding=f32(out.embedding))
    arrays = {k: sample(a, 1 << 22) for k, a in arrays.items()}
    arrays["params_sample"] = sample(np.concatenate([f32(p).reshape(-1) for p in model.parameters() if p.requires_grad]), 1 << 20)
    for name, a in arrays.items():
        np.save(os.path.join(dump_dir, name + ".npy"), a)


def run_mode(precision, args, rank, world, dev, x, lab, dump_dir=None):
    """W warm-up steps, exactly K timed steps (barrier + synchronize on both sides, max over ranks); with --full an instrumented replay."""
    import torch
    import torch.distributed as dist
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.optim import AdamW

    torch.manual_seed(0)
    base = TinyViTAdapter(args.model, pretrained=False, precision=precision)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True, serving=False).to(dev).train()
    if args.unfrozen:
        base.unfreeze_all()
    opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)    # main_coordinator_idun_s3.py:246-248
    opt.broadcast_params()                                                # DDP start-up: every rank begins with rank 0's weights
    N = x.shape[0]

    def step():
        if world > 1:
            opt.broadcast_buffers()                      # DDP(broadcast_buffers=True) before every training forward, as training/train_eval_loop.py does
        with opt.overlap_allreduce():                    # gradient buckets leave while the backward pass is still running
            out = model(pixel_values=x, labels=lab)      # nearest-centroid labels + soft targets fused in the head kernel
            out.loss.backward()
        opt.allreduce_grads()
        opt.step()
        opt.zero_grad()
        return out

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        out = step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    loss = float(out.loss.detach())
    images = args.steps * N * 4 * world
    res = dict(value=round(images / dt, 2), ms_per_step=round(1e3 * dt / args.steps, 3), loss=round(loss, 5))
    if dump_dir:
        dump_outputs(dump_dir, model, out)          # before anything below steps the model again
    if world > 1 and args.full:
        res.update(allreduce_cost(opt, dev, world))

    if args.full and not args.no_roofline:
        lib = L.lib()
        lib.gg_prof_reset(); lib.gg_prof_enable(1)
        sync()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync()
        dt_prof = time.perf_counter() - t1
        lib.gg_prof_enable(0)
        peak_tf = MFMA_PEAK_TF[precision]
        tot = {c: [0.0, 0, 0.0, 0.0] for c in range(len(CATS))}        # ms, launches, flops, bytes
        ideal_ms, mfma_bound_ms = 0.0, 0.0
        split_tot = [0.0, 0, 0.0, 0.0]
        cat, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        launches = []
        for i in range(lib.gg_prof_count()):
            L.check(lib.gg_prof_record(i, C.byref(cat), C.byref(ms), C.byref(fl), C.byref(by)), "gg_prof_record")
            cv, is_split = cat.value & 15, bool(cat.value & 16)            # bit 4: a split-bf16 GEMM (csrc/prof.h)
            launches.append((cv, ms.value, fl.value, by.value))
            t = tot[cv]
            t[0] += ms.value; t[1] += 1; t[2] += fl.value; t[3] += by.value
            if is_split:
                split_tot[0] += ms.value; split_tot[1] += 1; split_tot[2] += fl.value; split_tot[3] += by.value
            if cv == 0:
                tf, tb = fl.value / (peak_tf * 1e9), by.value / (HBM_PEAK_GBS * 1e6)       # ms at the MFMA / HBM roof
                ideal_ms += max(tf, tb)
                mfma_bound_ms += ms.value if tf >= tb else 0.0
        breakdown = {}
        for c, name in enumerate(CATS):
            ms_, n_, fl_, by_ = tot[c]
            breakdown[name] = dict(ms_per_step=round(ms_ / args.steps, 3), launches_per_step=n_ // args.steps,
                                   tflops=round(fl_ / max(ms_, 1e-9) / 1e9, 2) if fl_ else None,
                                   gbps=round(by_ / max(ms_, 1e-9) / 1e6, 1) if by_ else None)
        ms_, n_, fl_, by_ = tot[0]
        ach_tf, ach_gb = fl_ / max(ms_, 1e-9) / 1e9, by_ / max(ms_, 1e-9) / 1e6
        intensity = fl_ / max(by_, 1.0)
        kern = ("gemm_nt_f32_ring_kernel (LDS-DMA ring, single-buffer form; + gemm_tn_f32_kernel weight gradients)" if precision == "fp32"
                else "gemm_nt_split3a/b_kernel (the 80 transformer-block Linears per step: f32 activation split in the loader, weight planes cached) + gemm_nt_f32_ring_kernel (conv stages) + gemm_tn_f32_kernel" if precision == "fp32_split"
                else "gemm_nt_kernel (+ gemm_tn_kernel weight gradients)")
        traffic, traffic_info, pmc_classes = pmc_traffic(precision)
        res["class_rooflines"] = class_rooflines({name: tot[c] for c, name in enumerate(CATS)}, args.steps, precision, pmc_classes, traffic_info)
        common = dict(kernel=kern, traffic=traffic, traffic_source=traffic_info, launches=n_ // args.steps, avg_launch_us=round(1e3 * ms_ / max(n_, 1), 2),
                      gemm_ms_per_step=round(ms_ / args.steps, 3), algorithmic_gflop_per_launch=round(fl_ / max(n_, 1) / 1e9, 3),
                      algorithmic_bytes_per_launch=int(by_ / max(n_, 1)), flop_per_byte=round(intensity, 1),
                      mfma_achieved_tflops=round(ach_tf, 2), mfma_frac=round(ach_tf / peak_tf, 4),
                      hbm_achieved_gbps=round(ach_gb, 1), hbm_frac=round(ach_gb / HBM_PEAK_GBS, 4),
                      per_launch_frac=round(ideal_ms / max(ms_, 1e-9), 4), mfma_bound_time_share=round(mfma_bound_ms / max(ms_, 1e-9), 3))
        if intensity < peak_tf * 1e3 / HBM_PEAK_GBS:
            roof = dict(bound="hbm", achieved=round(ach_gb, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach_gb / HBM_PEAK_GBS, 4), **common)
        else:
            roof = dict(bound="mfma", achieved=round(ach_tf, 2), peak=peak_tf, unit="TFLOP/s", frac=round(ach_tf / peak_tf, 4), **common)
        if precision == "fp32_split" and split_tot[1]:
            # the dominant kernels of this mode are the split GEMMs: their roof is the bf16 matrix peak / 6 (six bf16 products per f32-accurate product)
            sms, sn, sfl, sby = split_tot
            s_tf = sfl / max(sms, 1e-9) / 1e9
            roof = dict(bound="mfma", achieved=round(s_tf, 2), peak=round(SPLIT_PEAK_TF, 1), unit="TFLOP/s (f32-equivalent: 2 M N K per product)", frac=round(s_tf / SPLIT_PEAK_TF, 4),
                        kernel="gemm_nt_split3a/b_kernel + gemm_tn_split3_kernel (f32-accurate products as six v_mfma_f32_16x16x32_bf16 each; f32 operands split in the loader)",
                        bf16_product_tflops=round(6.0 * s_tf, 1), bf16_mfma_peak=2500.0, launches=sn // args.steps, avg_launch_us=round(1e3 * sms / max(sn, 1), 2),
                        split_gemm_ms_per_step=round(sms / args.steps, 3), gemm_ms_per_step=round(ms_ / args.steps, 3),
                        split_share_of_gemm_time=round(sms / max(ms_, 1e-9), 4), split_share_of_gemm_launches=round(sn / max(n_, 1), 4),
                        algorithmic_gflop_per_launch=round(sfl / max(sn, 1) / 1e9, 3), algorithmic_bytes_per_launch=int(sby / max(sn, 1)),
                        all_gemm_f32_equivalent_tflops=round(ach_tf, 2), f32_mfma_peak=peak_tf, all_gemm_vs_f32_mfma_peak=round(ach_tf / peak_tf, 4),
                        traffic=traffic, traffic_source=traffic_info)
        if precision == "fp32" and roof["bound"] == "mfma":
            mhz, per_form = clock_under_gemm_load(dev)
            if mhz:
                pk = peak_tf * mhz / 2400.0
                roof.update(shader_clock_mhz_under_load=round(mhz, 0), shader_clock_mhz_per_form=per_form, peak_at_measured_clock=round(pk, 1),
                            frac_at_measured_clock=round(ach_tf / pk, 4))
        lib.gg_prof_reset()
        if args.dump_launches and rank == 0:
            # one step's launches in issue order (category, ms, algorithmic flops, algorithmic bytes): tools/pmc_traffic.py joins them with the PMC
            # rows of the same kernels by order to get the HBM over-fetch of every GEMM launch form
            per = len(launches) // args.steps
            with open(args.dump_launches + "." + precision + ".json", "w") as f:
                json.dump(dict(precision=precision, cats=CATS, launches=launches[(args.steps - 1) * per:]), f)
        breakdown["instrumented_ms_per_step"] = round(1e3 * dt_prof / args.steps, 3)
        res.update(roofline=roof, kernel_breakdown=breakdown)
    res["step_tflops"] = round(res["value"] * GFLOP_PER_IMAGE / 1e3, 2)
    res["step_frac_of_mfma_peak"] = round(res["value"] * GFLOP_PER_IMAGE / 1e3 / MFMA_PEAK_TF[precision] / world, 4)
    del opt, model, base, out
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--panoramas", type=int, default=256, help="panoramas per GPU per step (BASELINE: 256)")
    ap.add_argument("--model", default="tiny_vit_21m_224")
    ap.add_argument("--precision", default="both", choices=["both", "fp32", "bf16", "fp32_split"],
                    help="both: fp32_split (headline: f32-accurate, split-bf16 products); with --full also fp32 (f32 MFMA GEMMs, under 'fp32') and bf16 (under 'bf16')")
    ap.add_argument("--unfrozen", action="store_true", help="train every parameter instead of the reference freeze policy")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the other precisions, the instrumented roofline replay, the all-reduce cost (N > 1), the secondary configs and the "
                         "CPU baseline (N = 1); a plain run times the headline only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the headline mode's last timed step returned (ModelOutput fields, a seeded sample of the updated parameters) to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="(--full) skip the instrumented roofline replay")
    ap.add_argument("--dump-launches", default=None, help="(--full) write the per-launch (category, ms, flops, bytes) list of one instrumented step to PATH.<precision>.json")
    ap.add_argument("--no-secondary", action="store_true", help="(--full) skip the c1 / c4 / c5 secondary timings (N = 1 only, ~15 s)")
    args = ap.parse_args()
    if args.dump_launches and not args.full:
        ap.error("--dump-launches comes from the instrumented replay of --full")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))          # `python bench.py --gpus N`: become the launcher, BEFORE anything here touches the GPU

    import torch
    import torch.distributed as dist
    from geoguessr_ai_amd import _lib as L

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; launch with "
                 f"`python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} ... bench.py --gpus {args.gpus}` "
                 f"(or run `python bench.py --gpus {args.gpus}` and let it start the ranks itself)")
    L.require_gpu()
    backend = os.environ.get("GG_DIST_BACKEND", "nccl")          # "gloo" + GG_BENCH_ONE_DEVICE=1: rehearsal of the N>1 path on a one-GPU box
    # what carries the gradient buckets: torch.distributed's backend, or -- GG_NATIVE_COMM=1 -- the C-ABI communicator gg_comm_* (RCCL through comm.cpp;
    # torch.distributed then only carries the rendezvous, the barrier and this script's scalar reductions)
    from geoguessr_ai_amd import comm as _gg_comm
    comm_backend = "gg_comm (RCCL behind the C-ABI, csrc/comm.cpp)" if _gg_comm.enabled() else ("rccl (torch.distributed nccl)" if backend == "nccl" else backend)
    if os.environ.get("GG_BENCH_ONE_DEVICE"):
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    rccl_ranks = 1
    if world > 1:      # prove the transport before timing anything: every rank contributes 1 to a sum all-reduce on the device
        one = torch.ones(1, device=dev)
        dist.all_reduce(one)
        rccl_ranks = int(one.item())
        if rccl_ranks != args.gpus:
            sys.exit(f"bench.py: the all-reduce summed {rccl_ranks} ranks, --gpus says {args.gpus}")

    N = args.panoramas
    g = torch.Generator(device=dev).manual_seed(1234 + rank)              # SURVEY.md 8(d) synthetic inputs
    x = torch.randn(N, 4, 3, 224, 224, device=dev, generator=g)
    lab = torch.stack([torch.rand(N, device=dev, generator=g) * 360 - 180, torch.rand(N, device=dev, generator=g) * 180 - 90], 1)

    # Headline = fp32_split: f32 storage and f32-accurate arithmetic in which split-bf16 products (x = x1 + x2 + x3 in bf16, six bf16 MFMAs per product,
    # f32 accumulation) carry 80 % of the GEMM time (every Linear and weight gradient of the transformer blocks, the forward convolutions of the ConvNorms) and the window
    # attention; error against fp64 at or below the f32 MFMA kernels' per shape, the fp32 mode's parity gate at the fp32 mode's tolerances
    # (tests/test_gpu_precision.py::test_fp32_split_mode_passes_the_fp32_gate).  VERDICT r4 item 6 set exactly this bar for the mode to become the headline dtype,
    # labelled "fp32 (bf16x3 split MFMA)".  A plain run times the headline mode alone; --full times the plain f32-MFMA mode ("fp32") and bf16 ("bf16") after
    # it in the same run, so the headline is timed in the same state either way.
    modes = [args.precision] if args.precision != "both" else ["fp32_split", "fp32", "bf16"] if args.full else ["fp32_split"]
    dump_dir = args.dump_outputs if rank == 0 else None
    results = {m: run_mode(m, args, rank, world, dev, x, lab, dump_dir=dump_dir if m == modes[0] else None) for m in modes}
    head = results[modes[0]]

    secondary = None
    if args.full and rank == 0 and world == 1 and not args.no_secondary:
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):       # the shims print like the reference does; stdout carries the one JSON line only
            secondary = secondary_cases(dev)
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline()

    if rank == 0:
        line = dict(metric="images/sec TinyViT-21M-224 train, 4-heading batch", value=head["value"], unit="images/s",
                    n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=head["ms_per_step"],
                    higher_is_better=True, scaling="weak", vs_baseline=None, dtype=DTYPE_LABEL.get(modes[0], modes[0]), data="synthetic",
                    config=dict(workload=f"{args.model} 4x224x224 panoramas, fwd+bwd+AdamW, soft-CE over 12647 geocells, "
                                         f"{'all params' if args.unfrozen else 'freeze_all_but_last_stage'}, DropPath, train-mode BN",
                                panoramas_per_gpu=N, images_per_gpu=N * 4, global_batch_panoramas=N * world, parallelism=f"dp{world}",
                                precision=modes[0], **({"buffer_broadcast": "BatchNorm running statistics from rank 0 before every forward"} if world > 1 else {})),
                    rccl_ranks=rccl_ranks, comm_backend=(comm_backend if world > 1 else None),
                    allreduce_ms_per_step=head.get("allreduce_ms_per_step"), allreduce_bytes_per_step=head.get("allreduce_bytes_per_step"),
                    allreduce_busbw_gbps=head.get("allreduce_busbw_gbps"), allreduce_buckets=head.get("allreduce_buckets"),
                    allreduce_bucket_bytes=head.get("allreduce_bucket_bytes"),
                    step_tflops=head["step_tflops"], step_frac_of_mfma_peak=head["step_frac_of_mfma_peak"], loss=head["loss"],
                    roofline=head.get("roofline"), cpu_baseline=cpu, class_rooflines=head.get("class_rooflines"),
                    kernel_breakdown=head.get("kernel_breakdown"), secondary=secondary)
        for m in modes[1:]:
            line[m] = dict(dtype=DTYPE_LABEL.get(m, m), **results[m])
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
