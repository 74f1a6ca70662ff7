"""Activation recompute (TinyVitBackbone.set_grad_checkpointing): time and peak memory of the training step with and without it.

Cases (one GPU, bench.py's step: SuperGuessr on panoramas of 4 headings, smooth-label loss, forward + backward + AdamW):
  c2            tiny_vit_21m_224, 256 panoramas = 1024 images, fp32_split (the headline mode), reference freeze policy, recompute off and on;
  default512    tiny_vit_21m_512 (the reference's default model), 128 panoramas = 512 images, fp32, every tensor trainable, recompute on
                (without recompute its workspace plan is 359.5 GiB: it does not fit the card).
Per case: ms per step (median of the timed steps; forward and backward split by events around loss.backward()), torch.cuda.max_memory_allocated
over the timed steps, and the planned workspace.  One JSON line per case.

    python tools/bench_recompute.py [--steps 5] [--warmup 2] [--cases c2,default512]
"""
import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_case(name, model_name, panoramas, precision, policy, recompute, steps, warmup):
    import torch
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.optim import AdamW

    dev = torch.device("cuda:0")
    gc.collect(); torch.cuda.empty_cache()
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(model_name, pretrained=False, precision=precision, grad_checkpointing=recompute)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True, serving=False).to(dev).train()
    if policy == "all":
        base.unfreeze_all()
    else:
        base.freeze_all_but_last_stage()
    opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
    bb = base.backbone
    S = bb.cfg.img_size
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(panoramas, 4, 3, S, S, device=dev, generator=g)
    lab = torch.stack([torch.rand(panoramas, device=dev, generator=g) * 360 - 180, torch.rand(panoramas, device=dev, generator=g) * 180 - 90], 1)
    plan = L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(bb.cfg), panoramas * 4, 1, bb.trainable_mask())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fwd, bwd, tot, losses = [], [], [], []
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        ev[0].record()
        out = model(pixel_values=x, labels=lab)
        ev[1].record()
        out.loss.backward()
        ev[2].record()
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        if i >= warmup:
            tot.append((time.perf_counter() - t0) * 1e3)
            fwd.append(ev[0].elapsed_time(ev[1]))
            bwd.append(ev[1].elapsed_time(ev[2]))
            losses.append(round(float(out.loss.detach()), 6))
        del out
    peak = torch.cuda.max_memory_allocated()
    res = dict(case=name, model=model_name, images=panoramas * 4, precision=precision, policy=policy, recompute=int(recompute),
               ms_per_step=round(statistics.median(tot), 2), forward_ms=round(statistics.median(fwd), 2), backward_ms=round(statistics.median(bwd), 2),
               max_memory_allocated_GiB=round(peak / 2 ** 30, 2), workspace_plan_GiB=round(plan / 2 ** 30, 2), losses=losses,
               steps=steps, warmup=warmup, device=torch.cuda.get_device_name(0))
    del model, base, opt, bb, x
    gc.collect(); torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="c2,default512")
    args = ap.parse_args()
    want = set(args.cases.split(","))
    cases = []
    if "c2" in want:
        cases += [("c2", "tiny_vit_21m_224", 256, "fp32_split", "freeze", False), ("c2", "tiny_vit_21m_224", 256, "fp32_split", "freeze", True)]
    if "default512" in want:
        cases += [("default512", "tiny_vit_21m_512", 128, "fp32", "all", True)]
    for c in cases:
        print(json.dumps(run_case(*c, steps=args.steps, warmup=args.warmup)), flush=True)


if __name__ == "__main__":
    main()
