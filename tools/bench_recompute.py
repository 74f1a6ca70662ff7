"""Activation recompute (TinyVitBackbone.set_grad_checkpointing, CLIPVisionTower.gradient_checkpointing_enable): time and peak memory of the training
step with and without it.

Cases (one GPU, bench.py's step: SuperGuessr on panoramas of 4 headings, smooth-label loss, forward + backward + AdamW):
  c2            tiny_vit_21m_224, 256 panoramas = 1024 images, fp32_split (the headline mode), reference freeze policy, recompute off and on;
  default512    tiny_vit_21m_512 (the reference's default model), 128 panoramas = 512 images, fp32, every tensor trainable, recompute on
                (without recompute its workspace plan is 359.5 GiB: it does not fit the card);
  clip          openai/clip-vit-large-patch14-336 (the reference's CLIP tower), fp32 and bf16, every tensor trainable (the reference's policy without a
                pretrained head): recompute off and on at the largest panorama count whose recompute-off plan fits the card (the plan plus parameters,
                gradients, AdamW state, weight cache and input within 0.94 of the device memory), then recompute on at twice that, which does not
                fit without.  The on / off pair also reports t_on - t_off against the training forward of the same run: the recompute is at most one
                forward minus fc2 and the top layer, so more than 1.05 forwards means a launch re-runs that should not.
Per case: ms per step (median of the timed steps; forward and backward split by events around loss.backward()), torch.cuda.max_memory_allocated
over the timed steps, and the planned workspace.  One JSON line per case.

    python tools/bench_recompute.py [--steps 5] [--warmup 2] [--cases c2,default512,clip]
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


CLIP_MODEL = "openai/clip-vit-large-patch14-336"


def clip_cfg(precision, recompute):
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIP_CONFIGS, _precision_code
    kw = CLIP_CONFIGS[CLIP_MODEL]
    c = L.ClipCfg()
    c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads = kw["hidden_size"], kw["intermediate_size"], kw["num_layers"], kw["num_heads"]
    c.image_size, c.patch_size, c.ln_eps, c.act_dtype, c.recompute = kw["image_size"], kw["patch_size"], 1e-5, _precision_code(precision), int(recompute)
    return c


def clip_largest_panoramas(precision):
    """The largest panorama count (4 images each) whose recompute-off training plan, with everything else the step allocates, fits the card."""
    import torch
    from geoguessr_ai_amd import _lib as L
    lib, c = L.lib(), clip_cfg(precision, 0)
    budget = 0.94 * torch.cuda.get_device_properties(0).total_memory
    # parameters, gradients and the two AdamW moments (f32), the weight cache, the head (12647 x 1024: parameter, gradient, moments)
    fixed = 4 * 4 * lib.gg_clip_param_floats(C.byref(c)) + lib.gg_clip_wcache_bytes(C.byref(c)) + 4 * 4 * 12647 * (c.hidden_size + 1)
    per_pano = 4 * (3 * c.image_size ** 2 * 4) + 4 * 12647 * 4 * 3          # input, logits and their gradient
    need = lambda p: lib.gg_clip_workspace_bytes(C.byref(c), 4 * p, 1, None) + fixed + p * per_pano
    lo, hi = 1, 4096
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if need(mid) <= budget else (lo, mid - 1)
    return lo


def run_case(name, model_name, panoramas, precision, policy, recompute, steps, warmup):
    import torch
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.optim import AdamW

    dev = torch.device("cuda:0")
    gc.collect(); torch.cuda.empty_cache()
    torch.manual_seed(0)
    clip = "clip-vit" in model_name
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if clip:
            from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
            base = CLIPVisionTower(model_name, precision=precision, gradient_checkpointing=recompute)
        else:
            base = TinyViTAdapter(model_name, pretrained=False, precision=precision, grad_checkpointing=recompute)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True, serving=False).to(dev).train()
    if clip:
        assert policy == "all" and all(p.requires_grad for p in base.parameters())
    elif policy == "all":
        base.unfreeze_all()
    else:
        base.freeze_all_but_last_stage()
    opt = AdamW(model, lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
    bb = base.backbone
    S = bb.cfg.image_size if clip else bb.cfg.img_size
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(panoramas, 4, 3, S, S, device=dev, generator=g)
    lab = torch.stack([torch.rand(panoramas, device=dev, generator=g) * 360 - 180, torch.rand(panoramas, device=dev, generator=g) * 180 - 90], 1)
    if clip:
        plan = L.lib().gg_clip_workspace_bytes(C.byref(bb.cfg), panoramas * 4, 1, bb.trainable_mask())
        off_cfg = clip_cfg(precision, 0)
        plan_off = L.lib().gg_clip_workspace_bytes(C.byref(off_cfg), panoramas * 4, 1, bb.trainable_mask())
    else:
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
    if clip:
        res["workspace_plan_without_recompute_GiB"] = round(plan_off / 2 ** 30, 2)
        res["device_memory_GiB"] = round(torch.cuda.get_device_properties(0).total_memory / 2 ** 30, 2)
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
    if "clip" in want:
        for precision in ("fp32", "fp32_split", "bf16"):
            # (fp32_split at the fp32 batch: the same f32 workspace, so that the two modes' step times compare image for image)
            p = clip_largest_panoramas("fp32" if precision == "fp32_split" else precision)
            off = run_case("clip", CLIP_MODEL, p, precision, "all", False, args.steps, args.warmup)
            print(json.dumps(off), flush=True)
            on = run_case("clip", CLIP_MODEL, p, precision, "all", True, args.steps, args.warmup)
            # the recompute is at most one training forward (minus fc2 and the top layer): t_on <= t_off + 1.05 t_forward, all from this run
            on["ms_over_recompute_off"] = round(on["ms_per_step"] - off["ms_per_step"], 2)
            on["time_ratio"] = round(on["ms_per_step"] / off["ms_per_step"], 3)
            on["extra_in_forwards"] = round((on["ms_per_step"] - off["ms_per_step"]) / off["forward_ms"], 3)
            on["within_one_forward"] = bool(on["ms_per_step"] <= off["ms_per_step"] + 1.05 * off["forward_ms"])
            print(json.dumps(on), flush=True)
            big = run_case("clip_2x", CLIP_MODEL, 2 * p, precision, "all", True, args.steps, args.warmup)
            big["fits_without_recompute"] = bool(big["workspace_plan_without_recompute_GiB"] < big["device_memory_GiB"])
            print(json.dumps(big), flush=True)


if __name__ == "__main__":
    main()
