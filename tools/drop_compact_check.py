"""DropPath row compaction of the fp32_split TinyViT step (include/gg_drop.h, csrc/tinyvit.hip block_compacts) against the uncompacted schedule, bit for bit.
Run by tests/test_gpu_drop_compact.py::test_model_steps_are_bit_identical in a subprocess under GG_DEV_SWITCHES=1 GG_SPLIT_MIN_TILES=1 (the dev switches are read
once per process; without the lowered tile threshold the split routes -- and with them the compaction -- are not taken at a batch this small).

tiny_vit_21m_224, 8 images (2 panoramas), reference freeze policy (plus the trainable blocks' attention-bias tables, see run()), drop_path_rate 0.5: three AdamW steps with compaction on, then the same three steps from the
same state with it off.  Everything a step hands back must compare equal element for element (torch.equal after + 0.0, which only folds -0 onto +0): the loss, the
embedding, the retained taps of every block (x2 / attn.out / out; x1 where the plan keeps it), every parameter gradient, the BatchNorm running statistics.  The split
launch count must be the same in both runs, and the declared split flops smaller with compaction (the launches stay, their rows shrink).  Then once more with
grad_checkpointing=True (the recompute replay reads the forward's kept lists).  Exit code 0 and one "-> ok" line per case."""
import ctypes as C
import gc
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

MODEL, PANOS, STEPS, RATE = "tiny_vit_21m_224", 2, 3, 0.5


def _split_launches(lib, L):
    """(count, declared flops) of the split-flagged GEMM launches in the profiler's log."""
    cat, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    n, flops = 0, 0.0
    for i in range(lib.gg_prof_count()):
        L.check(lib.gg_prof_record(i, C.byref(cat), C.byref(ms), C.byref(fl), C.byref(by)), "gg_prof_record")
        if cat.value == 16:
            n += 1
            flops += fl.value
    return n, flops


def run(compact: bool, ckpt: bool):
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.optim import AdamW
    from tests.test_gpu_precision import _randomize
    lib = L.lib()
    lib.gg_graph_clear()
    lib.gg_tinyvit_set_drop_compact(int(compact))
    torch.manual_seed(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(MODEL, pretrained=False, precision="fp32_split", drop_path_rate=RATE, grad_checkpointing=ckpt)
    _randomize(base.backbone, 6)
    model = SuperGuessr(base.cuda(), panorama=True, should_smooth_labels=True).cuda().train()      # the reference freeze policy
    bb = base.backbone
    # The attention-bias tables of the TRAINABLE blocks are frozen here: their gradients are summed with float atomics in LDS (attention_split.h, attention_flash.hip), so
    # their last bits differ between any two runs of ONE schedule (tests/test_gpu_recompute.py, tests/test_gpu_graph.py) -- and through AdamW so would every later step
    for n, p in bb.named_parameters():
        if n.endswith("attention_biases"):
            p.requires_grad_(False)
    bb._drop_seed, bb._drop_counter = 20240517, 0                     # the same DropPath masks in both runs
    opt = AdamW(model, lr=1e-3)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(PANOS, 4, 3, 224, 224, generator=g).cuda()
    labels = torch.stack([torch.rand(PANOS, generator=g) * 360 - 180, torch.rand(PANOS, generator=g) * 180 - 90], 1).cuda()
    B = 4 * PANOS
    steps = []
    for k in range(STEPS):
        opt.zero_grad()
        if k == 0:
            lib.gg_prof_reset(); lib.gg_prof_enable(1)                # (with the hooks on the launches read their live counts back: that path runs here too)
        out = model(pixel_values=x, labels=labels)
        out.loss.backward()
        torch.cuda.synchronize()
        rec = {"loss": out.loss.detach().clone(), "embedding": out.embedding.detach().clone()}
        if k == 0:
            lib.gg_prof_enable(0)
            rec["launches"] = _split_launches(lib, L)
            lib.gg_prof_reset()
        for s, depth in enumerate(bb.depths[1:], start=1):
            for i in range(depth):
                for leaf in ("x1", "x2", "attn.out", "out"):
                    name = f"stages.{s}.blocks.{i}.{leaf}"
                    try:
                        rec["tap " + name] = bb.activation(name, B).clone()
                    except L.GgError as exc:                          # a temporary under the freeze policy / a recomputed tensor: not part of what a step hands back
                        assert "not retained" in str(exc), exc
        for n, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None, n
                rec["grad " + n] = p.grad.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        rec["buffers"] = bb._flat_buf.clone()
        rec["counters"] = bb._counters.clone()
        rec["params"] = bb._flat.detach().clone()
        steps.append(rec)
    lib.gg_tinyvit_set_drop_compact(1)
    del model, base, bb, opt, out
    gc.collect(); torch.cuda.empty_cache()
    lib.gg_graph_clear()
    return steps


def same(a, b):
    if a.dtype == torch.uint8:                                        # a tap: raw f32 bytes of the workspace
        a, b = a.view(torch.float32), b.view(torch.float32)
    if a.is_floating_point():
        a, b = a + 0.0, b + 0.0
    return torch.equal(a, b)


def main():
    assert os.environ.get("GG_DEV_SWITCHES") and os.environ.get("GG_SPLIT_MIN_TILES") == "1", "run under GG_DEV_SWITCHES=1 GG_SPLIT_MIN_TILES=1"
    ok = True
    for ckpt in (False, True):
        label = f"drop compaction {MODEL} {4 * PANOS} images drop_path_rate {RATE}{' grad_checkpointing' if ckpt else ''}"
        on, off = run(True, ckpt), run(False, ckpt)
        bad = []
        for k, (a, b) in enumerate(zip(on, off)):
            assert set(a) == set(b), sorted(set(a) ^ set(b))
            for key in a:
                if key == "launches":
                    continue
                if not same(a[key], b[key]):
                    bad.append(f"step {k}: {key}")
        (n_on, f_on), (n_off, f_off) = on[0]["launches"], off[0]["launches"]
        taps = sum(1 for key in on[0] if key.startswith("tap "))
        grads = sum(1 for key in on[0] if key.startswith("grad "))
        print(f"[{label}] split launches {n_on} / {n_off}, declared split GFLOP {f_on / 1e9:.2f} (compacted) / {f_off / 1e9:.2f}; compared per step: loss, embedding, "
              f"{taps} taps, {grads} gradients, running statistics, parameters after AdamW; loss {[float(s['loss']) for s in on]}", flush=True)
        if n_on != n_off or n_on == 0:
            bad.append(f"split launch count {n_on} != {n_off}")
        if not f_on < f_off:
            bad.append(f"declared split flops {f_on} not below {f_off}: the compacted schedule was not taken")
        if bad:
            ok = False
            print(f"{label} -> FAIL: {bad[:20]}", flush=True)
        else:
            print(f"{label} -> ok", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
