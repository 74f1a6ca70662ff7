"""The backward of patch_embed.conv2 on its two fp32_split routes -- the data gradient by input parity (include/gg_conv_dgrad_parity.h; csrc/tinyvit.hip
patch_embed_bwd) and the resident weight gradient (include/gg_wgrad_resident.h; dense_wgrad) -- against the schedule without them, in one model step.
Run by tests/test_gpu_patch_embed_bwd.py::test_routing_changes_only_patch_embed_gradients in a subprocess under GG_DEV_SWITCHES=1 GG_SPLIT_MIN_TILES=1 (without the
lowered tile threshold the split routes are not taken at a batch this small).

tiny_vit_21m_224, 8 images (2 panoramas), reference freeze policy: one forward + backward from the same state with both routes on (GG_SPLIT_TN_RESIDENT_MIN_M=1: conv2's
25 088 rows qualify) and with both off (the threshold out of reach, GG_NO_PE2_DGRAD_PARITY=1; both switches are read per call, the captured graphs are cleared in
between).  The routes replace launches that feed nothing but the gradients of patch_embed.conv2.weight (the weight gradient) and of patch_embed.conv1 (dz1), so
  * the loss, the embedding and every other gradient are equal element for element (torch.equal after + 0.0; the attention-bias tables of the trainable blocks,
    summed with float atomics, to 1e-5 of their largest magnitude);
  * the two convolution weights' gradients agree to rel-L2 2e-5, the tolerance the f32 kernels are held to against fp64 (tests/test_gpu_guards.py), BatchNorm1's
    parameter gradients -- sums over 100 352 pixels that cancel -- to 1e-4; all far inside the fp32 gate's 2e-3 per tensor; none is bit-equal (the routes were taken);
  * the split launch count is exactly one higher with the routes on and the f32-MFMA count one lower (the weight gradient; the data gradient replaces a split
    product by a split product).
Exit code 0 and one "-> ok" line."""
import ctypes as C
import gc
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

MODEL, PANOS = "tiny_vit_21m_224", 2
W2 = "patch_embed.conv2.conv.weight"


def _gemm_launches(lib, L):
    """(split-flagged, plain) GEMM launches in the profiler's log."""
    cat = C.c_int()
    split = plain = 0
    for i in range(lib.gg_prof_count()):
        L.check(lib.gg_prof_record(i, C.byref(cat), None, None, None), "gg_prof_record")
        split += cat.value == 16
        plain += cat.value == 0
    return split, plain


def run(on: bool):
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from tests.test_gpu_precision import _randomize
    lib = L.lib()
    lib.gg_graph_clear()
    os.environ["GG_SPLIT_TN_RESIDENT_MIN_M"] = "1" if on else str(1 << 40)
    if not on:
        os.environ["GG_NO_PE2_DGRAD_PARITY"] = "1"
    torch.manual_seed(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(MODEL, pretrained=False, precision="fp32_split", drop_path_rate=0.0)
    _randomize(base.backbone, 6)
    model = SuperGuessr(base.cuda(), panorama=True, should_smooth_labels=True).cuda().train()      # the reference freeze policy
    g = torch.Generator().manual_seed(7)
    x = torch.randn(PANOS, 4, 3, 224, 224, generator=g).cuda()
    labels = torch.stack([torch.rand(PANOS, generator=g) * 360 - 180, torch.rand(PANOS, generator=g) * 180 - 90], 1).cuda()
    lib.gg_prof_reset(); lib.gg_prof_enable(1)
    out = model(pixel_values=x, labels=labels)
    out.loss.backward()
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    rec = {"loss": out.loss.detach().clone(), "embedding": out.embedding.detach().clone(), "launches": _gemm_launches(lib, L)}
    lib.gg_prof_reset()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, n
            rec["grad " + n] = p.grad.detach().clone()
    del model, base, out
    gc.collect(); torch.cuda.empty_cache()
    lib.gg_graph_clear()
    os.environ.pop("GG_SPLIT_TN_RESIDENT_MIN_M")
    os.environ.pop("GG_NO_PE2_DGRAD_PARITY", None)
    return rec


def main():
    assert os.environ.get("GG_DEV_SWITCHES") and os.environ.get("GG_SPLIT_MIN_TILES") == "1", "run under GG_DEV_SWITCHES=1 GG_SPLIT_MIN_TILES=1"
    on, off = run(True), run(False)
    assert set(on) == set(off), sorted(set(on) ^ set(off))
    pe = {k: (1e-4 if ".bn." in k else 2e-5) for k in on if k.startswith("grad ") and (k.endswith(W2) or "patch_embed.conv1." in k)}
    assert sum(k.endswith(W2) for k in pe) == 1 and len(pe) == 4, sorted(k for k in on if "patch_embed" in k)
    bad, rels = [], {}
    for key in on:
        if key == "launches":
            continue
        if key in pe:
            a, b = on[key].double(), off[key].double()
            rels[key] = float((a - b).norm() / b.norm())
            if not 0.0 < rels[key] < pe[key]:
                bad.append(f"{key}: rel-L2 {rels[key]:.3e} (bound {pe[key]:.0e}; 0 = the route was not taken)")
        elif key.endswith("attention_biases"):
            # summed with float atomics in LDS (attention_split.h): the last bits differ between any two runs of ONE schedule (tests/test_gpu_recompute.py's tolerance)
            if float((on[key].double() - off[key].double()).abs().max()) > 1e-5 * float(off[key].double().abs().max()):
                bad.append(key)
        elif not torch.equal(on[key] + 0.0, off[key] + 0.0):
            bad.append(key)
    (s_on, p_on), (s_off, p_off) = on["launches"], off["launches"]
    print(f"[patch_embed.conv2 backward routes, {MODEL} {4 * PANOS} images] loss {float(on['loss']):.6f} / {float(off['loss']):.6f}; {len(on) - 3 - len(pe)} other gradients "
          f"compared for equality; rel-L2 on vs off: " + ", ".join(f"{k[5:]} {v:.3e}" for k, v in rels.items()) + f"; GEMM launches split {s_on} / {s_off}, f32-MFMA {p_on} / {p_off}",
          flush=True)
    if s_on != s_off + 1 or p_on != p_off - 1:
        bad.append(f"launch counts split {s_on} / {s_off}, f32-MFMA {p_on} / {p_off}")
    if bad:
        print(f"patch_embed backward routing -> FAIL: {bad[:20]}", flush=True)
        return 1
    print("patch_embed backward routing -> ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
