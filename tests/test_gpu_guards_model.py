"""Whole-step memory discipline: every tensor of a TinyViT / CLIP step lives in ONE flat workspace the library sizes itself
(gg_tinyvit_workspace_bytes_masked, gg_clip_workspace_bytes) and carves up with its capacity functions; with activation recompute many activations
share one region that holds the previous segment's bytes whenever a kernel starts.  Here the workspace is a guarded buffer (tests/guards.py) of EXACTLY
the size the library asks for, and

  * the bands either side of it are untouched after the step (an overrun of the last region, an under-sized size query);
  * a step whose workspace started as NaN bytes is bit-identical to the step whose workspace started as zeros: output, flat gradient, running
    statistics, counters -- and so are the second, third and fourth step in the same workspace (the real stale-data case of the recompute region),
    the later ones replayed from the captured graph.  An overrun of one inner region into its neighbour, or a read of bytes nobody wrote, shows here.

The weight cache and the DropPath scales are caller-allocated: they are guarded the same way (the cache starts as the fill, not as zeros).
The one exemption from bit-identity is the one tests/test_gpu_recompute.py states, at its tolerance: the attention-bias tables' gradients are summed
with float atomics in LDS (attention.hip, attention_flash.hip, attention_split.h) -- 1e-5 of their largest magnitude."""
import ctypes as C
import gc

import pytest
import torch

from tests import guards as G
from tests import masks as MASKS
from tests.test_gpu_recompute import _grad_mismatches, _model, _stats, _step

pytestmark = pytest.mark.gpu

# entry points whose buffers the tests of this file guard (the registry tests/test_guards_cpu.py checks against the header)
MODEL_ENTRIES = ("gg_tinyvit_forward", "gg_tinyvit_backward", "gg_tinyvit_refresh_weights", "gg_tinyvit_refresh_weights_masked", "gg_drop_path_scales",
                 "gg_clip_forward", "gg_clip_backward", "gg_clip_refresh_weights")

WS_ROW_BYTES = 64 * 1024          # longer than any row of any tensor inside a workspace (the widest: 4 * 2304 f32 columns): bands of 16 MiB


@pytest.fixture(autouse=True)
def _fresh_graph_cache():
    from geoguessr_ai_amd import _lib as L
    L.lib().gg_graph_clear()
    yield
    L.lib().gg_graph_clear()


def _install(bb, S, batch, training, zero):
    """Guarded workspace of exactly the library's size in bb._ws[training] (TinyVitBackbone._workspace reuses it: numel == need), guarded weight cache."""
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    mask = bb.trainable_mask() if training else None
    need = lib.gg_tinyvit_workspace_bytes_masked(C.byref(bb.cfg), batch, int(training), mask)
    assert need > 0
    ws = S.scratch("workspace", need, row_bytes=WS_ROW_BYTES, zero=zero)
    bb._ws[training] = ws.view[0]
    assert bb._ws[training].numel() == need and bb._ws[training].data_ptr() % 256 == 0
    wc = S.scratch("wcache", lib.gg_tinyvit_wcache_bytes(C.byref(bb.cfg)), row_bytes=WS_ROW_BYTES)
    bb._wcache, bb._wcache_version, bb._dirty_all = wc.view[0], -1, True
    return ws, wc


def _drop_scales(bb, S, batch, seed=11, counter=3):
    from geoguessr_ai_amd import _lib as L
    rates = S.inp("drop_rates", torch.tensor(bb.drop_rates, dtype=torch.float32))
    out = S.out("drop_scales", bb.num_drop_slots, batch, torch.float32)
    L.check(L.lib().gg_drop_path_scales(rates.ptr, bb.num_drop_slots, batch, seed, counter, out.ptr, L.stream()), "gg_drop_path_scales")
    torch.cuda.synchronize()
    return out


TRAIN = [(name, prec, pol, rc) for name in ("tiny_vit_5m_224", "tiny_vit_21m_224") for prec in ("fp32", "fp32_split", "bf16") for pol in ("freeze", "all")
         for rc in (False, True)]
# ... and under every mask of tests/masks.py (fp32; the reduced family in bf16): `policy` is the mask's name.  Recompute is covered under the masks by
# tests/test_gpu_masks.py (recompute on is bit-identical to recompute off), so these run the keep-what-the-mask-needs plan, the one the mask shapes
TRAIN += [(name, "fp32", pol, False) for name in ("tiny_vit_5m_224", "tiny_vit_21m_224") for pol in MASKS.FAMILY_NAMES]
TRAIN += [(name, "bf16", pol, False) for name in ("tiny_vit_5m_224", "tiny_vit_21m_224") for pol in MASKS.REDUCED]


@pytest.mark.parametrize("name,precision,policy,recompute", TRAIN)
def test_tinyvit_training_step_is_independent_of_workspace_contents(name, precision, policy, recompute):
    from geoguessr_ai_amd import _lib as L
    batch, calls = (8 if name == "tiny_vit_5m_224" else 4), 4           # two panoramas / one panorama of four headings
    runs, scales = {}, {}
    for fill, zero in (("nan", False), ("finite", True)):
        m = _model(name, precision, policy)
        bb = m.backbone
        bb.set_grad_checkpointing(recompute)
        S = G.GuardSet(fill)
        ws, wc = _install(bb, S, batch, True, zero)
        x = torch.randn(batch, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        d_out = torch.randn(batch, bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
        drop = _drop_scales(bb, S, batch)
        cap0, rep0 = _stats()
        runs[fill] = [_step(bb, x, drop.view, d_out) for _ in range(calls)]
        cap1, rep1 = _stats()
        assert bb._ws[True].data_ptr() == ws.ptr and bb._wcache.data_ptr() == wc.ptr        # the step ran in the guarded buffers
        assert rep1 - rep0 >= 2, (cap1 - cap0, rep1 - rep0)                                  # the later calls replayed the captured forward and backward
        S.check()                                                                            # bands of workspace, cache and scales; rates and scales unchanged
        scales[fill] = drop.view.clone()
        L.lib().gg_graph_clear()                                                             # before the buffers the captured graphs refer to are released
        del m, S, ws, wc, drop
        gc.collect(); torch.cuda.empty_cache()
    G.assert_bit_identical(scales["nan"], scales["finite"], "drop_scales")
    for k, (a, b) in enumerate(zip(runs["nan"], runs["finite"])):
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all() and float(a[1].abs().sum()) > 0, k
        G.assert_bit_identical(a[0], b[0], f"step {k}: output")
        bad = _grad_mismatches(bb, a[1], b[1])
        assert not bad, f"step {k}: gradients depend on the workspace's prior contents in {bad[:6]} ({len(bad)} tensors)"
        G.assert_bit_identical(a[2], b[2], f"step {k}: running statistics")
        G.assert_bit_identical(a[3], b[3], f"step {k}: num_batches_tracked")


@pytest.mark.parametrize("name", ["tiny_vit_5m_224", "tiny_vit_21m_224"])
@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
def test_tinyvit_eval_forward_is_independent_of_workspace_contents(name, precision):
    from geoguessr_ai_amd import _lib as L
    batch, outs = 4, {}
    for fill, zero in (("nan", False), ("finite", True)):
        m = _model(name, precision, "all").eval()
        bb = m.backbone
        S = G.GuardSet(fill)
        ws, wc = _install(bb, S, batch, False, zero)
        x = torch.randn(batch, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        b0, c0 = bb._flat_buf.clone(), bb._counters.clone()
        res = []
        for _ in range(4):                                               # eager, captured, replayed twice
            out = bb.forward_hip(x, False)
            torch.cuda.synchronize()
            res.append(out.clone())
            del out
        assert bb._ws[False].data_ptr() == ws.ptr
        assert torch.equal(bb._flat_buf, b0) and torch.equal(bb._counters, c0)             # inference leaves the running statistics alone
        S.check()
        outs[fill] = res
        L.lib().gg_graph_clear()
        del m, bb, S, ws, wc
        gc.collect(); torch.cuda.empty_cache()
    for k, (a, b) in enumerate(zip(outs["nan"], outs["finite"])):
        assert torch.isfinite(a).all()
        G.assert_bit_identical(a, b, f"forward {k}")
        G.assert_bit_identical(a, outs["nan"][0], f"forward {k} vs the first")


# ------------------------------------------------------------------------------------------- CLIP vision tower
def _clip_install(tower, S, batch, training, zero):
    from geoguessr_ai_amd import _lib as L
    vm, lib = tower.vision_model, L.lib()
    mask = vm.trainable_mask() if training else None
    need = lib.gg_clip_workspace_bytes(C.byref(tower.cfg), batch, int(training), mask)
    assert need > 0
    ws = S.scratch("clip workspace", need, row_bytes=WS_ROW_BYTES, zero=zero)
    vm._ws[training] = ws.view[0]
    wc = S.scratch("clip wcache", lib.gg_clip_wcache_bytes(C.byref(tower.cfg)), row_bytes=WS_ROW_BYTES)
    vm._wcache, vm._wcache_version = wc.view[0], -1
    return ws, wc


@pytest.mark.parametrize("precision,mode", [("fp32", "eval"), ("bf16", "eval"), ("fp16", "eval"), ("fp32", "finetune_last"), ("bf16", "finetune_last"),
                                            ("fp32", "finetune_all"), ("bf16", "finetune_all")] +
                         [("fp32", "mask:" + key) for key in ("biases", "layernorms", "middle_layer", "position_embedding", "class_embedding", "patch_embedding",
                                                              "layernorm_weights", "random[0]", "random[1]", "random[2]")])
def test_clip_step_is_independent_of_workspace_contents(golden_dir, precision, mode):
    """gg_clip_forward / gg_clip_backward with the tiny tower of tests/test_gpu_clip.py: inference in the three storage types, and the fine-tune step
    (last encoder layer, as SuperGuessr trains it with a pretrained head; every layer) -- twice in the same workspace.  No atomics in this path: every
    gradient is compared bit for bit."""
    import os
    import numpy as np
    from tests import clip_golden as CG
    from tests.test_gpu_clip import _tiny_tower
    case = CG.load(golden_dir)
    x = torch.from_numpy(np.load(os.path.join(golden_dir, "clip_tiny.npz"))["x"]).cuda()
    batch, res = x.shape[0], {}
    for fill, zero in (("nan", False), ("finite", True)):
        tower = _tiny_tower(case, precision).cuda()
        vm = tower.vision_model
        training = mode != "eval"
        tower.train(training)
        if mode == "finetune_last":
            last = f"encoder.layers.{tower.cfg.num_layers - 1}."
            for n, p in vm._params.items():
                p.requires_grad = n.startswith(last)
        elif mode.startswith("mask:"):       # a CLIP mask of tests/masks.py by name (half pairs included: the LayerNorm dump row)
            MASKS.apply(vm, MASKS.clip_family([t["name"] for t in vm.table], tower.cfg.num_layers)[mode[5:]])
        S = G.GuardSet(fill)
        ws, wc = _clip_install(tower, S, batch, training, zero)
        steps = []
        for _ in range(2):
            if training:
                for p in vm._params.values():
                    p.grad = None
                if vm._flat_grad is not None:
                    vm._flat_grad.zero_()
                out = tower(pixel_values=x)
                (out.pooled_mean.square().sum() + out.last_hidden_state.sum()).backward()
                torch.cuda.synchronize()
                steps.append((out.pooled_mean.detach().clone(), out.last_hidden_state.detach().clone(), vm.flat_grads().clone()))
            else:
                with torch.no_grad():
                    o, lh = tower.forward_hip(x, False, True)
                torch.cuda.synchronize()
                steps.append((o.clone(), lh.clone()))
        assert vm._ws[training].data_ptr() == ws.ptr and vm._wcache.data_ptr() == wc.ptr
        S.check()
        res[fill] = steps
        del tower, vm, S, ws, wc
        gc.collect(); torch.cuda.empty_cache()
    for k, (a, b) in enumerate(zip(res["nan"], res["finite"])):
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.isfinite(u.float()).all(), (k, i)
            G.assert_bit_identical(u, v, f"step {k}: {('pooled', 'last_hidden', 'flat gradient')[i]}")
        if training:
            assert float(a[2].abs().sum()) > 0
