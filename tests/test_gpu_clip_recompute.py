"""Activation recompute of the CLIP vision tower (CLIPVisionTower.gradient_checkpointing_enable, GgClipCfg.recompute = 1) on the GPU: a training step
with recompute is bit-identical to the step without -- pooled mean, last hidden state, every gradient, and the bytes of the flat gradient buffer no
trainable tensor owns -- under every mask of tests/masks.py, in fp32 and bf16, on the tiny golden tower and on the two real configurations (four layers of the large one also with
its lower layers frozen: several recomputes above in-place layers); several backwards of one forward give the recompute-off bits too; the
checkpointed plan is exactly as large as the step needs (guard bands, NaN-filled against zeroed); and the switch cannot come between a forward and its
backward.  The CLIP backward has no atomics: no comparison here has a tolerance except the one against the reference's own gradients."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from tests import clip_golden as CG
from tests import guards as G
from tests import masks as M
from tests.test_gpu_clip import _tiny_tower

pytestmark = pytest.mark.gpu

KEYS = ("biases", "layernorms", "middle_layer", "position_embedding", "class_embedding", "patch_embedding", "layernorm_weights",
        "random[0]", "random[1]", "random[2]", "all", "last_layer")
_TINY = {}


def _tiny(golden_dir, precision):
    """One tiny tower per precision for the whole module, its input and the two output gradients."""
    if precision not in _TINY:
        case = CG.load(golden_dir)
        tower = _tiny_tower(case, precision).cuda().train()
        x = torch.from_numpy(np.load(os.path.join(golden_dir, "clip_tiny.npz"))["x"]).cuda()
        _TINY[precision] = (tower, x) + _out_grads(tower, x.shape[0])
    return _TINY[precision]


def _out_grads(tower, batch):
    g = torch.Generator().manual_seed(9)
    d_out = torch.randn(batch, tower.cfg.hidden_size, generator=g).cuda()
    d_last = (torch.randn(batch, tower.num_tokens, tower.cfg.hidden_size, generator=g) * 0.1).cuda()
    return d_out, d_last


def _masks(tower):
    names = [t["name"] for t in tower.vision_model.table]
    nl = tower.cfg.num_layers
    fam = dict(M.clip_family(names, nl), all=frozenset(names), last_layer=frozenset(n for n in names if n.startswith(f"encoder.layers.{nl - 1}.")))
    assert set(fam) == set(KEYS)
    return fam


def _step(tower, x, d_out, d_last):
    """One forward + backward from a zeroed flat gradient buffer: (pooled mean, last hidden state, flat gradient buffer), cloned."""
    vm = tower.vision_model
    for p in vm._params.values():
        p.grad = None
    fg = vm.attach_grads()
    fg.zero_()
    out, last = tower.forward_hip(x, True, True)
    tower.backward_hip(d_out, d_last, vm._gen)
    torch.cuda.synchronize()
    return out.clone(), last.clone(), fg.clone()


def _off_and_on(tower, x, d_out, d_last):
    tower.gradient_checkpointing_disable()
    off = _step(tower, x, d_out, d_last)
    tower.gradient_checkpointing_enable()
    assert tower.vision_model._ws.get(True) is None            # the other plan's workspace is gone
    on = _step(tower, x, d_out, d_last)
    tower.gradient_checkpointing_disable()
    return off, on


def _assert_same_step(tower, mask, off, on, what):
    vm = tower.vision_model
    for u in off + on:
        assert torch.isfinite(u).all(), what
    G.assert_bit_identical(off[0], on[0], f"{what}: pooled_mean")
    G.assert_bit_identical(off[1], on[1], f"{what}: last_hidden_state")
    frozen = torch.ones(vm.param_floats, dtype=torch.bool, device="cuda")
    moved = 0
    for t in vm.table:
        lo, hi = t["offset"], t["offset"] + t["numel"]
        if t["name"] in mask:
            frozen[lo:hi] = False
            G.assert_bit_identical(off[2][lo:hi], on[2][lo:hi], f"{what}: gradient of {t['name']}")
            moved += int(bool(off[2][lo:hi].abs().sum() > 0))
    assert moved > 0, (what, "no gradient at all")
    for name, fg in (("off", off[2]), ("on", on[2])):
        assert bool((fg.view(torch.int32)[frozen] == 0).all()), (what, name, "frozen gradient ranges / padding written")
    G.assert_bit_identical(off[2], on[2], f"{what}: flat gradient buffer")


@pytest.mark.parametrize("both", [False, True], ids=["d_out", "d_out+d_last_hidden"])
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_recompute_is_bit_identical_on_the_tiny_tower(golden_dir, precision, key, both):
    tower, x, d_out, d_last = _tiny(golden_dir, precision)
    mask = M.apply(tower.vision_model, _masks(tower)[key])
    off, on = _off_and_on(tower, x, d_out, d_last if both else None)
    _assert_same_step(tower, mask, off, on, f"tiny {precision} {key}")


@pytest.mark.parametrize("policy", ["all_layers", "last_layer"])
def test_recompute_gradients_match_the_reference_golden(golden_dir, policy):
    """SuperGuessr on the tiny CLIP base, fp32, `model.base_model.gradient_checkpointing_enable()`: the tower gradients against the reference's own run
    (tests/clip_golden.py, clip_train.npz) at the 1e-4 of test_superguessr_on_clip_training_matches_reference_golden."""
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    case = CG.load(golden_dir)
    g = case["g"]
    tower = _tiny_tower(case, "fp32")
    model = SuperGuessr(base_model=tower, panorama=True, should_smooth_labels=True)
    model.base_model.gradient_checkpointing_enable()
    assert tower.is_gradient_checkpointing and tower.cfg.recompute == 1
    if policy == "last_layer":
        for layer in list(tower.vision_model.encoder.layers)[:-1]:
            for p in layer.parameters():
                p.requires_grad = False
    with torch.no_grad():
        model.cell_layer.weight.copy_(case["W"]); model.cell_layer.bias.copy_(case["b"])
    model = model.cuda().train()
    out = model(pixel_values=case["x"].cuda(), labels=case["labels"].cuda(), labels_clf=torch.from_numpy(g["labels_clf"]).cuda())
    out.loss.backward()
    torch.cuda.synchronize()
    vm = tower.vision_model
    frozen = [n for n, p in vm._params.items() if not p.requires_grad]
    assert bool(frozen) == (policy == "last_layer") and all(vm._params[n].grad is None for n in frozen)
    case_live = dict(case, names=[n for n in case["names"] if n not in frozen])
    errs = CG.grad_errors(case_live, {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in vm._params.items() if n not in frozen})
    worst = max(errs, key=errs.get)
    loss_rel = abs(float(out.loss.detach()) - float(g["loss"])) / float(g["loss"])
    print(f"\n[SuperGuessr on CLIP tiny, fp32, recompute, {policy}] loss rel {loss_rel:.2e}, {len(errs)} tower gradients: worst {worst} {errs[worst]:.2e}")
    assert loss_rel < 1e-5
    assert errs[worst] < 1e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


@pytest.mark.parametrize("mode", ["all", "last_layer", "middle_layer", "layernorm_weights"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_checkpointed_step_in_a_guarded_workspace(golden_dir, precision, mode):
    """The step with recompute in a workspace of exactly gg_clip_workspace_bytes(recompute = 1) between guard bands, twice in a row: NaN-filled and zeroed
    workspaces give the same bits (no launch reads a byte the step has not written, the shared segment region included), the bands stay untouched."""
    from tests.test_gpu_guards_model import _clip_install
    from geoguessr_ai_amd import _lib as L
    case = CG.load(golden_dir)
    x = torch.from_numpy(np.load(os.path.join(golden_dir, "clip_tiny.npz"))["x"]).cuda()
    batch, res = x.shape[0], {}
    for fill, zero in (("nan", False), ("finite", True)):
        tower = _tiny_tower(case, precision).cuda().train()
        tower.gradient_checkpointing_enable()
        vm = tower.vision_model
        mask = M.apply(vm, _masks(tower)[mode])
        d_out, d_last = _out_grads(tower, batch)
        S = G.GuardSet(fill)
        ws, wc = _clip_install(tower, S, batch, True, zero)
        need = L.lib().gg_clip_workspace_bytes(C.byref(tower.cfg), batch, 1, vm.trainable_mask())
        assert vm._ws[True].numel() == need
        cfg0 = L.ClipCfg.from_buffer_copy(tower.cfg)
        cfg0.recompute = 0
        assert need <= L.lib().gg_clip_workspace_bytes(C.byref(cfg0), batch, 1, vm.trainable_mask())
        steps = [_step(tower, x, d_out, d_last) for _ in range(2)]
        assert vm._ws[True].data_ptr() == ws.ptr and vm._wcache.data_ptr() == wc.ptr
        S.check()
        res[fill] = steps
        del tower, vm, S, ws, wc
        gc.collect(); torch.cuda.empty_cache()
    for k, (a, b) in enumerate(zip(res["nan"], res["finite"])):
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.isfinite(u).all(), (k, i)
            G.assert_bit_identical(u, v, f"step {k}: {('pooled', 'last_hidden', 'flat gradient')[i]}")
        assert float(a[2].abs().sum()) > 0
    for u, v in zip(res["nan"][0], res["nan"][1]):
        G.assert_bit_identical(u, v, "second step in the same workspace")
    assert mask


# (four layers of L/14-336 at 2 images: the smallest tower whose recompute-off plan is large enough to hold the dS hand-off while the checkpointed plan, left to
#  decide from its own size, would drop it -- per image 22 MB of dS against 1/8 of 58 MB + 38 MB per layer without, 67 MB + 38 MB in all with recompute)
L14 = "openai/clip-vit-large-patch14-336"
# (from_layer_1 / from_layer_2: layers below run frozen and in place, the kept ones above are re-formed one after the other -- l0 > 0 with several recomputes,
#  which the two-layer golden tower cannot show)
REAL = [("openai/clip-vit-base-patch32", {}, 8, "all"), (L14, dict(num_layers=2), 2, "all"), (L14, dict(num_layers=4), 2, "all"),
        (L14, dict(num_layers=4), 2, "from_layer_1"), (L14, dict(num_layers=4), 2, "from_layer_2")]


def _real_mask(tower, key):
    names = [t["name"] for t in tower.vision_model.table]
    if key == "all":
        return frozenset(names)
    l0 = int(key[len("from_layer_"):])
    return frozenset(n for n in names if n.startswith("encoder.layers.") and int(n.split(".")[2]) >= l0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("model,overrides,batch,key", REAL, ids=["B32x8", "L14-336-2layers-x2", "L14-336-4layers-x2", "L14-336-4layers-x2-from_layer_1",
                                                                  "L14-336-4layers-x2-from_layer_2"])
def test_recompute_is_bit_identical_at_real_shapes(model, overrides, batch, key, precision):
    """ViT-B/32 (50 tokens: the single-pass attention backward) and two layers of ViT-L/14-336 (577 tokens: the two-pass attention backward, whose dS
    hand-off exists or not by the recompute-off plan's decision in both settings), every tensor trainable; four layers of it also with the first one / two
    layers frozen."""
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    tower = CLIPVisionTower(model, precision=precision, seed=3, **overrides).cuda().train()
    T = tower.num_tokens
    assert bool(L.lib().gg_attention_flash_single_pass(T, 64, 0, 0)) == (T <= 256) and (T == 577 or T == 50)
    S = tower.cfg.image_size
    x = torch.randn(batch, 3, S, S, generator=torch.Generator().manual_seed(4)).cuda()
    d_out, d_last = _out_grads(tower, batch)
    mask = M.apply(tower.vision_model, _real_mask(tower, key))
    if key != "all":
        cfg1 = L.ClipCfg.from_buffer_copy(tower.cfg)
        cfg1.recompute = 1
        assert L.lib().gg_clip_first_trained_layer(C.byref(cfg1), tower.vision_model.trainable_mask()) == int(key[-1]) < tower.cfg.num_layers - 1
    off, on = _off_and_on(tower, x, d_out, d_last)
    _assert_same_step(tower, mask, off, on, f"{model} {precision} {key}")
    del tower, off, on
    gc.collect(); torch.cuda.empty_cache()


def _backwards_of_one_forward(tower, x, d_out, d_last):
    """ONE training forward, then three backwards of it: d_out alone, d_last_hidden on top (accumulated: the two-call form of giving both), and d_out alone
    again from a zeroed buffer.  The flat gradient buffer after each."""
    vm = tower.vision_model
    for p in vm._params.values():
        p.grad = None
    fg = vm.attach_grads()
    fg.zero_()
    tower.forward_hip(x, True, True)
    res = []
    for do, dl, zero in ((d_out, None, False), (None, d_last, False), (d_out, None, True)):
        if zero:
            fg.zero_()
        tower.backward_hip(do, dl, vm._gen)
        torch.cuda.synchronize()
        res.append(fg.clone())
    return res


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("which", ["tiny-all", "L14-336-4layers-x2-from_layer_1"])
def test_repeated_backwards_of_one_forward(golden_dir, which, precision):
    """The first backward re-forms the lower layers in the segment region, over the top layer's tensors the forward left there: a further backward of the same
    forward re-forms the top layer too.  Bit for bit the recompute-off results, and the third backward repeats the first."""
    if which == "tiny-all":
        tower, x, d_out, d_last = _tiny(golden_dir, precision)
        mask = M.apply(tower.vision_model, _masks(tower)["all"])
    else:
        from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
        tower = CLIPVisionTower(L14, precision=precision, seed=3, num_layers=4).cuda().train()
        S = tower.cfg.image_size
        x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(4)).cuda()
        d_out, d_last = _out_grads(tower, 2)
        mask = M.apply(tower.vision_model, _real_mask(tower, "from_layer_1"))
    assert mask
    tower.gradient_checkpointing_disable()
    off = _backwards_of_one_forward(tower, x, d_out, d_last)
    tower.gradient_checkpointing_enable()
    on = _backwards_of_one_forward(tower, x, d_out, d_last)
    tower.gradient_checkpointing_disable()
    for k, (u, v) in enumerate(zip(off, on)):
        assert torch.isfinite(u).all() and float(u.abs().sum()) > 0
        G.assert_bit_identical(u, v, f"{which} {precision}: flat gradient after backward {k} of one forward")
    assert not torch.equal(on[0], on[1])
    G.assert_bit_identical(on[0], on[2], f"{which} {precision}: the third backward repeats the first")
    if which != "tiny-all":
        del tower
        gc.collect(); torch.cuda.empty_cache()


def test_retain_graph_backward_twice_with_recompute(golden_dir):
    """autograd's form of the same: `backward(retain_graph=True)` then `backward()` of one loss, the second accumulating onto the first -- the bits of the same
    two calls without recompute."""
    tower, x, d_out, d_last = _tiny(golden_dir, "fp32")
    vm = tower.vision_model
    M.apply(vm, _masks(tower)["all"])
    res = {}
    for rc in (False, True):
        tower.gradient_checkpointing_enable() if rc else tower.gradient_checkpointing_disable()
        for p in vm._params.values():
            p.grad = None
        vm.attach_grads().zero_()
        out = tower(pixel_values=x)
        loss = (out.pooled_mean * d_out).sum() + (out.last_hidden_state * d_last).sum()
        loss.backward(retain_graph=True)
        torch.cuda.synchronize()
        once = vm.flat_grads().clone()
        loss.backward()
        torch.cuda.synchronize()
        res[rc] = (once, vm.flat_grads().clone())
    tower.gradient_checkpointing_disable()
    assert float(res[True][0].abs().sum()) > 0 and not torch.equal(res[True][0], res[True][1])
    G.assert_bit_identical(res[False][0], res[True][0], "first backward")
    G.assert_bit_identical(res[False][1], res[True][1], "second backward of the same forward")


def test_a_toggle_between_forward_and_backward_is_refused(golden_dir):
    from geoguessr_ai_amd import _lib as L
    tower, x, d_out, d_last = _tiny(golden_dir, "fp32")
    vm = tower.vision_model
    mask = M.apply(vm, _masks(tower)["all"])
    tower.gradient_checkpointing_disable()
    ref = _step(tower, x, d_out, None)
    # the Python layer: the workspace is released with the toggle, the pending backward is refused
    tower.forward_hip(x, True, False)
    tower.gradient_checkpointing_enable()
    assert vm._last is None and vm._ws.get(True) is None
    with pytest.raises(L.GgError, match="toggled since the training forward.*now recompute=1.*run the forward again"):
        tower.backward_hip(d_out, None, vm._gen)
    # through autograd too, and switching back does not revive the old forward
    for p in vm._params.values():
        p.grad = None
    out = tower(pixel_values=x)
    tower.gradient_checkpointing_disable()
    tower.gradient_checkpointing_enable()
    with pytest.raises(L.GgError, match="toggled since the training forward.*run the forward again"):
        out.pooled_mean.sum().backward()
    # a toggle followed by a fresh forward works, with the same bits
    on = _step(tower, x, d_out, None)
    _assert_same_step(tower, mask, ref, on, "after the toggle")
    # the library: the same workspace, the other cfg->recompute (the checkpointed plan is the smaller one: nothing could leave the allocation)
    tower.gradient_checkpointing_disable()
    tower.forward_hip(x, True, False)
    ws = vm._ws[True]
    cfg1 = L.ClipCfg.from_buffer_copy(tower.cfg)
    cfg1.recompute = 1
    assert L.lib().gg_clip_workspace_bytes(C.byref(cfg1), x.shape[0], 1, None) <= ws.numel()
    fg = vm.attach_grads()
    before = fg.clone()
    rc = L.lib().gg_clip_backward(C.byref(cfg1), x.shape[0], L.ptr(vm._flat), L.ptr(vm._wcache), L.ptr(ws), L.ptr(d_out), None, L.ptr(fg), None, L.stream())
    msg = L.lib().gg_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "recompute" in msg and "run the forward again" in msg, (rc, msg)
    G.assert_bit_identical(before, fg, "a refused backward writes no gradient")
    tower.backward_hip(d_out, None, vm._gen)                 # the matching setting is still accepted
    torch.cuda.synchronize()
