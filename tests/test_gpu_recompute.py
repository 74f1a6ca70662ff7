"""Activation recompute (TinyVitBackbone.set_grad_checkpointing, GgTinyVitCfg.recompute = 1) on the GPU: a training step with recompute is bit-identical
to the step without it -- output, every parameter gradient, the BatchNorm running statistics and num_batches_tracked -- in every mode, under both masks,
with DropPath on, eager and as a captured graph; the per-stage gradient callbacks keep their order and meaning; the running statistics are updated
once; and the reference's default model trains fully unfrozen at 512 images, which does not fit without recompute.

One exception to bit-identity, with or without recompute: the attention-bias tables' gradients.  The attention backward sums them per workgroup with
float atomics in LDS (attention.hip, attention_flash.hip), so their last bits depend on the order the waves arrive in -- two steps WITHOUT recompute
differ there as well (test_gpu_graph.py freezes them for the same reason).  They are compared to 1e-5 of their magnitude; every other gradient exactly."""
import ctypes as C
import gc
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_graph_cache():
    """Earlier tests' captured graphs were evicted unused (their addresses are gone): the cache would stop capturing -- start clean."""
    from geoguessr_ai_amd import _lib as L
    L.lib().gg_graph_clear()
    yield
    L.lib().gg_graph_clear()


def _grad_mismatches(bb, g0, g1, lo=0, hi=None):
    """Names of the parameter tensors within the flat range [lo, hi) whose gradients differ: bit for bit, except the attention-bias tables
    (LDS float atomics, see the module docstring): 1e-5 of their largest magnitude."""
    hi = g0.numel() if hi is None else hi
    bad = []
    for t in bb.table:
        if t["kind"] != 0 or t["offset"] < lo or t["offset"] >= hi:
            continue
        a, b = g0[t["offset"]:t["offset"] + t["numel"]], g1[t["offset"]:t["offset"] + t["numel"]]
        if t["name"].endswith("attention_biases"):
            if float((a - b).abs().max()) > 1e-5 * float(a.abs().max()) + 1e-30:
                bad.append(t["name"])
        elif not torch.equal(a, b):
            bad.append(t["name"])
    return bad


def _stats():
    from geoguessr_ai_amd import _lib as L
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    L.lib().gg_graph_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value


def _model(name, precision, policy, drop_path_rate=0.1, seed=0):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TinyViTAdapter(name, pretrained=False, precision=precision, drop_path_rate=drop_path_rate)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():        # away from timm's init (zero BatchNorm gamma of MBConv.conv3, zero biases): every gradient is non-trivial
        for n, p in m.backbone.named_parameters():
            if n.endswith(("bn.weight", "norm.weight")): p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith("attention_biases") or (n.endswith(".bias") and p.dim() == 1): p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith(".weight") and p.dim() == 2: p.copy_(0.05 * torch.randn(p.shape, generator=g))
    m = m.cuda().train()
    if policy == "freeze":
        m.freeze_all_but_last_stage()
    elif policy != "all":            # a mask of tests/masks.py by name
        from tests import masks
        masks.apply(m.backbone, policy)
    return m


def _step(bb, x, drop, d_out):
    for p in bb._params.values():
        p.grad = None
    if bb._flat_grad is not None:
        bb._flat_grad.zero_()
    out = bb.forward_hip(x, True, drop)
    bb.backward_hip(d_out)
    torch.cuda.synchronize()
    res = (out.clone(), bb._flat_grad.clone(), bb._flat_buf.clone(), bb._counters.clone())
    del out                      # same addresses on the next call: the graph path replays
    return res


def _run_both(bb, x, drop, d_out, calls):
    """`calls` steps without recompute, then the same steps from the same running statistics / counters with recompute."""
    b0, c0 = bb._flat_buf.clone(), bb._counters.clone()
    runs = {}
    for rc in (False, True):
        bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
        bb.set_grad_checkpointing(rc)
        cap0, rep0 = _stats()
        runs[rc] = [_step(bb, x, drop, d_out) for _ in range(calls)]
        cap1, rep1 = _stats()
        runs[rc, "graphs"] = (cap1 - cap0, rep1 - rep0)
    bb.set_grad_checkpointing(False)
    return runs


CASES = [("tiny_vit_5m_224", prec, pol, 8) for prec in ("fp32", "fp32_split", "bf16") for pol in ("freeze", "all")]
CASES += [("tiny_vit_5m_224", "fp32_split", "all", 256),        # the split-product routes (forward Linears, conv forwards, weight gradients)
          ("tiny_vit_21m_384", "fp32", "all", 2)]               # 24 x 24 windows: the flash backward's dS hand-off (scratch.attn_ds)


@pytest.mark.parametrize("name,precision,policy,batch", CASES)
def test_recompute_is_bit_identical(name, precision, policy, batch):
    m = _model(name, precision, policy)
    bb = m.backbone
    S = bb.cfg.img_size
    x = torch.randn(batch, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    drop = bb.make_drop_scales(batch, generator=torch.Generator().manual_seed(11))
    assert drop is not None
    d_out = torch.randn(batch, bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    calls = 3 if batch <= 8 else 1
    runs = _run_both(bb, x, drop, d_out, calls)
    if batch <= 8:
        for rc in (False, True):
            assert runs[rc, "graphs"][1] >= 2, (rc, runs[rc, "graphs"])      # the third call replays the captured forward and backward
    for k, (off, on) in enumerate(zip(runs[False], runs[True])):
        o0, g0, b0, c0 = off
        o1, g1, b1, c1 = on
        assert torch.isfinite(o0).all() and float(g0.abs().sum()) > 0
        assert torch.equal(o0, o1), (k, "output")
        bad = _grad_mismatches(bb, g0, g1)
        assert not bad, f"call {k}: gradients differ in {bad[:6]} ({len(bad)} tensors)"
        assert torch.equal(b0, b1), (k, "running statistics")
        assert torch.equal(c0, c1), (k, "num_batches_tracked")
    del m, bb
    gc.collect(); torch.cuda.empty_cache()


def test_stage_callbacks_keep_order_and_meaning():
    """With a gradient-ready hook (the eager backward with a host callback per stage: optim.AdamW.overlap_allreduce), the callbacks come in the order
    3, 2, 1, 0, -1 with recompute on, and when one fires the stage's gradient range already holds its final value (the recompute-off result)."""
    m = _model("tiny_vit_5m_224", "fp32", "all")
    bb = m.backbone
    x = torch.randn(8, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    drop = bb.make_drop_scales(8, generator=torch.Generator().manual_seed(11))
    d_out = torch.randn(8, bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    b0, c0 = bb._flat_buf.clone(), bb._counters.clone()
    _, ref, _, _ = _step(bb, x, drop, d_out)
    bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
    by_range = {v: k for k, v in bb._stage_ranges().items()}
    seen = []

    def hook(lo, hi):
        torch.cuda.synchronize()
        seen.append((by_range[(lo, hi)], _grad_mismatches(bb, ref, bb._flat_grad, lo, hi)))
    bb.set_grad_checkpointing(True)
    bb._grad_ready_hook = hook
    try:
        _, g1, _, _ = _step(bb, x, drop, d_out)
    finally:
        bb._grad_ready_hook = None
    assert [s for s, _ in seen] == [3, 2, 1, 0, -1]
    assert not any(bad for _, bad in seen), seen
    assert not _grad_mismatches(bb, ref, g1)


def test_setting_change_between_forward_and_backward_and_single_stat_update():
    from geoguessr_ai_amd import _lib as L
    m = _model("tiny_vit_5m_224", "fp32", "freeze")
    bb = m.backbone
    x = torch.randn(8, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    d_out = torch.randn(8, bb.num_features, device="cuda")
    b0, c0 = bb._flat_buf.clone(), bb._counters.clone()
    bb.forward_hip(x, True, None)
    bb.set_grad_checkpointing(True)
    with pytest.raises(L.GgError, match="set_grad_checkpointing"):
        bb.backward_hip(d_out)
    # one step without recompute, one from the same state with: the running statistics move once, by the same bits
    bb.set_grad_checkpointing(False)
    bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
    _, _, b_off, c_off = _step(bb, x, None, d_out)
    bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
    bb.set_grad_checkpointing(True)
    _, _, b_on, c_on = _step(bb, x, None, d_out)
    assert not torch.equal(b_off, b0)
    assert torch.equal(b_on, b_off) and torch.equal(c_on, c_off) and torch.equal(c_on, c0 + 1)


def test_c2_peak_memory_with_recompute():
    """The headline size (21M-224, 1024 images, fp32_split, the reference's freeze policy): the step's peak allocation with recompute is at most
    0.65 x the peak without, with the same embedding and gradients."""
    m = _model("tiny_vit_21m_224", "fp32_split", "freeze", drop_path_rate=0.2)
    bb = m.backbone
    B = 1024
    x = torch.randn(B, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    drop = bb.make_drop_scales(B, generator=torch.Generator().manual_seed(11))
    d_out = torch.randn(B, bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    names = ["stages.3.blocks.1.mlp.fc2.weight", "stages.3.blocks.0.attn.qkv.weight", "stages.3.downsample.conv1.conv.weight",
             "patch_embed.conv1.conv.weight", "patch_embed.conv2.bn.weight", "head.norm.weight"]
    peak, res = {}, {}
    for rc in (False, True):
        bb.set_grad_checkpointing(rc)
        bb._ws.clear()
        gc.collect(); torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        out, _, _, _ = _step(bb, x, drop, d_out)
        peak[rc] = torch.cuda.max_memory_allocated()
        res[rc] = (out, [bb._params[n].grad.clone() for n in names])
    assert peak[True] <= 0.65 * peak[False], (peak[True] / 2 ** 30, peak[False] / 2 ** 30)
    assert torch.equal(res[False][0], res[True][0])
    for n, a, b in zip(names, res[False][1], res[True][1]):
        assert float(a.abs().sum()) > 0 and torch.equal(a, b), n
    bb._ws.clear()
    del m, bb, x
    gc.collect(); torch.cuda.empty_cache()


def test_default_512_model_trains_fully_unfrozen_with_recompute():
    """tiny_vit_21m_512 (the reference's default, config.py:9), every tensor trainable (unfreeze_all), fp32, 512 images per GPU: the plan without
    recompute (359.5 GiB) does not fit the card; with recompute it does.  The size-independent property of test_gpu_fullsize512.py: 64 copies of 8
    images have the 8 images' batch statistics, so every copy's embedding and every gradient of a batch-mean loss equal the 8-image step's."""
    from geoguessr_ai_amd import _lib as L
    gc.collect(); torch.cuda.empty_cache()
    m = _model("tiny_vit_21m_512", "fp32", "all", drop_path_rate=0.0)
    m.unfreeze_all()
    bb = m.backbone
    B, REP = 512, 64
    mask = bb.trainable_mask()
    without = L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(bb.cfg), B, 1, mask)
    bb.set_grad_checkpointing(True)
    need = L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(bb.cfg), B, 1, mask)
    assert without > 288 * 2 ** 30 and need < 200 * 2 ** 30
    free, _ = torch.cuda.mem_get_info()
    if free < need + 12e9:
        pytest.skip(f"needs an idle MI355X: free {free / 2**30:.1f} GiB, torch reserved {torch.cuda.memory_reserved() / 2**30:.1f} / allocated "
                    f"{torch.cuda.memory_allocated() / 2**30:.1f} GiB, plan {need / 2**30:.1f} GiB")
    x8 = torch.randn(B // REP, 3, 512, 512, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    names = ["stages.3.blocks.1.mlp.fc2.weight", "stages.2.blocks.3.attn.qkv.weight", "stages.1.downsample.conv2.conv.weight",
             "stages.0.blocks.0.conv1.conv.weight", "patch_embed.conv1.conv.weight", "patch_embed.conv2.conv.weight"]

    def step(x):
        for p in bb._params.values():
            p.grad = None
        if bb._flat_grad is not None:
            bb._flat_grad.zero_()
        out = m(pixel_values=x).pooler_output
        out.square().mean().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), [bb._params[n].grad.clone() for n in names]
    o8, g8 = step(x8)
    assert torch.isfinite(o8).all() and all(torch.isfinite(t).all() and float(t.abs().sum()) > 0 for t in g8)
    bb._ws.clear()
    gc.collect(); torch.cuda.empty_cache()
    x = x8.repeat(REP, 1, 1, 1)
    o, gr = step(x)
    assert bb._ws[True].numel() == need
    del x
    o = o.view(REP, B // REP, -1)
    err = float((o - o8[None]).abs().max() / o8.abs().max())
    assert err < 1e-4, err
    for n, a, b in zip(names, g8, gr):
        rel = float((a - b).norm() / a.norm())
        assert rel < 1e-3, (n, rel)
    bb._ws.clear()
    del m, bb
    gc.collect(); torch.cuda.empty_cache()
