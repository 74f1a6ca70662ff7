"""Memory discipline of include/gg_clip_interp.h and of the CLIP tower at a foreign input size, in the way tests/test_gpu_guards_fp8.py holds its header: every
tensor of a call lives in a guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill, inputs stay unchanged, only -- and all
of -- the logical outputs are written, and the two runs agree bit for bit.  The tower runs a forward and a training step at 40 x 56 in a workspace of exactly
gg_clip_workspace_bytes and a weight cache of exactly gg_clip_wcache_bytes for that size (the resampled table is the cache's last region)."""
import ctypes as C
import gc
import os
import re

import numpy as np
import pytest
import torch

from tests import clip_interp_cases as IC
from tests import guards as G
from tests.test_gpu_guards import run_guarded

gpu = pytest.mark.gpu
F32 = torch.float32
CASES = {}
EXEMPT = {}                  # both prototypes take the caller's tensors: nothing is exempt
WS_ROW_BYTES = 4 * 3 * 128   # the longest row laid out in the tiny tower's workspace: f32 qkv


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def test_every_entry_point_is_guarded_or_exempt():
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_clip_interp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    assert len(guarded) == len(declared) == 2


GEOMS = [(4, 5, 7, 64), (4, 3, 3, 128), (2, 5, 3, 64), (7, 16, 16, 128), (24, 32, 32, 1024), (4, 4, 4, 64), (64, 1, 64, 4)]


@case("gg_clip_pos_interp_fwd")
@gpu
@pytest.mark.parametrize("Gs,Gh,Gw,D", GEOMS)
def test_forward(Gs, Gh, Gw, D):
    pos = torch.from_numpy(IC.table(Gs, D, seed=Gs + Gh + Gw))
    ref = IC.interp_ref(pos.numpy(), Gh, Gw)

    def call(S, L):
        pi = S.inp("pos", pos)
        o = S.out("out", Gh * Gw + 1, D, F32)
        L.check(L.lib().gg_clip_pos_interp_fwd(pi.ptr, Gs, Gh, Gw, D, o.ptr, L.stream()), "gg_clip_pos_interp_fwd")

        def check(val):
            assert float((val["out"].double() - torch.from_numpy(ref)).abs().max()) < 1e-4
        return {"out": o}, check
    run_guarded(call)


@case("gg_clip_pos_interp_bwd")
@gpu
@pytest.mark.parametrize("Gs,Gh,Gw,D", GEOMS)
def test_backward(Gs, Gh, Gw, D):
    g = torch.Generator().manual_seed(Gs * 7 + Gh)
    d_out, pre = torch.randn(Gh * Gw + 1, D, generator=g), torch.randn(Gs * Gs + 1, D, generator=g)
    ref = pre.double() + torch.from_numpy(IC.interp_ref_bwd(d_out.numpy(), Gs, Gh, Gw))

    def call(S, L):
        di = S.inp("d_out", d_out)
        o = S.out("d_pos", Gs * Gs + 1, D, F32, init=pre)      # accumulated: starts from known values
        L.check(L.lib().gg_clip_pos_interp_bwd(di.ptr, Gs, Gh, Gw, D, o.ptr, L.stream()), "gg_clip_pos_interp_bwd")

        def check(val):
            assert float((val["d_pos"].double() - ref).abs().max()) < 1e-4
        return {"d_pos": o}, check
    run_guarded(call)


def _install(tower, S, hw, batch, training, zero):
    from geoguessr_ai_amd import _lib as L
    vm, lib = tower.vision_model, L.lib()
    cfg = vm._cfg_at(hw)
    mask = vm.trainable_mask() if training else None
    need = lib.gg_clip_workspace_bytes(C.byref(cfg), batch, int(training), mask)
    assert need > lib.gg_clip_workspace_bytes(C.byref(tower.cfg), batch, int(training), mask) > 0
    ws = S.scratch("clip workspace", need, row_bytes=WS_ROW_BYTES, zero=zero)
    vm._ws[training] = ws.view[0]
    wbytes = lib.gg_clip_wcache_bytes(C.byref(cfg))
    assert wbytes > lib.gg_clip_wcache_bytes(C.byref(tower.cfg)) > 0
    wc = S.scratch("clip wcache", wbytes, row_bytes=WS_ROW_BYTES)
    vm._wcache, vm._wcache_version = wc.view[0], -1
    return ws, wc


@gpu
@pytest.mark.parametrize("precision,mode", [("fp32", "eval"), ("bf16", "eval"), ("fp16", "eval"), ("fp8", "eval"), ("fp32", "train"), ("fp32_split", "train"),
                                            ("bf16", "train"), ("bf16", "train_recompute")])
def test_step_at_40x56_is_independent_of_workspace_and_cache_contents(precision, mode):
    hw = (40, 56)
    x = IC.tiny_input(*hw).cuda()
    training = mode != "eval"
    res = {}
    for fill, zero in (("nan", False), ("finite", False)):
        tower = IC.tiny_tower(precision, interpolate_pos_encoding=True, gradient_checkpointing=mode == "train_recompute").cuda()
        vm = tower.vision_model
        if not training:
            for p in tower.parameters():
                p.requires_grad = False
            tower.eval()
        else:
            tower.train()
        S = G.GuardSet(fill)
        ws, wc = _install(tower, S, hw, x.shape[0], training, zero)
        if training:
            fg = S.scratch("flat gradient buffer", vm.param_floats * 4, row_bytes=4 * 256, zero=True)
            vm._flat_grad = fg.view[0].view(torch.float32)
        steps = []
        for _ in range(2):
            if training:
                tower.zero_grad(set_to_none=False)
                o = tower(pixel_values=x)
                (o.pooled_mean.square().sum() + o.last_hidden_state.square().mean()).backward()
                torch.cuda.synchronize()
                steps.append((o.pooled_mean.detach().clone(), o.last_hidden_state.detach().clone(), vm._flat_grad.clone()))
            else:
                with torch.no_grad():
                    o = tower(pixel_values=x)
                torch.cuda.synchronize()
                steps.append((o.pooled_mean.clone(), o.last_hidden_state.clone()))
        assert vm._ws[training].data_ptr() == ws.ptr and vm._wcache.data_ptr() == wc.ptr and (not training or vm._flat_grad.data_ptr() == fg.ptr)
        S.check()
        res[fill] = steps
        del tower, vm, S, ws, wc
        gc.collect(); torch.cuda.empty_cache()
    for k, (a, b) in enumerate(zip(res["nan"], res["finite"])):
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.isfinite(u.float()).all(), (k, i)
            G.assert_bit_identical(u, v, f"step {k}: {('pooled', 'last_hidden', 'flat gradient')[i]}")
    for u, v in zip(res["nan"][0], res["nan"][1]):
        assert torch.equal(u, v)
    assert res["nan"][0][1].shape == (2, 36, 128)
