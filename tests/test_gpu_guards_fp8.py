"""Memory discipline of include/gg_fp8.h and of the CLIP tower's fp8 eval forward, in the way tests/test_gpu_guards_pad.py holds its header: every tensor of a call
lives in a guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill, inputs stay unchanged, only -- and all of -- the logical
outputs are written, and the two runs agree bit for bit.  (Under the NaN fill the padding of a code matrix holds 0xFF bytes: e4m3 NaN codes.)"""
import ctypes as C
import gc
import os
import re

import pytest
import torch

from tests import clip_fp8_ref as R
from tests import guards as G
from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
F16, F32, U8 = torch.float16, torch.float32, torch.uint8
CASES = {}
EXEMPT = {}                  # all three prototypes take the caller's tensors: nothing is exempt


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def test_every_fp8_entry_point_is_guarded_or_exempt():
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_fp8.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    assert len(guarded) == len(declared) == 3


def _no_nan_codes(q):
    assert not bool(((q & 0x7F) == 0x7F).any()), "a code was never written (0xFF pre-fill) or is a NaN code"


@case("gg_quant_rows_e4m3")
@gpu
@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("M,K,pad", [(5, 128, 8), (67, 512, 24), (3, 4096, 0), (2, 8192, 16)])
def test_quant_rows(dtype, M, K, pad):
    x = rnd(M, K, seed=K + M, dtype=dtype)
    x[M - 1] = 0.0
    want_q, want_s = R.quant_rows(x)

    def call(S, L):
        xi = S.inp("x", x.to(dtype), ld=K + pad)
        q = S.out("q", M, K, U8, ld=K + 2 * pad)
        s = S.out("scale", 1, M, F32)
        L.check(L.lib().gg_quant_rows_e4m3(xi.ptr, int(dtype == F32), K + pad, M, K, q.ptr, K + 2 * pad, s.ptr, L.stream()), "gg_quant_rows_e4m3")

        def check(val):
            assert torch.equal(val["q"], want_q) and torch.equal(val["scale"][0], want_s)
        return {"q": q, "scale": s}, check
    run_guarded(call)


@case("gg_layernorm_fwd_e4m3")
@gpu
@pytest.mark.parametrize("M,Cc,pad", [(1, 128, 0), (67, 768, 8), (6, 1024, 40)])
def test_layernorm(M, Cc, pad):
    x, gamma, beta = rnd(M, Cc, seed=Cc, dtype=F16), 1 + 0.1 * rnd(Cc, seed=1), 0.1 * rnd(Cc, seed=2)

    def call(S, L):
        xi, gi, bi = S.inp("x", x.to(F16)), S.inp("gamma", gamma), S.inp("beta", beta)
        q = S.out("q", M, Cc, U8, ld=Cc + pad)
        s = S.out("scale", 1, M, F32)
        L.check(L.lib().gg_layernorm_fwd_e4m3(xi.ptr, gi.ptr, bi.ptr, M, Cc, L.f32(1e-5), q.ptr, Cc + pad, s.ptr, L.stream()), "gg_layernorm_fwd_e4m3")

        def check(val):
            _no_nan_codes(val["q"])
            y = torch.nn.functional.layer_norm(x.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
            assert R.rel_l2(R.decode(val["q"]) * val["scale"][0].double()[:, None], y) < 0.05
        return {"q": q, "scale": s}, check
    run_guarded(call)


@case("gg_gemm_nt_e4m3")
@gpu
@pytest.mark.parametrize("epi", ["bias", "quick_gelu", "residual", "alias"])
@pytest.mark.parametrize("M,N,K,pad", [(1, 64, 128, 16), (200, 192, 512, 0), (577, 384, 1024, 32), (260, 512, 4096, 16)])
def test_gemm(M, N, K, pad, epi):
    ca, sa = R.quant_rows(rnd(M, K, seed=M))
    cw, sw = R.quant_rows(rnd(N, K, seed=N, scale=K ** -0.5))
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4, dtype=F16)
    ref = R.dequant(ca, sa) @ R.dequant(cw, sw).T + bias.double()
    ref = ref * torch.sigmoid(1.702 * ref) if epi == "quick_gelu" else (ref + res.double() if epi in ("residual", "alias") else ref)

    def call(S, L):
        Ai, Wi = S.inp("A", ca, ld=K + pad), S.inp("W", cw, ld=K + 2 * pad)
        sai, swi, bi = S.inp("sa", sa), S.inp("sw", sw), S.inp("bias", bias)
        a = L.GemmArgs()
        a.A, a.lda, a.B, a.ldb, a.M, a.N, a.K, a.bias, a.split_k = Ai.ptr, K + pad, Wi.ptr, K + 2 * pad, M, N, K, bi.ptr, 1
        if epi == "alias":
            c = S.out("C", M, N, F16, ld=N + 8, init=res.to(F16))
            a.residual, a.ldr = c.ptr, N + 8
        else:
            c = S.out("C", M, N, F16, ld=N + 8)
            if epi == "residual":
                ri = S.inp("residual", res.to(F16), ld=N + 16)
                a.residual, a.ldr = ri.ptr, N + 16
        a.C, a.ldc, a.act = c.ptr, N + 8, 2 if epi == "quick_gelu" else 0
        L.check(L.lib().gg_gemm_nt_e4m3(C.byref(a), sai.ptr, swi.ptr, L.stream()), "gg_gemm_nt_e4m3")

        def check(val):
            assert R.rel_l2(val["C"], ref) < 2e-3
        return {"C": c}, check
    run_guarded(call)


@gpu
def test_clip_fp8_eval_forward_is_independent_of_workspace_contents(golden_dir):
    """The case tests/test_gpu_guards_model.py::test_clip_step_is_independent_of_workspace_contents runs for ("fp16", "eval"), in the fp8 mode: workspace of exactly
    gg_clip_workspace_bytes and weight cache of exactly gg_clip_wcache_bytes in guarded buffers (the cache starts as the fill), two forwards in one workspace."""
    import numpy as np
    from tests import clip_golden as CG
    from tests.test_gpu_clip import _tiny_tower
    from tests.test_gpu_guards_model import _clip_install
    case_ = CG.load(golden_dir)
    x = torch.from_numpy(np.load(os.path.join(golden_dir, "clip_tiny.npz"))["x"]).cuda()
    res = {}
    for fill, zero in (("nan", False), ("finite", True)):
        tower = _tiny_tower(case_, "fp8").cuda().eval()
        vm = tower.vision_model
        S = G.GuardSet(fill)
        ws, wc = _clip_install(tower, S, x.shape[0], False, zero)
        steps = []
        for _ in range(2):
            with torch.no_grad():
                o, lh = tower.forward_hip(x, False, True)
            torch.cuda.synchronize()
            steps.append((o.clone(), lh.clone()))
        assert vm._ws[False].data_ptr() == ws.ptr and vm._wcache.data_ptr() == wc.ptr
        S.check()
        res[fill] = steps
        del tower, vm, S, ws, wc
        gc.collect(); torch.cuda.empty_cache()
    for k, (a, b) in enumerate(zip(res["nan"], res["finite"])):
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.isfinite(u.float()).all(), (k, i)
            G.assert_bit_identical(u, v, f"step {k}: {('pooled', 'last_hidden')[i]}")
    assert torch.equal(res["nan"][0][1], res["nan"][1][1])
