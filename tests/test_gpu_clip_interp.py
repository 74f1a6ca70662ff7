"""CLIP vision tower at any input size on the GPU: the resampling kernels (include/gg_clip_interp.h) against the fp64 separable form of
tests/clip_interp_cases.py, and the tower with ``interpolate_pos_encoding`` -- unchanged at the native size, bit for bit a native tower on the resampled table at a
foreign one, and held to the oracle / to transformers' own run (tests/golden/clip_interp_tiny.npz) at the gates tests/test_gpu_clip.py, test_gpu_clip_split.py and
test_gpu_clip_fp8.py use for the same quantities at the native size.

The kernel gate is computed per case: twice the largest error of torch's own f32 ``F.interpolate`` against the same fp64 reference on the same table -- torch
sums 16 taps in f32 over f32 weights, the kernels in f64 over f64 weights and round once.  The backward into zeros is held to the SAME figure against the transposed fp64
form (at the identity geometry both gates are exactly 0), and the add into a pre-filled ``d_pos`` is shown exactly: the kernel stores ``d_pos + (its result into zeros)``."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from tests import clip_interp_cases as IC

pytestmark = pytest.mark.gpu

TRAIN_MODES = ["fp32", "fp32_split", "bf16"]
EVAL_MODES = ["fp16", "fp8"]


def _rel(a, b):
    a, b = torch.as_tensor(a).flatten().double().cpu(), torch.as_tensor(b).flatten().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _freeze(tower):
    for p in tower.parameters():
        p.requires_grad = False
    return tower


def _loss(out):
    return out.pooled_mean.square().sum() + out.last_hidden_state.square().mean()


def _grads(tower):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in tower.vision_model._params.items()}


# ------------------------------------------------------------------------------------------- the kernels
_KERNEL_CASES = [(g, D) for g in IC.GEOMETRIES for D in ((1024,) if g == (24, 32, 32) else (64, 128))]


@pytest.mark.parametrize("geom,D", _KERNEL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernels_against_the_fp64_separable_form(geom, D):
    from geoguessr_ai_amd import ops
    Gs, Gh, Gw = geom
    pos = IC.table(Gs, D, seed=1000 * Gs + 10 * Gh + Gw)
    ref = IC.interp_ref(pos, Gh, Gw)
    torch_f32 = IC.torch_interp(torch.from_numpy(pos), Gh, Gw).numpy()
    gate = 2.0 * float(np.abs(torch_f32.astype(np.float64) - ref).max())
    x = torch.from_numpy(pos).cuda()
    got = ops.clip_pos_interp(x, (Gh, Gw))
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"\n[{geom}, D {D}] forward: max abs error {err:.3e}, gate (2 x torch f32's own) {gate:.3e}")
    assert got.shape == (Gh * Gw + 1, D) and torch.isfinite(got).all()
    assert err <= gate
    assert torch.equal(got[0], x[0])                                             # the class row passes straight through
    assert torch.equal(ops.clip_pos_interp(x, (Gh, Gw)), got)                    # two runs: the same bits
    if Gs == Gh == Gw:
        assert torch.equal(got, x)                                               # the native grid returns the input bits
    # the adjoint into zeros against the transposed fp64 form, under the same gate
    rng = np.random.default_rng(7 + D)
    y = rng.standard_normal((Gh * Gw + 1, D), dtype=np.float32)
    pre = rng.standard_normal((Gs * Gs + 1, D), dtype=np.float32)
    yd = torch.from_numpy(y).cuda()
    zero_t = ops.clip_pos_interp_bwd(yd, Gs * Gs + 1, (Gh, Gw))
    zero_b = zero_t.cpu().numpy().astype(np.float64)
    err_b = float(np.abs(zero_b - IC.interp_ref_bwd(y, Gs, Gh, Gw)).max())
    print(f"[{geom}, D {D}] backward into zeros: max abs error {err_b:.3e}, gate {gate:.3e}")
    assert err_b <= gate
    # ... and into a pre-filled d_pos: the kernel ADDS, exactly d_pos + (the result into zeros)
    got_b = ops.clip_pos_interp_bwd(yd, Gs * Gs + 1, (Gh, Gw), accumulate_into=torch.from_numpy(pre).cuda())
    assert torch.equal(got_b, torch.from_numpy(pre).cuda() + zero_t)
    assert torch.equal(zero_t[0], yd[0])                                         # row 0 passes straight through
    assert torch.equal(ops.clip_pos_interp_bwd(yd, Gs * Gs + 1, (Gh, Gw)), zero_t)      # two runs: the same bits
    # <fwd(x), y> == <x, bwd(y)>: each side carries at most `gate` per element
    a = float((got.cpu().numpy().astype(np.float64) * y.astype(np.float64)).sum())
    b = float((pos.astype(np.float64) * zero_b).sum())
    bound = gate * (float(np.abs(y).sum()) + float(np.abs(pos).sum()))
    print(f"[{geom}, D {D}] <fwd(x), y> - <x, bwd(y)> = {a - b:.3e}, bound {bound:.3e}")
    assert abs(a - b) <= bound


def test_kernels_refuse_on_the_device_path_too():
    from geoguessr_ai_amd import _lib as L, ops
    x = torch.zeros(17, 64, device="cuda")
    with pytest.raises(L.GgError, match="above the cap of 64"):
        ops.clip_pos_interp(x, (65, 4))
    with pytest.raises(L.GgError, match="below 1"):
        ops.clip_pos_interp(x, (0, 4))
    with pytest.raises(L.GgError, match="multiple of 4"):
        ops.clip_pos_interp(torch.zeros(17, 66, device="cuda"), (5, 7))
    with pytest.raises(L.GgError, match="Gs \\* Gs \\+ 1 rows"):
        ops.clip_pos_interp(torch.zeros(16, 64, device="cuda"), (5, 7))


# ------------------------------------------------------------------------------------------- the native size: nothing changes
def _launches(fn):
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    lib.gg_prof_reset(); lib.gg_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        cat, cats = C.c_int(), []
        for i in range(lib.gg_prof_count()):
            L.check(lib.gg_prof_record(i, C.byref(cat), None, None, None), "gg_prof_record")
            cats.append(cat.value)
    finally:
        lib.gg_prof_enable(0); lib.gg_prof_reset()
    return out, cats


@pytest.mark.parametrize("precision", TRAIN_MODES + EVAL_MODES)
def test_native_size_is_unchanged_by_the_flag(precision):
    x = IC.tiny_input(32, 32).cuda()
    res = {}
    for flag in (False, True):
        tower = IC.tiny_tower(precision).cuda()
        if precision in EVAL_MODES:
            _freeze(tower).eval()

            def step():
                with torch.no_grad():
                    o = tower(pixel_values=x, interpolate_pos_encoding=flag)
                return o.pooled_mean, o.last_hidden_state, {}
        else:
            tower.train()

            def step():
                o = tower(pixel_values=x, interpolate_pos_encoding=flag)
                _loss(o).backward()
                return o.pooled_mean.detach(), o.last_hidden_state.detach(), _grads(tower)
        res[flag] = _launches(step)
    (p0, l0, g0), c0 = res[False]
    (p1, l1, g1), c1 = res[True]
    assert torch.equal(p0, p1) and torch.equal(l0, l1) and l0.shape == (2, 17, 128)
    assert g0.keys() == g1.keys() and all(torch.equal(g0[n], g1[n]) for n in g0 if g0[n] is not None)
    assert c0 == c1 and len(c0) > 0, (len(c0), len(c1))                         # the same launch list


def test_foreign_size_is_refused_without_the_flag_as_before():
    from geoguessr_ai_amd import _lib as L
    tower = _freeze(IC.tiny_tower("fp32").cuda().eval())
    with pytest.raises(L.GgError, match=r"CLIPVisionTower expects \(B,3,32,32\) pixel_values, got \(2, 3, 40, 56\)"):
        tower(pixel_values=IC.tiny_input(40, 56).cuda())
    with pytest.raises(L.GgError, match="not a multiple of the patch size 8"):
        tower(pixel_values=torch.zeros(1, 3, 40, 52).cuda(), interpolate_pos_encoding=True)
    out = tower(pixel_values=IC.tiny_input(40, 56).cuda(), interpolate_pos_encoding=True)
    assert out.last_hidden_state.shape == (2, 36, 128) and out.pooled_mean.shape == (2, 128)


# ------------------------------------------------------------------------------------------- equivalence, bit for bit
def _pair(precision, size, **kw):
    """Tower A (image_size 32, the flag on) and tower B built natively at ``size`` with its table = ops.clip_pos_interp of A's."""
    from geoguessr_ai_amd import ops
    A = IC.tiny_tower(precision, interpolate_pos_encoding=True, **kw).cuda()
    B = IC.tiny_tower(precision, image_size=size, **kw).cuda()
    g = size // IC.TINY[5]
    with torch.no_grad():
        B.vision_model._params["embeddings.position_embedding.weight"].copy_(ops.clip_pos_interp(A.vision_model._params["embeddings.position_embedding.weight"].data, (g, g)))
    B.vision_model.mark_params_dirty()
    for n, p in A.vision_model._params.items():
        if n != "embeddings.position_embedding.weight":
            assert torch.equal(p.data, B.vision_model._params[n].data), n
    return A, B, g


@pytest.mark.parametrize("precision,size,kw", [("fp32", 48, {}), ("fp32_split", 48, {}), ("bf16", 48, {}), ("fp32", 48, dict(gradient_checkpointing=True)),
                                               ("bf16", 128, dict(gradient_checkpointing=True)), ("bf16", 128, dict(attention16_train=True)), ("fp32_split", 128, {})],
                         ids=lambda v: str(v).replace(" ", ""))
def test_training_step_equals_a_native_tower_on_the_resampled_table(precision, size, kw):
    from geoguessr_ai_amd import _lib as L, ops
    A, B, g = _pair(precision, size, **kw)
    A.train(); B.train()
    x = IC.tiny_input(size, size).cuda()
    n16 = L.lib().gg_attention_flash16_bwd_calls()
    oa = A(pixel_values=x); _loss(oa).backward()
    ran16 = L.lib().gg_attention_flash16_bwd_calls() - n16
    ob = B(pixel_values=x); _loss(ob).backward()
    torch.cuda.synchronize()
    assert oa.last_hidden_state.shape == (2, g * g + 1, 128)
    assert torch.equal(oa.pooled_mean, ob.pooled_mean) and torch.equal(oa.last_hidden_state, ob.last_hidden_state)
    ga, gb = _grads(A), _grads(B)
    for n in ga:
        if n == "embeddings.position_embedding.weight":
            continue
        assert torch.equal(ga[n], gb[n]), n
    pa, pb = ga["embeddings.position_embedding.weight"], gb["embeddings.position_embedding.weight"]
    assert pa.shape == (17, 128) and pb.shape == (g * g + 1, 128) and float(pa.abs().sum()) > 0
    assert torch.equal(pa, ops.clip_pos_interp_bwd(pb.contiguous(), 17, (g, g)))
    assert (ran16 > 0) == bool(kw.get("attention16_train")) or size < 128      # 257 tokens: the first size on the 16-bit-MFMA route
    # a second step accumulates into the table's gradient: the adjoint ADDS
    oa2 = A(pixel_values=x); _loss(oa2).backward()
    torch.cuda.synchronize()
    assert torch.equal(A.vision_model._params["embeddings.position_embedding.weight"].grad, pa + pa)
    del A, B
    gc.collect(); torch.cuda.empty_cache()


@pytest.mark.parametrize("precision,size,kw", [("fp16", 48, {}), ("fp8", 48, {}), ("bf16", 128, dict(attention16=True)), ("fp16", 128, dict(attention16=True)),
                                               ("fp8", 128, dict(attention16=True))], ids=lambda v: str(v).replace(" ", ""))
def test_inference_equals_a_native_tower_on_the_resampled_table(precision, size, kw):
    from geoguessr_ai_amd import _lib as L
    A, B, g = _pair(precision, size, **kw)
    _freeze(A).eval(); _freeze(B).eval()
    x = IC.tiny_input(size, size).cuda()
    n16 = L.lib().gg_attention_flash16_calls()
    with torch.no_grad():
        oa = A(pixel_values=x)
        ran16 = L.lib().gg_attention_flash16_calls() - n16
        ob = B(pixel_values=x)
    assert torch.isfinite(oa.last_hidden_state).all()
    assert torch.equal(oa.pooled_mean, ob.pooled_mean) and torch.equal(oa.last_hidden_state, ob.last_hidden_state)
    assert (ran16 > 0) == bool(kw.get("attention16"))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_non_square_128x136_recompute_and_repeat_are_bit_identical(precision):
    """No tower is native at a non-square size, so this case is held to itself -- two steps and the checkpointed step give the same bits -- and, in fp32, to the
    oracle on the torch-interpolated table (test_against_the_oracle's gates)."""
    x = IC.tiny_input(128, 136).cuda()
    runs = []
    for rc in (False, False, True):
        t = IC.tiny_tower(precision, interpolate_pos_encoding=True, gradient_checkpointing=rc).cuda().train()
        o = t(pixel_values=x); _loss(o).backward()
        torch.cuda.synchronize()
        runs.append((o.pooled_mean.detach().clone(), o.last_hidden_state.detach().clone(), _grads(t)))
        del t
    assert runs[0][1].shape == (2, 16 * 17 + 1, 128)
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])
        assert all(torch.equal(runs[0][2][n], other[2][n]) for n in runs[0][2])
    if precision == "fp32":
        st = IC.tiny_weights()
        t = IC.tiny_tower("fp32", interpolate_pos_encoding=True).cuda().train()
        o = t(pixel_values=x); o.pooled_mean.square().sum().backward()
        pooled, ref = IC.oracle_grads(st, x.cpu())
        errs = {n: _rel(p.grad, ref[n]) for n, p in t.vision_model._params.items() if not n.endswith("k_proj.bias") and not n.startswith("post_layernorm")}
        worst = max(errs, key=errs.get)
        print(f"\n[128 x 136 fp32] pooled rel-L2 {_rel(o.pooled_mean.detach(), pooled):.2e}, gradients worst {worst} {errs[worst]:.2e}")
        assert _rel(o.pooled_mean.detach(), pooled) < 1e-4 and errs[worst] < 1e-4


# ------------------------------------------------------------------------------------------- against the oracle and transformers' own run
_ORACLE = {}


def _oracle(H, W):
    if (H, W) not in _ORACLE:
        _ORACLE[(H, W)] = IC.oracle_grads(IC.tiny_weights(), IC.tiny_input(H, W))
    return _ORACLE[(H, W)]


def _measure(precision, H, W):
    """Errors of one step at (H, W) against the fp64 oracle: pooled rel-L2 / max abs, and per-gradient rel-L2 (training modes)."""
    x = IC.tiny_input(H, W)
    pooled, ref = _oracle(H, W)
    tower = IC.tiny_tower(precision, interpolate_pos_encoding=True).cuda()
    if precision in EVAL_MODES:
        _freeze(tower).eval()
        with torch.no_grad():
            o = tower(pixel_values=x.cuda())
        errs = {}
    else:
        tower.train()
        o = tower(pixel_values=x.cuda())
        o.pooled_mean.square().sum().backward()
        # k_proj.bias: its true gradient is zero (softmax ignores a constant added to every key's score): measured against q_proj.bias's, as tests/clip_golden.py does
        errs = {}
        for n, p in tower.vision_model._params.items():
            if n.startswith("post_layernorm"):
                continue
            floor = float(ref[n.replace("k_proj", "q_proj")].norm()) if n.endswith("k_proj.bias") else 0.0
            errs[n] = float((p.grad.double().cpu() - ref[n]).norm() / (ref[n].norm() + floor + 1e-300))
    got = o.pooled_mean.detach().double().cpu()
    return dict(rel=_rel(got, pooled), maxabs=float((got - pooled).abs().max()), errs=errs, last=o.last_hidden_state.detach())


@pytest.mark.parametrize("size", [(40, 56), (24, 24), (128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", TRAIN_MODES + ["fp16"])
def test_against_the_oracle(precision, size):
    """oracle.clip_ref.forward (fp64) fed the torch-interpolated table, and its autograd.  Gates: fp32 and fp32_split -- pooled rel-L2 1e-4, every gradient rel-L2
    1e-4 (tests/test_gpu_clip.py, tests/test_gpu_clip_split.py: the tiny tower's); bf16 -- pooled max abs 3e-2, gradients worst 0.15 and median 5e-2; fp16 -- pooled
    max abs 4e-3 (tests/test_gpu_clip.py).  The native-size figures of the same tower are printed beside them."""
    m, nat = _measure(precision, *size), _measure(precision, 32, 32)
    worst = max(m["errs"], key=m["errs"].get) if m["errs"] else None
    nworst = max(nat["errs"], key=nat["errs"].get) if nat["errs"] else None
    med = float(np.median(list(m["errs"].values()))) if m["errs"] else 0.0
    print(f"\n[{precision} {size[0]} x {size[1]}] pooled rel-L2 {m['rel']:.2e} max abs {m['maxabs']:.2e} (native 32 x 32: {nat['rel']:.2e} / {nat['maxabs']:.2e})"
          + (f"; gradients worst {worst} {m['errs'][worst]:.2e}, median {med:.2e} (native worst {nworst} {nat['errs'][nworst]:.2e})" if worst else ""))
    if precision in ("fp32", "fp32_split"):
        assert m["rel"] < 1e-4 and m["errs"][worst] < 1e-4, sorted(m["errs"].items(), key=lambda kv: -kv[1])[:5]
    elif precision == "bf16":
        assert m["maxabs"] < 3e-2
        assert m["errs"][worst] < 0.15 and med < 5e-2, sorted(m["errs"].items(), key=lambda kv: -kv[1])[:5]
    else:
        assert m["maxabs"] < 4e-3


@pytest.mark.parametrize("size", [(40, 56), (24, 24), (128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fp8_against_its_contract_at_a_foreign_size(size):
    """tests/test_gpu_clip_fp8.py's gates (0.5 e_emu <= e_gpu <= 1.5 e_emu on last_hidden_state, 1 - cos <= 2.25 x the emulation's on the pooled embedding), the
    fp64 forwards fed the torch-interpolated table."""
    from tests import clip_fp8_ref as R
    from tests.test_gpu_clip_fp8 import _gates
    H, W = size
    st = {k: v.double() for k, v in IC.tiny_weights().items()}
    st["embeddings.position_embedding.weight"] = IC.torch_interp(st["embeddings.position_embedding.weight"], H // 8, W // 8)
    x = IC.tiny_input(H, W)
    tower = _freeze(IC.tiny_tower("fp8", interpolate_pos_encoding=True).cuda().eval())
    with torch.no_grad():
        o = tower(pixel_values=x.cuda())
    _gates(f"CLIP tiny fp8 {H} x {W}", o.last_hidden_state, o.pooled_mean, R.forward_fp8(IC.TINY, st, x, quant=False), R.forward_fp8(IC.TINY, st, x, quant=True))


@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16", "fp16"])
def test_against_the_transformers_fixture(golden_dir, precision):
    """transformers' CLIPVisionModel(interpolate_pos_encoding=True) itself: last_hidden_state and the position gradient at 40 x 56 and 24 x 24.  fp32 at the fp32
    gates of tests/test_gpu_clip.py's golden test (rel-L2 1e-4, pooled rtol 1e-4 / atol 2e-5; gradient 1e-4); the 16-bit modes at that test's gates for them."""
    g = np.load(os.path.join(golden_dir, "clip_interp_tiny.npz"))
    for H, W in g["sizes"]:
        H, W = int(H), int(W)
        key = f"{H}x{W}"
        tower = IC.tiny_tower(precision, interpolate_pos_encoding=True).cuda()
        x = IC.tiny_input(H, W).cuda()
        if precision == "fp16":
            _freeze(tower).eval()
            with torch.no_grad():
                o = tower(pixel_values=x)
            e_g = None
        else:
            tower.train()
            o = tower(pixel_values=x)
            o.pooled_mean.square().sum().backward()
            e_g = _rel(tower.vision_model._params["embeddings.position_embedding.weight"].grad, g["g_pos." + key])
        y, lh = o.pooled_mean.detach().cpu().numpy(), o.last_hidden_state.detach().cpu().numpy()
        e_y, e_lh = _rel(y, g["pooled." + key]), _rel(lh, g["last_hidden_state." + key])
        print(f"\n[{precision} {key}] vs transformers: pooled rel-L2 {e_y:.2e} (max abs {np.abs(y - g['pooled.' + key]).max():.2e}), last_hidden rel-L2 {e_lh:.2e}, "
              f"position gradient rel-L2 {e_g if e_g is None else format(e_g, '.2e')}")
        if precision in ("fp32", "fp32_split"):
            assert e_y < 1e-4 and e_lh < 1e-4 and e_g < 1e-4
            np.testing.assert_allclose(y, g["pooled." + key], rtol=1e-4, atol=2e-5)
        elif precision == "fp16":
            assert np.abs(y - g["pooled." + key]).max() < 4e-3 and e_lh < 2e-3
        else:
            assert np.abs(y - g["pooled." + key]).max() < 3e-2 and e_lh < 2e-2 and e_g < 0.15


# ------------------------------------------------------------------------------------------- trainable masks, lifecycle
def test_frozen_table_and_last_layer_finetune_at_a_foreign_size():
    """The last-layer fine-tune (SuperGuessr's policy with a pretrained head) at 40 x 56: nothing embedding-side trains, so no adjoint runs; its gradients equal the
    all-trainable step's.  With only the position table frozen the other embedding gradients are unchanged and the table's slice of the flat buffer stays zero."""
    x = IC.tiny_input(40, 56).cuda()

    def run(frozen):
        t = IC.tiny_tower("fp32", interpolate_pos_encoding=True).cuda().train()
        for n, p in t.vision_model._params.items():
            p.requires_grad = not frozen(n)
        o = t(pixel_values=x); _loss(o).backward()
        torch.cuda.synchronize()
        return _grads(t), t.vision_model.flat_grads().clone(), {e["name"]: e for e in t.vision_model.table}

    full, _, _ = run(lambda n: False)
    last, _, _ = run(lambda n: not n.startswith("encoder.layers.1."))
    assert all(torch.equal(last[n], full[n]) for n in last if last[n] is not None) and sum(v is not None for v in last.values()) == 16
    nopos, flat, table = run(lambda n: n == "embeddings.position_embedding.weight")
    e = table["embeddings.position_embedding.weight"]
    assert float(flat[e["offset"]:e["offset"] + e["numel"]].abs().max()) == 0.0
    assert all(torch.equal(nopos[n], full[n]) for n in nopos if nopos[n] is not None)


def test_sizes_alternate_and_a_backward_belongs_to_the_size_of_its_forward():
    from geoguessr_ai_amd import _lib as L
    t = IC.tiny_tower("fp32", interpolate_pos_encoding=True).cuda().train()
    xs = {s: IC.tiny_input(*s).cuda() for s in ((40, 56), (32, 32), (24, 24))}
    want = {}
    for s, x in xs.items():
        t.zero_grad(set_to_none=True)
        o = t(pixel_values=x); _loss(o).backward()
        want[s] = (o.last_hidden_state.detach().clone(), _grads(t))
    # again in another order, with an eval forward at another size between a training forward and its backward
    for s in ((24, 24), (40, 56), (32, 32)):
        t.zero_grad(set_to_none=True)
        o = t(pixel_values=xs[s])
        with torch.no_grad():
            t(pixel_values=xs[(40, 56) if s != (40, 56) else (24, 24)])
        _loss(o).backward()
        assert torch.equal(o.last_hidden_state, want[s][0])
        assert all(torch.equal(p, want[s][1][n]) for n, p in _grads(t).items()), s
    # the existing refusal keeps its wording: a second training forward takes the workspace
    o1 = t(pixel_values=xs[(40, 56)])
    t(pixel_values=xs[(24, 24)])
    with pytest.raises(L.GgError, match="every training forward must be followed by its backward"):
        _loss(o1).backward()
    # new weights reach the resampled table of the cache
    with torch.no_grad():
        t.vision_model._params["embeddings.position_embedding.weight"].mul_(0.5)
        assert not torch.equal(t(pixel_values=xs[(40, 56)]).last_hidden_state, want[(40, 56)][0])


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_growing_sizes_in_one_tower_equal_fresh_towers(training):
    """24 x 24 -> 32 x 32 -> 40 x 56 in ONE tower: the workspace grows from call to call, the native call leaves a cache without a table and the larger foreign
    size regrows it, and 24 x 24 again finds a cache large enough and rebuilds the table alone.  Each call equals a fresh tower's, bit for bit."""
    def run(t, x):
        if not training:
            with torch.no_grad():
                o = t(pixel_values=x)
            return o.pooled_mean.clone(), o.last_hidden_state.clone(), {}
        t.zero_grad(set_to_none=True)
        o = t(pixel_values=x)
        _loss(o).backward()
        torch.cuda.synchronize()
        return o.pooled_mean.detach().clone(), o.last_hidden_state.detach().clone(), _grads(t)

    def make():
        t = IC.tiny_tower("fp32", interpolate_pos_encoding=True).cuda()
        return t.train() if training else _freeze(t).eval()
    one = make()
    sizes, ws, wc = [], [], []
    for s in ((24, 24), (32, 32), (40, 56), (24, 24)):
        x = IC.tiny_input(*s).cuda()
        got, want = run(one, x), run(make(), x)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), s
        assert all(torch.equal(got[2][n], want[2][n]) for n in want[2]), s
        vm = one.vision_model
        ws.append(vm._ws[training].numel()); wc.append(vm._wcache.numel())
    assert ws[0] < ws[1] < ws[2] == ws[3], ws                                    # grown to the largest call, then kept
    assert wc[1] == wc[0] and wc[2] > wc[1] and wc[3] == wc[2], wc               # regrown for the larger table, then kept


# ------------------------------------------------------------------------------------------- through the mirrors
def test_superguessr_clipmodel_and_clipembedding_at_a_foreign_size(centroids):
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPEmbedding, clip_preprocess
    from geoguessr_ai_amd.pretrain.clip_model import CLIPModel
    from tests import clip_text_golden as TG
    hs, inter, nl, nh, img, ps = IC.TINY
    # SuperGuessr calls base_model(pixel_values=...) with no other keyword: the tower default carries the flag
    tower = IC.tiny_tower("fp32", interpolate_pos_encoding=True)
    model = SuperGuessr(base_model=tower, panorama=True, should_smooth_labels=True).cuda().train()
    x = torch.stack([IC.tiny_input(40, 56, B=4, seed=s) for s in (1, 2)]).cuda()                   # (N, 4, 3, 40, 56)
    labels = torch.tensor([[10.75, 59.91], [-73.98, 40.75]]).cuda()
    out = model(pixel_values=x, labels=labels)
    out.loss.backward()
    ref = IC.oracle_forward(IC.tiny_weights(), x.flatten(0, 1).cpu()).view(2, 4, hs)
    assert out.embedding.shape == (2, 4, hs) and _rel(out.embedding.detach(), ref) < 1e-4 and np.isfinite(float(out.loss.detach()))
    assert float(tower.vision_model._params["embeddings.position_embedding.weight"].grad.abs().sum()) > 0
    # CLIPModel: the keyword of transformers' get_image_features / forward
    cfg = TG.tiny_config()
    cfg["vision"] = dict(hidden_size=hs, intermediate_size=inter, num_layers=nl, num_heads=nh, image_size=img, patch_size=ps)
    m = CLIPModel(config=cfg, precision="fp32").cuda().eval()
    m.vision_tower.load_hf_state_dict(IC.tiny_weights())
    xi = IC.tiny_input(24, 24).cuda()
    with pytest.raises(Exception, match=r"expects \(B,3,32,32\)"):
        m.get_image_features(pixel_values=xi)
    feats = m.get_image_features(pixel_values=xi, interpolate_pos_encoding=True)
    with torch.no_grad():
        lh = m.vision_tower(pixel_values=xi, interpolate_pos_encoding=True).last_hidden_state
        pooled = torch.nn.functional.layer_norm(lh[:, 0].double(), (hs,), m.vision_model._params["post_layernorm.weight"].double(),
                                                m.vision_model._params["post_layernorm.bias"].double(), 1e-5)
    assert feats.shape == (2, cfg["projection_dim"]) and _rel(feats, pooled @ m.visual_projection.weight.double().T) < 1e-4
    ids = torch.randint(1, 60, (2, 8), generator=torch.Generator().manual_seed(3))
    ids[:, -1] = 63
    fw = m(input_ids=ids.cuda(), pixel_values=xi, interpolate_pos_encoding=True)
    assert fw.logits_per_image.shape == (2, 2) and torch.isfinite(fw.logits_per_image).all()
    # CLIPEmbedding(image_size=...): raw images are brought to that size and the tower (here one layer of ViT-B/32, native 224) resamples its table
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (300, 448, 3), dtype=np.uint8)
    for bt in (False, True):
        e = CLIPEmbedding("openai/clip-vit-base-patch32", device="cuda", precision="fp32", num_layers=1, image_size=288, batch_transform=bt)
        assert e.image_size == 288 and e.clip_model.cfg.image_size == 224 and e.clip_model.interpolate_pos_encoding
        px = clip_preprocess(img, 288, "cuda")
        assert px.shape == (1, 3, 288, 288)
        a = e(img)
        with torch.no_grad():
            o = e.clip_model(pixel_values=px)
        assert o.last_hidden_state.shape == (1, 82, 768) and a.shape == (1, 768) and torch.allclose(a, o.pooled_mean, atol=1e-5)
        assert e(torch.randn(2, 3, 224, 224).cuda()).shape == (2, 768)      # pixel_values at the native size still run
    with pytest.raises(ValueError, match="multiple of the patch size"):
        CLIPEmbedding("openai/clip-vit-base-patch32", device="cuda", precision="fp32", num_layers=1, image_size=300)
