"""The long-sequence attention backward on the 16-bit MFMA (gg_attention_flash16_bwd, include/gg_attn16b.h) and the bf16 CLIP vision tower's opt-in training
route to the 16-bit-MFMA pair (gg_clip_set_attention16_train, ``attention16_train=True``) on the GPU.

* Conditioning: the cases of tests/attention16_bwd_cases.py through ``attention_cases.check`` (e <= 4 max(yardstick, floor) for dq, dk, dv; the CPU file shows the
  restated contract meets the same gates), with out and lse from the 16-bit-MFMA forward.
* One-hot and two-hot rows: every expected value is bf16-exact, so a k-order mismatch in the dV, dK or dQ product, an lse or delta taken from a neighbouring
  row, or a pad row that leaks -- which random data only blurs -- is a wrong bit.
* Interface: both qkv layouts, padded pitches (16-byte and 8-byte aligned rows), untouched columns, determinism, independence of num_windows, the f32-MFMA
  forward's out / lse as input, refusals with the output untouched.
* Tower: the token geometry of ViT-L/14-336 (577 tokens) at hidden 128, two layers, batch 2, all tensors trainable, against fp64 autograd through
  oracle.clip_ref.forward, relative to the figure of the switch-off run; the launch counters; recompute; the routes that must not move."""
import ctypes as C

import pytest
import torch

from tests import attention16_bwd_cases as B
from tests import attention16_cases as A
from tests import attention_cases as AC

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _ops():
    from geoguessr_ai_amd import ops
    return ops


def _fwd(qkv, kw, **more):
    return _ops().attention_flash16(qkv, **kw, want_lse=True, **more)


def _bwd(qkv, out, lse, dout, kw, **more):
    return _ops().attention_flash16_bwd(qkv, out, lse, dout, **kw, **more)


# ------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("N,cls", B.params())
def test_conditioning(N, cls):
    c = B.get_case(N, cls)
    kw, qkv, dout = B.kw_of(c), c["qkv"].cuda(), c["dout"].cuda()
    out, lse = _fwd(qkv, kw)
    dqkv = _bwd(qkv, out, lse, dout, kw)
    got = dict(zip(("dq", "dk", "dv"), AC.canon_dqkv(c, dqkv)))
    bad = B.check(c, got, f"flash16 bwd N={N}")
    assert not bad, bad


# ------------------------------------------------------------------------------------------- exact families
def _exact(c):
    """dq, dk, dv of the kernel pair on an exact family's inputs, canonical; the forward's out must already be the closed form."""
    qkv, dout, kw = B.flat_inputs(c)
    qkv, dout = qkv.cuda(), dout.cuda()
    out, lse = _fwd(qkv, kw, scale=c["scale"])
    W, H, N, D = c["q"].shape
    cc = dict(idx=AC.token_index("clip", N, W, 0, 0), windows=W, N=N, heads=H, hd=D)
    assert torch.equal(AC.canon_out(cc, out), c["out"])
    return B.canon(c["q"].shape, "clip", _bwd(qkv, out, lse, dout, kw, scale=c["scale"])), lse


@pytest.mark.parametrize("N", B.ONE_HOT_SIZES)
def test_one_hot_rows_bit_for_bit(N):
    """Query i aligned with key sel(i) = (7 i + 3) mod N at a margin where every other P is exactly 0, integer dout: dv[sel(i)] is dout[i] bit for bit wherever
    the key sits in its tile, and dq = dk = 0 exactly (dP = delta on the selected key)."""
    c = B.one_hot_bwd_case(N)
    assert c["margin"] >= 13
    got, _ = _exact(c)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], c["want"][n]), (n, float((got[n] - c["want"][n]).abs().max()))


@pytest.mark.parametrize("N", B.TWO_HOT_SIZES)
def test_two_hot_rows_bit_for_bit(N):
    """P exactly 1/2 on two keys (tests/attention16_bwd_cases.py, two_hot_case): dq, dk, dv equal the closed form bit for bit -- the k order of the dK and dQ
    products, which random data only blurs."""
    c = B.two_hot_case(N)
    got, lse = _exact(c)
    assert float((lse.double().cpu() - c["lse"]).abs().max()) <= 2e-4
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], c["want"][n]), (n, float((got[n] - c["want"][n]).abs().max()))


# ------------------------------------------------------------------------------------------- interface
def _plain(N):
    return B.get_case(N, "plain")


@pytest.mark.parametrize("layout", ["clip", "tinyvit"])
@pytest.mark.parametrize("pad", [8, 24, 4])
def test_layouts_padded_pitches_and_untouched_columns(layout, pad):
    """Both qkv layouts with ld, ldo and lddo padded (8, 24: 16-byte rows; 4: 8-byte rows): the bits of the unpadded clip-layout call, and
    the pad columns of dqkv keep their NaN."""
    N = 257
    c = _plain(N)
    kw0, qkv0, dout0 = B.kw_of(c), c["qkv"].cuda(), c["dout"].cuda()
    out0, lse0 = _fwd(qkv0, kw0)
    want = B.canon((2, 2, N, 64), "clip", _bwd(qkv0, out0, lse0, dout0, kw0))
    qkv, kw = A.flat_qkv(c["q"], c["k"], c["v"], layout, BF16, pad=pad)
    qkv = qkv.cuda()
    wide = lambda t: torch.cat([t, torch.full((t.shape[0], pad), float("nan"), dtype=BF16, device="cuda")], 1)[:, :t.shape[1]]
    out, dout = wide(out0), wide(dout0)
    dbuf = torch.full_like(qkv, float("nan"))
    dqkv = _bwd(qkv[:, :384], out, lse0, dout, kw, dqkv=dbuf[:, :384])
    assert dqkv.data_ptr() == dbuf.data_ptr() and qkv.stride(0) == 384 + pad and out.stride(0) == 128 + pad
    got = B.canon((2, 2, N, 64), layout, dqkv)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], want[n]), n
    assert bool(torch.isnan(dbuf[:, 384:].float()).all())                    # the row padding of dqkv is untouched
    assert not bool(torch.isnan(dbuf[:, :384].float()).any())                # the dq, dk, dv columns of every token are written


def test_columns_outside_q_k_v_are_untouched():
    """Head stride 256 with [q | k | v | 64 foreign columns] per head: the foreign block of dqkv keeps its fill, the zero fill of ops.attention_flash16_bwd shows."""
    N = 65
    c = _plain(N)
    kw0, qkv0, dout = B.kw_of(c), c["qkv"].cuda(), c["dout"].cuda()
    out, lse = _fwd(qkv0, kw0)
    want = B.canon((2, 2, N, 64), "clip", _bwd(qkv0, out, lse, dout, kw0))
    q5 = qkv0.view(2 * N, 3, 2, 64).permute(0, 2, 1, 3)                      # (tokens, heads, 3, 64)
    qkv = torch.cat([q5, torch.full((2 * N, 2, 1, 64), float("nan"), dtype=BF16, device="cuda")], 2).reshape(2 * N, 512).contiguous()
    kw = dict(kw0, q_off=0, k_off=64, v_off=128, head_stride=256)
    dbuf = torch.full_like(qkv, 7.0)
    _bwd(qkv, out, lse, dout, kw, dqkv=dbuf)
    d4 = dbuf.view(2 * N, 2, 4, 64)
    assert bool((d4[:, :, 3] == 7.0).all())
    zero = _bwd(qkv, out, lse, dout, kw).view(2 * N, 2, 4, 64)
    assert bool((zero[:, :, 3] == 0).all()) and torch.equal(zero[:, :, :3], d4[:, :, :3])
    got = d4[:, :, :3].contiguous().double().cpu().view(2, N, 2, 3, 64).permute(3, 0, 2, 1, 4)
    for i, n in enumerate(("dq", "dk", "dv")):
        assert torch.equal(got[i], want[n]), n


def test_determinism_and_window_independence():
    N = 320
    c = _plain(N)
    kw, qkv, dout = B.kw_of(c), c["qkv"].cuda(), c["dout"].cuda()
    out, lse = _fwd(qkv, kw)
    dqkv = _bwd(qkv, out, lse, dout, kw)
    assert torch.equal(_bwd(qkv, out, lse, dout, kw), dqkv)                  # two calls, the same bits
    for w in (0, 1):                                                         # window w alone
        s = slice(w * N, (w + 1) * N)
        assert torch.equal(_bwd(qkv[s], out[s], lse[s], dout[s], dict(kw, num_windows=1)), dqkv[s])
    three = lambda t: torch.cat([t, t[:N]])
    d3 = _bwd(three(qkv), three(out), three(lse), three(dout), dict(kw, num_windows=3))
    assert torch.equal(d3[:2 * N], dqkv) and torch.equal(d3[2 * N:], dqkv[:N])


def test_out_and_lse_of_the_f32_mfma_forward_pass_the_same_gates():
    """Either forward's out / lse is a valid input: gg_attention_flash_fwd (dtype 0) in front of the new backward, N = 257, every class."""
    for cls in AC.classes_for(False, False):
        c = B.get_case(257, cls)
        qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
        out, lse = _ops().attention_flash(qkv, want_lse=True, **c["kw"])
        got = dict(zip(("dq", "dk", "dv"), AC.canon_dqkv(c, _bwd(qkv, out, lse, dout, B.kw_of(c)))))
        bad = B.check(c, got, "flash16 bwd after the f32-MFMA forward N=257")
        assert not bad, bad


def test_refusals_leave_the_output_untouched():
    from geoguessr_ai_amd import _lib as L
    from tests.test_attention16_bwd_cpu import REFUSALS
    lib = L.lib()
    c = _plain(65)
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    out, lse = _fwd(qkv, B.kw_of(c))
    dqkv = torch.full((130, 384), float("nan"), dtype=BF16, device="cuda")
    aux = torch.zeros(64, device="cuda")
    ptrs = dict(qkv=qkv, out=out, dout=dout, dqkv=dqkv)
    before = lib.gg_attention_flash16_bwd_calls()
    for over, dtype, msg in REFUSALS:
        a = L.AttnArgs()
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), 384, 0, 128, 256, 64, 64
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = 2, 2, 65, 0, 0.125
        a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = out.data_ptr(), 128, lse.data_ptr(), dout.data_ptr(), 128, dqkv.data_ptr()
        for k, v in over.items():
            if k in ("bias", "bias_table", "dbias", "window_map", "num_windows_dev"):
                v = aux.data_ptr()
            elif k in ptrs and v is not None:
                v = ptrs[k].data_ptr() + 8
            setattr(a, k, v)
        assert lib.gg_attention_flash16_bwd(C.byref(a), dtype, L.stream()) != 0, (over, dtype)
        err = lib.gg_last_error().decode()
        assert err.startswith("gg_attention_flash16_bwd:") and msg in err, err
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv.float()).all()) and lib.gg_attention_flash16_bwd_calls() == before


# ------------------------------------------------------------------------------------------- the tower with the switch on
L14 = "openai/clip-vit-large-patch14-336"
CFG = (128, 256, 2, 2, 336, 14)          # hidden, intermediate, layers, heads, image, patch: 577 tokens


@pytest.fixture()
def switch():
    """The library switches, restored to off whatever the test did."""
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    lib.gg_clip_set_attention16_train(0); lib.gg_clip_set_attention16(0)
    yield lib
    lib.gg_clip_set_attention16_train(0); lib.gg_clip_set_attention16(0)


@pytest.fixture(scope="module")
def tower_case():
    """Seeded weights, two images, d_out, and fp64: the pooled mean and every gradient by autograd through oracle.clip_ref.forward (loss = sum(pooled * d_out)),
    last_hidden_state from the same op sequence restated in tests/clip_fp8_ref.py (the oracle returns the pooled mean only) -- computed once."""
    from oracle import clip_ref as CR
    from tests import clip_fp8_ref as R
    st = R.seeded_state(CFG, seed=5)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 336, 336, generator=g)
    d_out = torch.randn(2, CFG[0], generator=g)
    st64 = {n: p.double().requires_grad_(True) for n, p in st.items()}
    pooled = CR.forward(CR.ClipVisionConfig(*CFG), st64, x.double())
    (pooled * d_out.double()).sum().backward()
    grads = {n: t.grad for n, t in st64.items()}
    pooled_r, last = R.forward_fp8(CFG, st, x, quant=False)
    assert float((pooled_r - pooled.detach()).abs().max()) <= 1e-12
    return dict(st=st, x=x, d_out=d_out, pooled=pooled.detach(), last=last, grads=grads)


def _tower(case, **more):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    tower = CLIPVisionTower(L14, precision="bf16", hidden_size=CFG[0], intermediate_size=CFG[1], num_layers=CFG[2], num_heads=CFG[3], **more).cuda().train()
    tower.load_hf_state_dict(case["st"])
    return tower


def _step(tower, case):
    """One training step: last_hidden_state and every gradient (clones), and how far the two launch counters moved in the forward and in the backward."""
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    for p in tower.vision_model._params.values():
        p.grad = None
    n = [(lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls())]
    res = tower(pixel_values=case["x"].cuda())
    n.append((lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls()))
    (res.pooled_mean * case["d_out"].cuda()).sum().backward()
    torch.cuda.synchronize()
    n.append((lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls()))
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in tower.vision_model._params.items()}
    moved = dict(fwd=(n[1][0] - n[0][0], n[1][1] - n[0][1]), bwd=(n[2][0] - n[1][0], n[2][1] - n[1][1]))
    return res.last_hidden_state.detach().clone(), grads, moved


def _figures(case, last, grads):
    """rel-L2 against fp64 per tensor; k_proj.bias, whose exact gradient is zero, relative to the q_proj.bias gradient of its layer (tests/clip_golden.py's rule)."""
    from tests import clip_fp8_ref as R
    fig = {"last_hidden_state": R.rel_l2(last, case["last"])}
    for n, ref in case["grads"].items():
        if ref is None:                                       # post_layernorm: not on the path
            assert grads[n] is None or float(grads[n].abs().max()) == 0.0, n
            continue
        if n.endswith("k_proj.bias"):
            qb = case["grads"][n.replace("k_proj", "q_proj")]
            fig[n] = float((grads[n].double().cpu() - ref).norm() / qb.norm())
        else:
            fig[n] = R.rel_l2(grads[n], ref)
    return fig


def test_tower_training_step_with_the_switch_on(tower_case, switch):
    """``attention16_train=True`` against fp64, per tensor at most 1.5 x the figure of the switch-off run of the same test (existing code, never the code under
    test); the counters: 2 forward launches per training forward and 2 backward calls per backward with the keyword, 0 without; the library switch reads 0 after
    each call; results with the switch on and off are not bit-equal."""
    lib = switch
    last_off, g_off, m_off = _step(_tower(tower_case), tower_case)
    assert m_off == dict(fwd=(0, 0), bwd=(0, 0)), m_off
    tower = _tower(tower_case, attention16_train=True)
    assert tower.attention16_train and not tower.attention16
    last_on, g_on, m_on = _step(tower, tower_case)
    assert m_on == dict(fwd=(2, 0), bwd=(0, 2)), m_on
    assert lib.gg_clip_set_attention16_train(0) == 0 and lib.gg_clip_set_attention16(0) == 0      # the keyword set the switch for its own calls only
    f_off, f_on = _figures(tower_case, last_off, g_off), _figures(tower_case, last_on, g_on)
    print("\n[L/14-336 geometry, hidden 128 x 2 layers, bf16] rel-L2 against fp64, switch off / on:")
    bad = []
    for n in f_off:
        print(f"  {n:55s} {f_off[n]:.3e} {f_on[n]:.3e}  x{f_on[n] / f_off[n]:.2f}")
        if not f_on[n] <= 1.5 * f_off[n]:
            bad.append((n, f_off[n], f_on[n]))
    assert not bad, bad
    assert not torch.equal(last_on, last_off)                                 # another kernel, other roundings
    assert any(not torch.equal(g_on[n], g_off[n]) for n in g_on if g_on[n] is not None)


def test_recompute_gives_the_same_bits_and_replays_through_the_same_kernel(tower_case, switch):
    """Gradient checkpointing on and off with the keyword on: the same bits.  Under recompute the backward re-forms every kept layer below the top one (the top
    layer's tensors are still the forward's) through the same forward kernel: one more forward launch per re-formed layer."""
    last0, g0, m0 = _step(_tower(tower_case, attention16_train=True), tower_case)
    last1, g1, m1 = _step(_tower(tower_case, attention16_train=True, gradient_checkpointing=True), tower_case)
    assert m0 == dict(fwd=(2, 0), bwd=(0, 2)), m0
    assert m1 == dict(fwd=(2, 0), bwd=(CFG[2] - 1, 2)), m1
    assert torch.equal(last0, last1)
    for n in g0:
        assert (g0[n] is None and g1[n] is None) or torch.equal(g0[n], g1[n]), n
    # without the keyword the replay does not reach the new kernels either
    _, _, m2 = _step(_tower(tower_case, gradient_checkpointing=True), tower_case)
    assert m2 == dict(fwd=(0, 0), bwd=(0, 0)), m2


def test_switch_that_differs_between_forward_and_backward(tower_case, switch):
    """The f32-MFMA training forward followed by a backward with the library switch on (and the reverse): not refused, the backward of the step goes through
    the kernel the switch names when it is enqueued, and every gradient stays within 1.5 x the switch-off figure."""
    lib = switch
    _, g_off, _ = _step(_tower(tower_case), tower_case)
    f_off = _figures(tower_case, tower_case["last"], g_off)
    for fwd_on in (0, 1):
        tower = _tower(tower_case)
        for p in tower.vision_model._params.values():
            p.grad = None
        lib.gg_clip_set_attention16_train(fwd_on)
        n0 = (lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls())
        res = tower(pixel_values=tower_case["x"].cuda())
        lib.gg_clip_set_attention16_train(1 - fwd_on)
        (res.pooled_mean * tower_case["d_out"].cuda()).sum().backward()
        torch.cuda.synchronize()
        lib.gg_clip_set_attention16_train(0)
        n1 = (lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls())
        assert (n1[0] - n0[0], n1[1] - n0[1]) == ((2, 0) if fwd_on else (0, 2))
        grads = {k: p.grad for k, p in tower.vision_model._params.items()}
        f = _figures(tower_case, tower_case["last"], grads)
        bad = [(n, f_off[n], f[n]) for n in f if n != "last_hidden_state" and not f[n] <= 1.5 * f_off[n]]
        assert not bad, (fwd_on, bad)


def test_routes_the_training_switch_does_not_move(tower_case, switch):
    """An inference forward of the same tower is bit-identical with the keyword on and off, and with the library switch on: no launch of the new kernels; a
    50-token tower's training step does not move either."""
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    lib = switch
    x = tower_case["x"].cuda()
    n0 = (lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls())
    runs = []
    for more, setting in ((dict(), 0), (dict(attention16_train=True), 0), (dict(), 1)):
        lib.gg_clip_set_attention16_train(setting)
        tower = _tower(tower_case, **more).eval()
        with torch.no_grad():
            runs.append(tower(pixel_values=x).last_hidden_state.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    small = {}
    for setting in (0, 1):
        lib.gg_clip_set_attention16_train(setting)
        t = CLIPVisionTower("openai/clip-vit-base-patch32", precision="bf16", num_layers=1, seed=3, hidden_size=128, intermediate_size=256, num_heads=2).cuda().train()
        xs = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
        res = t(pixel_values=xs)
        res.pooled_mean.sum().backward()
        small[setting] = (res.last_hidden_state.detach().clone(), t.vision_model._params["encoder.layers.0.self_attn.q_proj.weight"].grad.clone())
    lib.gg_clip_set_attention16_train(0)
    assert torch.equal(small[0][0], small[1][0]) and torch.equal(small[0][1], small[1][1])
    assert (lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls()) == n0
