"""The long-sequence attention forward on the 16-bit MFMA (gg_attention_flash16_fwd, include/gg_attn16.h) and the CLIP vision tower's opt-in route to it
(gg_clip_set_attention16, ``attention16=True``) on the GPU.

* Conditioning: the cases of tests/attention16_cases.py through ``attention_cases.check`` (e <= 4 max(yardstick, floor) for out and lse; the CPU file shows the
  restated contract meets the same gates).
* Integer data: every product and sum exact, so a k-permutation mismatch between the P operand and the V fragment -- which random data only blurs -- is a wrong
  integer.
* Interface: both qkv layouts, padded pitches (16-byte and 8-byte aligned rows), lse NULL, determinism, independence of num_windows, refusals with the output
  untouched.
* Tower: ViT-L/14-336 dimensions, two layers, one image (577 tokens), seeded weights, with the switch on, against the modes' own gates; the launch counter; the
  routes that must not move."""
import ctypes as C
import math

import pytest
import torch

from tests import attention16_cases as A
from tests import attention_cases as AC

pytestmark = pytest.mark.gpu
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def _ops():
    from geoguessr_ai_amd import ops
    return ops


def _run(qkv, kw, **more):
    return _ops().attention_flash16(qkv.cuda() if not qkv.is_cuda else qkv, **kw, **more)


def _kw(c):
    return {k: v for k, v in c["kw"].items() if k not in ("map_h", "map_w", "head_dim", "window_size")}


# ------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("storage,N,cls", A.params())
def test_conditioning(storage, N, cls):
    c = A.get_case(storage, N, cls)
    out, lse = _run(c["qkv"], _kw(c), want_lse=True)
    got = {"out": AC.canon_out(c, out), "lse": AC.canon_lse(c, lse)}
    bad = AC.check(c, got, f"flash16 {storage} N={N}", tensors=("out", "lse"))
    assert not bad, bad


# ------------------------------------------------------------------------------------------- integer data
@pytest.mark.parametrize("storage", A.STORAGES)
@pytest.mark.parametrize("N", [17, 65, 320, 577])
def test_scale_zero_gives_the_column_mean(storage, N):
    """scale = 0: every P is exactly 1, O the exact integer column sum of v, l = N; out is the mean up to the one output rounding, lse = log N."""
    st = DT[storage]
    q, k, v = A.integer_case(N, st)
    qkv, kw = A.flat_qkv(q, k, v, "clip", st)
    out, lse = _run(qkv, kw, scale=0.0, want_lse=True)
    c = dict(idx=AC.token_index("clip", N, 2, 0, 0), windows=2, N=N, heads=2, hd=64)
    got, mean = AC.canon_out(c, out), v.mean(-2, keepdim=True).expand_as(v)
    err = (got - mean).abs()
    assert bool((err <= A.half_ulp(mean, st)).all()), float((err / A.half_ulp(mean, st).clamp_min(1e-30)).max())
    assert float((lse.double().cpu() - math.log(N)).abs().max()) <= 1e-6


@pytest.mark.parametrize("storage", A.STORAGES)
@pytest.mark.parametrize("N", [1, 17, 65, 320, 577])
def test_one_hot_rows_select_a_v_row_bit_for_bit(storage, N):
    """Query i aligned with key (7 i + 3) mod N at a margin where every other P is exactly 0: out[i] is that key's v row, bit for bit, wherever the key sits in
    its tile -- with the V fragment in another k order than the P operand it is another row's (or a mixture)."""
    st = DT[storage]
    q, k, v, sel, margin = A.one_hot_case(N)
    assert margin >= 16
    qkv, kw = A.flat_qkv(q, k, v, "clip", st)
    out, lse = _run(qkv, kw, scale=8.0, want_lse=True)
    c = dict(idx=AC.token_index("clip", N, 2, 0, 0), windows=2, N=N, heads=2, hd=64)
    assert torch.equal(AC.canon_out(c, out), v[:, :, sel])
    assert float((lse.double().cpu() - 512.0).abs().max()) <= 2e-4          # 64 * 8: the selected score, l = 1; three f32 roundings at magnitude 739 (ulp 6.1e-5)


# ------------------------------------------------------------------------------------------- interface
def _plain(storage, N):
    return A.get_case(storage, N, "plain")


@pytest.mark.parametrize("storage", A.STORAGES)
@pytest.mark.parametrize("layout", ["clip", "tinyvit"])
@pytest.mark.parametrize("pad", [8, 24, 4])
def test_layouts_and_padded_pitches(storage, layout, pad):
    """Both qkv layouts with ld and ldo padded (8, 24: 16-byte rows; 4: 8-byte rows, the two-load form): the bits of the unpadded clip-layout call."""
    st, N = DT[storage], 257
    c = _plain(storage, N)
    want, want_lse = _run(c["qkv"], _kw(c), want_lse=True)
    qkv, kw = A.flat_qkv(c["q"], c["k"], c["v"], layout, st, pad=pad)
    qkv = qkv.cuda()
    outbuf = torch.full((qkv.shape[0], 128 + pad), float("nan"), dtype=st, device="cuda")
    out, lse = _run(qkv[:, :384], kw, want_lse=True, out=outbuf[:, :128])
    assert out.data_ptr() == outbuf.data_ptr() and qkv.stride(0) == 384 + pad
    assert torch.equal(out, want) and torch.equal(lse, want_lse)
    assert bool(torch.isnan(outbuf[:, 128:].float()).all())                  # the row padding of out is untouched


@pytest.mark.parametrize("storage", A.STORAGES)
def test_lse_null_determinism_and_window_independence(storage):
    c = _plain(storage, 320)
    kw = _kw(c)
    qkv = c["qkv"].cuda()
    out, lse = _run(qkv, kw, want_lse=True)
    assert torch.equal(_run(qkv, kw), out)                                  # lse NULL: the same out
    again, lse2 = _run(qkv, kw, want_lse=True)
    assert torch.equal(again, out) and torch.equal(lse2, lse)               # two calls, the same bits
    for w in (0, 1):                                                        # window w alone
        one, lse1 = _run(qkv[w * 320:(w + 1) * 320], dict(kw, num_windows=1), want_lse=True)
        assert torch.equal(one, out[w * 320:(w + 1) * 320]) and torch.equal(lse1, lse[w * 320:(w + 1) * 320])
    three = torch.cat([qkv, qkv[:320]])
    out3 = _run(three, dict(kw, num_windows=3))
    assert torch.equal(out3[:640], out) and torch.equal(out3[640:], out[:320])


def test_refusals_leave_the_output_untouched():
    from geoguessr_ai_amd import _lib as L
    from tests.test_attention16_cpu import REFUSALS
    lib = L.lib()
    c = _plain("f16", 65)
    qkv = c["qkv"].cuda()
    out = torch.full((130, 128), 7.0, dtype=torch.float16, device="cuda")
    lse = torch.full((130, 2), 7.0, device="cuda")
    aux = torch.zeros(64, device="cuda")
    for over, dtype, msg in REFUSALS:
        a = L.AttnArgs()
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), 384, 0, 128, 256, 64, 64
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.scale = 2, 2, 65, 0, 0.125
        a.out, a.ldo, a.lse = out.data_ptr(), 128, lse.data_ptr()
        for k, v in over.items():
            if k in ("bias", "bias_table", "window_map", "num_windows_dev"):
                v = aux.data_ptr()
            elif k == "qkv" and v is not None:
                v = qkv.data_ptr() + 8
            elif k == "out" and v is not None:
                v = out.data_ptr() + 8
            setattr(a, k, v)
        assert lib.gg_attention_flash16_fwd(C.byref(a), dtype, L.stream()) != 0, (over, dtype)
        err = lib.gg_last_error().decode()
        assert err.startswith("gg_attention_flash16_fwd:") and msg in err, err
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all())


def test_bits_unchanged_from_the_parent_build(golden_dir):
    """out and lse of the seeded calls of tests/attention16_cases.py::parent_bits equal, bit for bit, what the build before the head-dim 64 and the head-dim 32
    kernel became one template gave (tests/golden/attention16_parent.npz, tools/make_attention16_parent_golden.py)."""
    import os
    import numpy as np
    gold = np.load(os.path.join(golden_dir, "attention16_parent.npz"))
    got = A.parent_bits(_ops(), window=False)
    assert sorted(got) == sorted(k for k in gold.files if k.startswith("lin_")) and got
    for name, x in got.items():
        assert x.dtype == gold[name].dtype and np.array_equal(x, gold[name]), name


# ------------------------------------------------------------------------------------------- the tower with the switch on
L14 = "openai/clip-vit-large-patch14-336"
B32 = "openai/clip-vit-base-patch32"


def _l14(layers=2):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIP_CONFIGS
    kw = dict(CLIP_CONFIGS[L14], num_layers=layers)
    return kw, (kw["hidden_size"], kw["intermediate_size"], layers, kw["num_heads"], kw["image_size"], kw["patch_size"])


@pytest.fixture(scope="module")
def l14_case():
    """Seeded two-layer ViT-L/14-336 weights, one image, and the fp64 forwards (plain, and with the fp8 contract's quantisation) -- computed once."""
    from tests import clip_fp8_ref as R
    kw, cfg = _l14()
    st = R.seeded_state(cfg, seed=2)
    x = torch.randn(1, 3, 336, 336, generator=torch.Generator().manual_seed(9))
    return dict(kw=kw, cfg=cfg, st=st, x=x, ref=R.forward_fp8(cfg, st, x, quant=False), emu=R.forward_fp8(cfg, st, x, quant=True))


@pytest.fixture()
def switch():
    """The library switch, restored to off whatever the test did."""
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    lib.gg_clip_set_attention16(0)
    yield lib
    lib.gg_clip_set_attention16(0)


def _embedder(case, precision, **more):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPEmbedding
    return CLIPEmbedding(L14, device="cuda", state_dict=case["st"], precision=precision, num_layers=2, **more)


@pytest.mark.parametrize("precision", ["fp8", "fp16", "bf16"])
def test_tower_with_the_switch_on_meets_the_modes_gates(l14_case, switch, precision):
    """``attention16=True`` against the gates the mode already has: fp8 the two of tests/test_gpu_clip_fp8.py (0.5 e_emu <= e_gpu <= 1.5 e_emu, pooled 1 - cos
    within 2.25 x), fp16 / bf16 the rel-L2 of last_hidden_state against the fp64 forward under 2e-3 / 2e-2 (tests/test_gpu_clip.py).  The switch-off figure is
    printed beside each.  The launch counter advances by num_layers per forward with the keyword, by 0 without."""
    from tests import clip_fp8_ref as R
    from tests.test_gpu_clip_fp8 import _gates
    lib, x = switch, l14_case["x"].cuda()
    n0 = lib.gg_attention_flash16_calls()
    off = _embedder(l14_case, precision).clip_model(pixel_values=x)
    assert lib.gg_attention_flash16_calls() == n0
    tower = _embedder(l14_case, precision, attention16=True).clip_model
    assert tower.attention16 and tower.precision == precision
    on = tower(pixel_values=x)
    assert lib.gg_attention_flash16_calls() == n0 + 2
    assert lib.gg_clip_set_attention16(0) == 0                              # the keyword set the switch for its own call only
    ref = l14_case["ref"]
    e_off, e_on = R.rel_l2(off.last_hidden_state, ref[1]), R.rel_l2(on.last_hidden_state, ref[1])
    print(f"\n[L/14-336 x2 {precision}] last_hidden rel-L2 against fp64: switch off {e_off:.3e}, on {e_on:.3e}; pooled 1 - cos: off "
          f"{R.one_minus_cos(off.pooled_mean, ref[0]):.3e}, on {R.one_minus_cos(on.pooled_mean, ref[0]):.3e}")
    if precision == "fp8":
        _gates("L/14-336 x2 fp8, attention16", on.last_hidden_state, on.pooled_mean, ref, l14_case["emu"])
    else:
        assert e_on < (2e-3 if precision == "fp16" else 2e-2)
    assert not torch.equal(on.last_hidden_state, off.last_hidden_state)     # another kernel, other roundings


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_switch_off_on_off_on(l14_case, switch, precision):
    """The library switch flipped between forwards of one tower: the off results are the bits of a forward taken before the switch was touched, the on results
    agree with each other, for one image and for a batch of two run twice in a row (the second is the call a cached graph would replay); the counter advances
    by num_layers on the first forward after the switch is set and by 0 with it off."""
    lib = switch
    tower = _embedder(l14_case, precision).clip_model
    x1 = l14_case["x"].cuda()
    x2 = torch.cat([x1, x1.flip(-1)])
    base = {1: tower(pixel_values=x1).last_hidden_state.clone(), 2: tower(pixel_values=x2).last_hidden_state.clone()}
    on = {}
    for setting in (0, 1, 0, 1):
        lib.gg_clip_set_attention16(setting)
        for b, x in ((1, x1), (2, x2), (2, x2)):
            n = lib.gg_attention_flash16_calls()
            got = tower(pixel_values=x).last_hidden_state
            assert lib.gg_attention_flash16_calls() - n == (2 if setting else 0)
            if setting == 0:
                assert torch.equal(got, base[b]), (setting, b)
            else:
                assert torch.equal(got, on.setdefault(b, got.clone())), (setting, b)
                assert not torch.equal(got, base[b])
    lib.gg_clip_set_attention16(0)


def test_routes_the_switch_does_not_move(l14_case, switch):
    """A training forward (bf16, 577 tokens), a ViT-B/32 tower (50 tokens), an fp32 L/14 tower and the text tower: bit-identical with the switch on and off, and
    no launch of the new kernel."""
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    from tests import clip_fp8_ref as R
    lib = switch
    x1 = l14_case["x"].cuda()
    runs = {}

    def train_fwd():
        tower = CLIPVisionTower(L14, precision="bf16", num_layers=2).cuda().train()
        tower.load_hf_state_dict(l14_case["st"])
        return tower(pixel_values=x1).last_hidden_state.detach().clone()

    def b32():
        tower = CLIPVisionTower(B32, precision="fp16", num_layers=2, seed=3).cuda().eval()
        for p in tower.parameters():
            p.requires_grad = False
        x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
        return tower(pixel_values=x).last_hidden_state.clone()

    def f32():
        tower = CLIPVisionTower(L14, precision="fp32", num_layers=1, seed=3).cuda().eval()
        for p in tower.parameters():
            p.requires_grad = False
        return tower(pixel_values=x1).last_hidden_state.clone()

    def text():
        from geoguessr_ai_amd.pretrain.clip_model import CLIPModel
        cfg = dict(text=dict(hidden_size=128, intermediate_size=256, num_layers=2, num_heads=2),
                   vision=dict(hidden_size=128, intermediate_size=256, num_layers=1, num_heads=2, image_size=64, patch_size=32), projection_dim=64)
        model = CLIPModel(B32, seed=1, precision="bf16", config=cfg).cuda().eval()
        ids = torch.randint(3, 1000, (2, 77), generator=torch.Generator().manual_seed(6))
        ids[:, -1] = 49407
        with torch.no_grad():
            return model.get_text_features(input_ids=ids.cuda()).clone()

    routes = dict(train=train_fwd, b32=b32, f32=f32, text=text)
    for setting in (0, 1):
        lib.gg_clip_set_attention16(setting)
        n = lib.gg_attention_flash16_calls()
        for name, fn in routes.items():
            runs[(name, setting)] = fn()
        assert lib.gg_attention_flash16_calls() == n
    lib.gg_clip_set_attention16(0)
    for name in routes:
        assert torch.equal(runs[(name, 0)], runs[(name, 1)]), name
