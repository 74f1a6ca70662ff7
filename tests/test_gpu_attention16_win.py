"""The 16-bit-MFMA window attention forward beyond 256 tokens (gg_attention_flash16_win_fwd, include/gg_attn16w.h) and TinyViT's opt-in route to it
(gg_tinyvit_set_attention16, ``attention16=True``) on the GPU.

* Conditioning: the cases of tests/attention16_win_cases.py through ``attention_cases.check`` (e <= 4 max(yardstick, floor) for out and lse, the bias unrounded;
  the CPU file shows the restated contract meets the same gates).
* Exact data: the bias as a mask (every P exactly 1 or 0: a wrong gather index, window partition or P / V k order is another integer), scale 0 with a zero table
  (the column mean), one-hot rows (a v row bit for bit).
* Interface: bias_table NULL, a window alone or among four, determinism, lse NULL, independence of num_windows, both qkv layouts, padded pitches, refusals with
  the output untouched.
* Model: tiny_vit_21m_384 / _512 cut to a few blocks, at sizes that pad the stage-2 window (288, 320) and one that does not (768), bf16 eval with the keyword
  against the existing bf16 eval gates; the launch counter; off / on / off / on over captured graphs; the routes that must not move; the other surfaces."""
import ctypes as C
import gc
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention16_cases as AL
from tests import attention16_win_cases as A
from tests import attention_cases as AC

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ops():
    from geoguessr_ai_amd import ops
    return ops


def _run(qkv, kw, **more):
    return _ops().attention_flash16_win(qkv if qkv.is_cuda else qkv.cuda(), **kw, **more)


def _table(t):
    return None if t is None else t.float().contiguous().cuda()


# ------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("ws,cls", A.params())
def test_conditioning(ws, cls):
    c = A.get_case(ws, cls)
    out, lse = _run(c["qkv"], c["kw"], bias_table=_table(c["table"]), want_lse=True)
    got = {"out": AC.canon_out(c, out), "lse": AC.canon_lse(c, lse)}
    bad = AC.check(c, got, f"flash16_win ws={ws} map={c['map_hw']}", tensors=("out", "lse"))
    assert not bad, bad


# ------------------------------------------------------------------------------------------- exact data
@pytest.mark.parametrize("ws,m", [(5, 2), (17, 2), (24, 1), (32, 1)])
def test_bias_as_an_exact_mask(ws, m):
    """q = 0 and a table of 0 on S_h / -200 elsewhere: out[q] is the mean of the integer v over the keys whose (|dy|, |dx|) from q is in S_h -- an exact sum, one
    division, one rounding -- and lse the log of their number."""
    W = 2 * m * m
    q, k, v, table, mean, count = A.mask_case(ws, W)
    qkv, kw, idx = A.flat_qkv(q, k, v, ws, m)
    out, lse = _run(qkv, kw, bias_table=_table(table), want_lse=True)
    got = A.canon(idx, out, 2)
    err, tol = (got - mean).abs(), A.half_ulp(mean)
    assert bool((err <= tol).all()), (int((err > tol).sum()), float(err.max()))
    assert float((A.canon(idx, lse, 2) - torch.log(count)[None]).abs().max()) <= 1e-6


@pytest.mark.parametrize("ws", [9, 17, 32])
def test_scale_zero_with_a_zero_table_gives_the_column_mean(ws):
    N = ws * ws
    q, k, v = A.integer_case(ws, 2)
    qkv, kw, idx = A.flat_qkv(q, k, v, ws, 1)
    out, lse = _run(qkv, kw, bias_table=torch.zeros(2, N, device="cuda"), scale=0.0, want_lse=True)
    got, mean = A.canon(idx, out, 2), v.mean(-2, keepdim=True).expand_as(v)
    err = (got - mean).abs()
    assert bool((err <= A.half_ulp(mean)).all()), float((err / A.half_ulp(mean).clamp_min(1e-30)).max())
    assert float((lse.double().cpu() - math.log(N)).abs().max()) <= 1e-6


@pytest.mark.parametrize("ws", [9, 17, 32])
def test_one_hot_rows_select_a_v_row_bit_for_bit(ws):
    """Query i aligned with key (7 i + 3) mod N at a margin where every other P is exactly 0: out[i] is that key's v row, bit for bit, wherever the key sits in its
    tile."""
    q, k, v, sel, margin = A.one_hot_case(ws)
    assert margin >= 4 and margin * A.ONE_HOT_SCALE * A.LOG2E >= 150
    qkv, kw, idx = A.flat_qkv(q, k, v, ws, 1)
    out, lse = _run(qkv, kw, bias_table=torch.zeros(2, ws * ws, device="cuda"), scale=A.ONE_HOT_SCALE, want_lse=True)
    assert torch.equal(A.canon(idx, out, 2), v[:, :, sel])
    # 32 * 32: the selected score, l = 1; three f32 roundings at magnitude 1477 (ulp 1.2e-4)
    assert float((lse.double().cpu() - A.HD * A.ONE_HOT_SCALE).abs().max()) <= 4e-4


# ------------------------------------------------------------------------------------------- interface
def _canon_case(ws, W, seed=0):
    g = torch.Generator().manual_seed(977 * ws + seed)
    q, k, v = (torch.randn(W, 2, ws * ws, A.HD, generator=g).to(BF).double() for _ in range(3))
    table = (0.5 * torch.randn(2, ws * ws, generator=g)).float()
    return q, k, v, table


def test_null_table_equals_a_zero_table():
    ws = 17
    q, k, v, _ = _canon_case(ws, 4)
    qkv, kw, _ = A.flat_qkv(q, k, v, ws, 2)
    qkv = qkv.cuda()
    a, la = _run(qkv, kw, want_lse=True)
    b, lb = _run(qkv, kw, bias_table=torch.zeros(2, ws * ws, device="cuda"), want_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert bool(torch.isfinite(a.float()).all())


@pytest.mark.parametrize("ws", [5, 17])
def test_a_window_alone_or_among_four(ws):
    """The same four windows' data as one 2 x 2 map (gathered) and as four maps of one window each (linear): the same bits per window."""
    q, k, v, table = _canon_case(ws, 4)
    tab = _table(table)
    qkv2, kw2, idx2 = A.flat_qkv(q, k, v, ws, 2)
    qkv1, kw1, idx1 = A.flat_qkv(q, k, v, ws, 1)
    o2, l2 = _run(qkv2, kw2, bias_table=tab, want_lse=True)
    o1, l1 = _run(qkv1, kw1, bias_table=tab, want_lse=True)
    assert torch.equal(A.canon(idx2, o2, 2), A.canon(idx1, o1, 2)) and torch.equal(A.canon(idx2, l2, 2), A.canon(idx1, l1, 2))
    assert not torch.equal(o2, o1)                                           # (the rows really are in another order)


def test_lse_null_determinism_and_window_independence():
    ws, N = 17, 289
    q, k, v, table = _canon_case(ws, 2)
    tab = _table(table)
    qkv, kw, _ = A.flat_qkv(q, k, v, ws, 1)
    qkv = qkv.cuda()
    out, lse = _run(qkv, kw, bias_table=tab, want_lse=True)
    assert torch.equal(_run(qkv, kw, bias_table=tab), out)                   # lse NULL: the same out
    again, lse2 = _run(qkv, kw, bias_table=tab, want_lse=True)
    assert torch.equal(again, out) and torch.equal(lse2, lse)                # two calls, the same bits
    for w in (0, 1):                                                         # window w alone
        one, lse1 = _run(qkv[w * N:(w + 1) * N], dict(kw, num_windows=1), bias_table=tab, want_lse=True)
        assert torch.equal(one, out[w * N:(w + 1) * N]) and torch.equal(lse1, lse[w * N:(w + 1) * N])
    three = torch.cat([qkv, qkv[:N]])
    out3 = _run(three, dict(kw, num_windows=3), bias_table=tab)
    assert torch.equal(out3[:2 * N], out) and torch.equal(out3[2 * N:], out[:N])


@pytest.mark.parametrize("layout", ["tinyvit", "clip"])
@pytest.mark.parametrize("pad", [8, 4])
def test_layouts_and_padded_pitches(layout, pad):
    """Both qkv layouts with ld and ldo padded (8: 16-byte rows; 4: 8-byte rows, the two-load form): the bits of the unpadded tinyvit-layout call."""
    ws = 17
    q, k, v, table = _canon_case(ws, 4)
    tab = _table(table)
    base, kwb, _ = A.flat_qkv(q, k, v, ws, 2)
    want, want_lse = _run(base, kwb, bias_table=tab, want_lse=True)
    qkv, kw, _ = A.flat_qkv(q, k, v, ws, 2, layout=layout, pad=pad)
    qkv = qkv.cuda()
    outbuf = torch.full((qkv.shape[0], 64 + pad), float("nan"), dtype=BF, device="cuda")
    out, lse = _run(qkv[:, :192], kw, bias_table=tab, want_lse=True, out=outbuf[:, :64])
    assert out.data_ptr() == outbuf.data_ptr() and qkv.stride(0) == 192 + pad
    assert torch.equal(out, want) and torch.equal(lse, want_lse)
    assert bool(torch.isnan(outbuf[:, 64:].float()).all())                   # the row padding of out is untouched


def test_refusals_leave_the_output_untouched():
    from geoguessr_ai_amd import _lib as L
    from tests.test_attention16_win_cpu import REFUSALS, WHO
    lib = L.lib()
    ws, N = 17, 289
    q, k, v, table = _canon_case(ws, 4)
    qkv, _, _ = A.flat_qkv(q, k, v, ws, 2)
    qkv = qkv.cuda()
    out = torch.full((4 * N, 64), 7.0, dtype=BF, device="cuda")
    lse = torch.full((4 * N, 2), 7.0, device="cuda")
    tab = _table(table)
    aux = torch.zeros(1156, device="cuda")
    n0 = lib.gg_attention_flash16_win_calls()
    for over, dtype, msg in REFUSALS:
        a = L.AttnArgs()
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), 192, 0, 32, 64, 96, 32
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = 2, 4, N, ws, 2 * ws, 2 * ws, 32 ** -0.5
        a.bias_table, a.out, a.ldo, a.lse = tab.data_ptr(), out.data_ptr(), 64, lse.data_ptr()
        for key, val in over.items():
            if key in ("bias", "window_map", "num_windows_dev", "dbias"):
                val = aux.data_ptr()
            elif key == "bias_table" and val is not None:
                val = tab.data_ptr() + 2
            elif key == "lse":
                val = lse.data_ptr() + 2
            elif key == "qkv" and val is not None:
                val = qkv.data_ptr() + 8
            elif key == "out" and val is not None:
                val = out.data_ptr() + 8
            setattr(a, key, val)
        assert lib.gg_attention_flash16_win_fwd(C.byref(a), dtype, L.stream()) != 0, (over, dtype)
        err = lib.gg_last_error().decode()
        assert err.startswith(WHO + ":") and msg in err, err
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all())
    assert lib.gg_attention_flash16_win_calls() == n0


def test_bits_unchanged_from_the_parent_build(golden_dir):
    """out and lse of the seeded calls of tests/attention16_cases.py::parent_bits equal, bit for bit, what the build before the head-dim 64 and the head-dim 32
    kernel became one template gave (tests/golden/attention16_parent.npz, tools/make_attention16_parent_golden.py)."""
    import os
    gold = np.load(os.path.join(golden_dir, "attention16_parent.npz"))
    got = AL.parent_bits(_ops(), window=True)
    assert sorted(got) == sorted(k for k in gold.files if k.startswith("win_")) and got
    for name, x in got.items():
        assert x.dtype == gold[name].dtype and np.array_equal(x, gold[name]), name


# ------------------------------------------------------------------------------------------- the model with the switch on
# id -> (variant, img_size, depths, batch, stage-2 blocks, the oracle needs the padded block)
MODELS = {
    "21m384_288": ("tiny_vit_21m_384", 288, (1, 1, 2, 1), 2, 2, True),       # tests/test_gpu_window_pad.py::MODEL_CASES: 18 -> one padded 24 x 24 window, 576 tokens
    "21m512_320": ("tiny_vit_21m_512", 320, (1, 1, 1, 1), 2, 1, True),       # likewise: 20 -> one padded 32 x 32 window, 1024 tokens
    "21m384_768": ("tiny_vit_21m_384", 768, (1, 1, 1, 1), 1, 1, False),      # 48 x 48 map: four unpadded 24 x 24 windows per image
}


@pytest.fixture(autouse=True)
def _fresh_graph_cache_and_switch():
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    lib.gg_graph_clear(); lib.gg_tinyvit_set_attention16(0)
    yield
    lib.gg_graph_clear(); lib.gg_tinyvit_set_attention16(0)


def _lib():
    from geoguessr_ai_amd import _lib as L
    return L.lib()


def _free(*objs):
    del objs
    gc.collect(); torch.cuda.empty_cache()


def _state(case_id, seed=3):
    """Seeded weights with randomised running statistics (tests/test_gpu_window_pad.py::test_eval_surfaces_at_160), as a CPU state dict."""
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from tests.test_gpu_precision import _randomize
    name, img, depths, *_ = MODELS[case_id]
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(name, pretrained=False, precision="bf16", drop_path_rate=0.0, img_size=img, depths=depths)
    _randomize(base.backbone, seed + 1)
    st = {k: v.detach().cpu().clone() for k, v in base.backbone.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    for k in st:
        if k.endswith("running_mean"):
            st[k] = 0.1 * torch.randn(st[k].shape, generator=g)
        elif k.endswith("running_var"):
            st[k] = 0.5 + torch.rand(st[k].shape, generator=g)
    return st


_CASES = {}


def _case(case_id):
    if case_id not in _CASES:
        name, img, depths, batch, *_ = MODELS[case_id]
        x = torch.randn(batch, 3, img, img, generator=torch.Generator().manual_seed(1))
        _CASES[case_id] = dict(st=_state(case_id), x=x)
    return _CASES[case_id]


def _adapter(case_id, precision="bf16", drop_path_rate=0.0, **more):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    name, img, depths, *_ = MODELS[case_id]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(name, pretrained=False, precision=precision, drop_path_rate=drop_path_rate, img_size=img, depths=depths, seed=0, **more)
    base.backbone.load_state_dict(_case(case_id)["st"])
    return base.cuda().eval()


@pytest.mark.parametrize("case_id", list(MODELS))
def test_model_with_the_keyword_meets_the_bf16_eval_gates(monkeypatch, case_id):
    """``attention16=True`` against the gates the bf16 eval forward already has (tests/test_gpu_window_pad.py::test_eval_surfaces_at_160, tests/test_gpu_model.py):
    max |err| 4e-2 against the bf16-emulating oracle, 8e-2 and cosine 0.999 against the fp32 oracle.  The switch-off figures are printed beside.  The launch counter
    advances by the number of stage-2 blocks on the first call (a new graph key runs eagerly); gg_attention_flash16_calls does not move."""
    from oracle import tinyvit_ref as R
    from tests import tinyvit_pad_ref as P
    name, img, depths, batch, blocks, pads = MODELS[case_id]
    case = _case(case_id)
    if pads:
        monkeypatch.setattr(R, "_tinyvit_block_m", P.tinyvit_block_padded)
    cfg = R.config_for(name, drop_path_rate=0.0, img_size=img, depths=depths)
    with torch.no_grad():
        ref = R.forward(cfg, case["st"], case["x"], training=False)
        emu = R.forward(cfg, case["st"], case["x"], training=False, emulate_bf16=True)
    lib, x = _lib(), case["x"].cuda()
    off_m = _adapter(case_id)
    assert bool(off_m.backbone.padded_maps) == pads
    n0, c0 = lib.gg_attention_flash16_win_calls(), lib.gg_attention_flash16_calls()
    with torch.no_grad():
        off = off_m(pixel_values=x).pooler_output.float().cpu()
    assert lib.gg_attention_flash16_win_calls() == n0
    on_m = _adapter(case_id, attention16=True)
    assert on_m.backbone.attention16
    with torch.no_grad():
        on = on_m(pixel_values=x).pooler_output.float().cpu()
    assert lib.gg_attention_flash16_win_calls() == n0 + blocks and lib.gg_attention_flash16_calls() == c0
    assert lib.gg_tinyvit_set_attention16(0) == 0                            # the keyword set the switch for its own call only
    cos = lambda a, b: float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0))
    for label, got in (("off", off), ("on", on)):
        print(f"\n[{case_id} bf16 eval, attention16 {label}] max|err| against the bf16-emulating oracle {float((got - emu).abs().max()):.3e}, against fp32 "
              f"{float((got - ref).abs().max()):.3e}, cosine {cos(got, ref):.6f}")
    assert float((on - emu).abs().max()) < 4e-2
    assert float((on - ref).abs().max()) < 8e-2 and cos(on, ref) > 0.999
    assert not torch.equal(on, off)                                          # another kernel, other roundings
    _free(off_m, on_m)


def _graph_stats():
    from tests.test_gpu_recompute import _stats
    return _stats()


@pytest.mark.parametrize("case_id", ["21m384_288", "21m384_768"])
def test_switch_off_on_off_on_over_captured_graphs(case_id):
    """The library switch flipped between forwards of one backbone, three calls per setting (eager, capture, replay; the graph key holds the switch): every off
    result is the bits of a backbone built without the keyword and run before the switch was touched, the on results agree with each other and differ from off."""
    lib, x = _lib(), _case(case_id)["x"].cuda()
    blocks = MODELS[case_id][4]
    ref_m = _adapter(case_id)
    with torch.no_grad():
        base = ref_m.backbone.forward_hip(x, False).clone()
    bb = _adapter(case_id).backbone
    on = None
    cap0, rep0 = _graph_stats()
    for setting in (0, 1, 0, 1):
        lib.gg_tinyvit_set_attention16(setting)
        for call in range(3):
            n = lib.gg_attention_flash16_win_calls()
            got = bb.forward_hip(x, False)
            moved = lib.gg_attention_flash16_win_calls() - n
            assert moved in ((0, blocks) if setting else (0,)), (setting, call, moved)          # (a replay enqueues the captured launches: the host counter stands)
            if setting == 0:
                assert torch.equal(got, base), (setting, call)
            else:
                on = got.clone() if on is None else on
                assert torch.equal(got, on), (setting, call)
                assert not torch.equal(got, base)
            del got                                                          # same addresses on the next call: the graph path replays
    cap1, rep1 = _graph_stats()
    print(f"\n[{case_id}] graphs captured {cap1 - cap0}, replays {rep1 - rep0}")
    assert cap1 - cap0 >= 2 and rep1 - rep0 >= 2                             # one graph per setting, each replayed
    lib.gg_tinyvit_set_attention16(0)
    _free(ref_m, bb)


def test_routes_the_switch_does_not_move():
    """With the process switch forced to 1: a train-mode step (forward output and gradients), an fp32 eval forward and a tiny_vit_5m_224 bf16 eval forward (no
    window beyond 256 tokens) equal their switch-off results bit for bit (the attention-bias gradients, which the backward sums with float atomics, to rounding:
    tests/test_gpu_recompute.py::_grad_mismatches), and the counter does not move."""
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from tests.test_gpu_recompute import _grad_mismatches, _step
    lib = _lib()
    case_id = "21m384_288"
    x = _case(case_id)["x"].cuda()
    runs, bbs = {}, {}

    def train():
        m = _adapter(case_id, drop_path_rate=0.1).train()
        m.unfreeze_all()
        bb = bbs["train"] = m.backbone
        drop = bb.make_drop_scales(x.shape[0], generator=torch.Generator().manual_seed(11))
        d_out = torch.randn(x.shape[0], bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
        out, grad, buf, _ = _step(bb, x, drop, d_out)
        assert float(grad.abs().sum()) > 0
        return out, grad, buf

    def f32():
        m = _adapter(case_id, precision="fp32")
        with torch.no_grad():
            return (m.backbone.forward_hip(x, False).clone(),)

    def small():
        torch.manual_seed(2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="bf16", drop_path_rate=0.0, depths=(1, 1, 2, 1), seed=2).cuda().eval()
        xs = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
        with torch.no_grad():
            return (m.backbone.forward_hip(xs, False).clone(),)

    routes = dict(train=train, f32=f32, small=small)
    for setting in (0, 1):
        lib.gg_graph_clear()
        lib.gg_tinyvit_set_attention16(setting)
        n = lib.gg_attention_flash16_win_calls()
        for name, fn in routes.items():
            runs[(name, setting)] = fn()
        assert lib.gg_attention_flash16_win_calls() == n, setting
    lib.gg_tinyvit_set_attention16(0)
    for name in routes:
        a, b = runs[(name, 0)], runs[(name, 1)]
        assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]), name
    _, g0, s0 = runs[("train", 0)]
    _, g1, s1 = runs[("train", 1)]
    bad = _grad_mismatches(bbs["train"], g0, g1)
    assert not bad, bad[:6]
    assert torch.equal(s0, s1)                                               # running statistics
    _free(bbs)


def test_the_other_surfaces_route_to_the_kernel(monkeypatch):
    """TinyViTEmbedding, TinyViTClassifier.forward and SuperGuessr(serving=True) over an ``attention16=True`` adapter, by the launch counter; the same surfaces
    without the keyword launch nothing."""
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    lib = _lib()
    case_id = "21m384_288"
    name, img, depths, batch, blocks, _ = MODELS[case_id]
    x = _case(case_id)["x"].cuda()
    cent = np.stack([np.linspace(-170, 170, 40), np.linspace(-80, 80, 40)], 1).astype(np.float32)
    for keyword in (False, True):
        more = {"attention16": True} if keyword else {}
        want = blocks if keyword else 0
        lib.gg_graph_clear()
        n = lib.gg_attention_flash16_win_calls()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = TinyViTClassifier(name, num_classes=7, precision="bf16", img_size=img, depths=depths, drop_path_rate=0.0, seed=4, **more).cuda().eval()
        with torch.no_grad():
            logits = clf(x)
        assert logits.shape == (batch, 7) and bool(torch.isfinite(logits).all())
        assert lib.gg_attention_flash16_win_calls() - n == want, ("classifier", keyword)

        lib.gg_graph_clear()
        n = lib.gg_attention_flash16_win_calls()
        model = SuperGuessr(_adapter(case_id, **more), panorama=False, serving=True, centroids=cent).cuda().eval()
        with torch.no_grad():
            llh, topk, emb = model(pixel_values=x)
        assert emb.shape[0] == batch and bool(torch.isfinite(emb).all())
        assert lib.gg_attention_flash16_win_calls() - n == want, ("serving", keyword)

        lib.gg_graph_clear()
        n = lib.gg_attention_flash16_win_calls()
        monkeypatch.setenv("GG_PRECISION", "bf16")                           # the embedder has no precision keyword
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            e = TinyViTEmbedding(model_name="tiny_vit_21m_384", device="cuda", load_checkpoint=False, panorama=False, img_size=288, **more)
        assert e.tinyvit_model.backbone.attention16 is keyword and e.tinyvit_model.backbone.precision == "bf16"
        v = e(x[:1])
        assert v.shape[0] == 1 and bool(torch.isfinite(v).all())
        assert lib.gg_attention_flash16_win_calls() - n == (6 if keyword else 0), ("embedder", keyword)          # the full model: six stage-2 blocks
        _free(clf, model, e)
    assert lib.gg_tinyvit_set_attention16(0) == 0
