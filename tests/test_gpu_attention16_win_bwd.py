"""The 16-bit-MFMA window attention backward beyond 256 tokens (gg_attention_flash16_win_bwd, include/gg_attn16wb.h) and the bf16 TinyViT's opt-in training route to
the 16-bit-MFMA kernels (gg_tinyvit_set_attention16_train, ``attention16_train=True``) on the GPU.

Kernel
* K1 conditioning: the cases of tests/attention16_win_bwd_cases.py through ``attention_cases.check`` (e <= 4 max(yardstick, floor) for dq, dk, dv, dbias; the CPU
  file shows the restated contract meets the same gates), with out and lse from the 16-bit-MFMA forward.
* K2 one-hot and two-hot rows: every expected value is bf16- / f32-exact, so a k-order mismatch in the dV, dK or dQ product, an lse or delta taken from a
  neighbouring row, a bias bin of the wrong offset or a pad row that leaks -- which random data only blurs -- is a wrong bit.
* K3 the f32-MFMA forward's out / lse as input; K4 determinism, independence of ``want_dbias``, of num_windows and of the window's place in its map, a NULL table
  against a zero table, dbias with and without the scratch; K5 both qkv layouts, padded pitches, untouched columns and rows; K6 the f32-pipe backward through the
  same gate; K7 refusals with the outputs untouched; K8 the head-dim-64 entry point's bits against the parent build's (tests/golden/attention16_bwd_parent.npz).

Model: the padded 576- and 1024-token cases of tests/test_gpu_window_pad.py through its own gate with the switch on (M1), a 768-pixel model with four unpadded
windows per image against the bf16-emulating oracle at the same gradient bounds, recompute (M2), a switch that differs between forward and backward (M3), frozen
attention biases (M4), the routes the switch does not move (M5), captured graphs (M6)."""
import ctypes as C
import gc
import os
import warnings

import numpy as np
import pytest
import torch

from tests import attention16_win_bwd_cases as WB
from tests import attention16_win_cases as WC
from tests import attention_cases as AC

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
F32 = torch.float32


def _ops():
    from geoguessr_ai_amd import ops
    return ops


def _lib():
    from geoguessr_ai_amd import _lib as L
    return L.lib()


def _dev(t):
    return None if t is None else t.cuda()


def _fwd(qkv, kw, table=None, **more):
    return _ops().attention_flash16_win(qkv, **kw, bias_table=table, want_lse=True, **more)


def _bwd(qkv, out, lse, dout, kw, table=None, **more):
    return _ops().attention_flash16_win_bwd(qkv, out, lse, dout, **kw, bias_table=table, **more)


def _got(c, dqkv, dbias):
    got = dict(zip(("dq", "dk", "dv"), AC.canon_dqkv(c, dqkv)))
    got["dbias"] = None if dbias is None else dbias.double().cpu()
    return got


def _case_tensors(c):
    return c["qkv"].cuda(), c["dout"].cuda(), _dev(c["table"]), WB.kw_of(c)


# ------------------------------------------------------------------------------------------- K1: conditioning
@pytest.mark.parametrize("ws,cls", WB.params())
def test_conditioning(ws, cls):
    c = WB.get_case(ws, cls)
    qkv, dout, table, kw = _case_tensors(c)
    out, lse = _fwd(qkv, kw, table)
    dqkv, dbias = _bwd(qkv, out, lse, dout, kw, table, want_dbias=True)
    bad = WB.check(c, _got(c, dqkv, dbias), f"flash16 win bwd ws={ws}")
    assert not bad, bad


# ------------------------------------------------------------------------------------------- K2: exact families
def _exact(c, out=None, lse=None):
    qkv, dout, kw, idx = WB.flat_inputs(c, c["ws"], c["m"])
    qkv, dout, table = qkv.cuda(), dout.cuda(), c["table"].cuda()
    if out is None:
        out, lse = _fwd(qkv, kw, table, scale=c["scale"])
        assert torch.equal(WC.canon(idx, out, 2), c["out"])                  # the forward's out is already the closed form
    dqkv, dbias = _bwd(qkv, out, lse, dout, kw, table, want_dbias=True, scale=c["scale"])
    got = WB.canon(idx, 2, "tinyvit", dqkv)
    got["dbias"] = dbias.double().cpu()
    return got


@pytest.mark.parametrize("ws", WB.ONE_HOT_SIZES)
def test_one_hot_rows_bit_for_bit(ws):
    """Query i aligned with key sel(i) = (7 i + 3) mod N at a margin where every other P is exactly 0, integer dout, a zero table: dv[sel(i)] is dout[i] bit for
    bit wherever the key sits in its tile and its window in the map, and dq = dk = 0 and dbias = 0 exactly (dP = delta on the selected key, so dS = 0)."""
    c = WB.one_hot_bwd_case(ws)
    got = _exact(c)
    for n in WB.TENSORS:
        assert torch.equal(got[n], c["want"][n]), (n, float((got[n] - c["want"][n]).abs().max()))


def test_two_hot_rows_bit_for_bit():
    """P exactly 1/2 on two keys (tests/attention16_win_bwd_cases.py, two_hot_case; out and lse given in closed form): dq, dk, dv and dbias equal the closed form
    bit for bit -- the k order of the dK and dQ products and the signed-offset bin of every pair, which random data only blurs."""
    c = WB.two_hot_case()
    idx = AC.token_index("tinyvit", c["N"], c["windows"], c["ws"], c["m"] * c["ws"])
    out = WB.flat_out(idx, c["out"]).to(BF16).cuda()
    lse = torch.full((idx.numel(), 2), c["lse"], dtype=F32).cuda()
    got = _exact(c, out, lse)
    for n in WB.TENSORS:
        assert torch.equal(got[n], c["want"][n]), (n, float((got[n] - c["want"][n]).abs().max()))


# ------------------------------------------------------------------------------------------- K3, K6: the other forward, the other backward
@pytest.mark.parametrize("ws", [17, 24])
def test_out_and_lse_of_the_f32_mfma_forward_pass_the_same_gates(ws):
    """Either forward's out / lse is a valid input: gg_attention_flash_fwd (dtype 0) in front of the new backward, every class."""
    for cls in AC.classes_for(True, False):
        c = WB.get_case(ws, cls)
        qkv, dout, table, kw = _case_tensors(c)
        out, lse = _ops().attention_flash(qkv, want_lse=True, bias_table=table, **c["kw"])
        dqkv, dbias = _bwd(qkv, out, lse, dout, kw, table, want_dbias=True)
        bad = WB.check(c, _got(c, dqkv, dbias), f"flash16 win bwd after the f32-MFMA forward ws={ws}")
        assert not bad, bad


@pytest.mark.parametrize("ws", [17, 24])
def test_the_f32_pipe_backward_passes_the_same_gate(ws):
    """gg_attention_bwd (beyond 256 tokens: the streaming f32-MFMA pair) on the same inputs, out / lse of the 16-bit forward: the yardstick does not favour the new
    kernel."""
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    for cls in AC.classes_for(True, False):
        c = WB.get_case(ws, cls)
        qkv, dout, table, kw = _case_tensors(c)
        out, lse = _fwd(qkv, kw, table)
        dqkv, dbias = torch.zeros_like(qkv), torch.zeros_like(table)
        rows = lib.gg_attention_flash_dbias_rows(kw["num_windows"], kw["tokens_per_window"])
        scratch = torch.empty(rows * 2 * ws * ws, dtype=F32, device="cuda")
        a = L.AttnArgs()
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), qkv.stride(0), kw["q_off"], kw["k_off"], kw["v_off"], kw["head_stride"], 32
        a.num_heads, a.num_windows, a.tokens_per_window = kw["num_heads"], kw["num_windows"], kw["tokens_per_window"]
        a.window_size, a.map_h, a.map_w, a.scale = ws, kw["map_h"], kw["map_w"], 32 ** -0.5
        a.bias_table, a.dbias, a.dbias_scratch = table.data_ptr(), dbias.data_ptr(), scratch.data_ptr()
        a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = out.data_ptr(), out.stride(0), lse.data_ptr(), dout.data_ptr(), dout.stride(0), dqkv.data_ptr()
        L.check(lib.gg_attention_bwd(C.byref(a), L.stream()), "gg_attention_bwd")
        bad = WB.check(c, _got(c, dqkv, dbias), f"f32-pipe gg_attention_bwd ws={ws}")
        assert not bad, bad


# ------------------------------------------------------------------------------------------- K4: what dqkv must not depend on
@pytest.mark.parametrize("ws", [5, 17])
def test_dqkv_bits_do_not_depend_on_dbias_calls_windows_or_a_zero_table(ws):
    c = WB.get_case(ws, "plain")
    m, W = WB.GEOM[ws]
    assert (m, W) == (2, 4)
    qkv, dout, table, kw = _case_tensors(c)
    out, lse = _fwd(qkv, kw, table)
    dqkv, dbias = _bwd(qkv, out, lse, dout, kw, table, want_dbias=True)
    d2, none = _bwd(qkv, out, lse, dout, kw, table, want_dbias=False)
    assert none is None and torch.equal(d2, dqkv)                             # with and without the bias gradient
    d3, dbias3 = _bwd(qkv, out, lse, dout, kw, table, want_dbias=True)
    assert torch.equal(d3, dqkv)                                              # two calls, the same bits
    # dbias through the partial rows and through global atomics: both within check's gate
    d4, dbias4 = _bwd(qkv, out, lse, dout, kw, table, want_dbias=True, deterministic_dbias=False)
    assert torch.equal(d4, dqkv)
    for label, db in (("scratch", dbias), ("scratch, second call", dbias3), ("atomics", dbias4)):
        bad = WB.check(c, dict(dbias=db.double().cpu()), f"dbias {label} ws={ws}", tensors=("dbias",))
        assert not bad, bad
    # a window computed alone (a 1 x 1-window map) or among the four of its 2 x 2 map
    full = _got(c, dqkv, None)
    for w in (0, 3):
        sub = {n: c[n][w:w + 1] for n in ("q", "k", "v", "dout_c")}
        q1, do1, kw1, idx1 = WB.flat_inputs(sub, ws, 1)
        q1, do1 = q1.cuda(), do1.cuda()
        o1, l1 = _fwd(q1, kw1, table)
        alone = WB.canon(idx1, 2, "tinyvit", _bwd(q1, o1, l1, do1, kw1, table)[0])
        for n in ("dq", "dk", "dv"):
            assert torch.equal(alone[n], full[n][w:w + 1]), (w, n)
    # no table against a zero table
    zero = torch.zeros_like(table)
    oz, lz = _fwd(qkv, kw, zero)
    on, ln = _fwd(qkv, kw, None)
    assert torch.equal(oz, on) and torch.equal(lz, ln)
    assert torch.equal(_bwd(qkv, oz, lz, dout, kw, zero)[0], _bwd(qkv, on, ln, dout, kw, None)[0])


# ------------------------------------------------------------------------------------------- K5: layouts, pitches, what is not written
@pytest.mark.parametrize("layout", ["tinyvit", "clip"])
@pytest.mark.parametrize("pad", [8, 4])
def test_layouts_padded_pitches_and_untouched_columns_and_rows(layout, pad):
    """Both qkv layouts with ld, ldo and lddo padded (8: 16-byte rows; 4: 8-byte rows), NaN in the pad columns of every input: the bits of the unpadded call, and
    the pad columns of dqkv and three rows behind the live tokens keep their sentinel."""
    ws = 17
    c = WB.get_case(ws, "plain")
    m, W = WB.GEOM[ws]
    qkv0, dout0, table, kw0 = _case_tensors(c)
    out0, lse0 = _fwd(qkv0, kw0, table)
    want = _got(c, _bwd(qkv0, out0, lse0, dout0, kw0, table)[0], None)
    qkv, kw, idx = WC.flat_qkv(c["q"], c["k"], c["v"], ws, m, layout, pad=pad)
    qkv = qkv.cuda()
    wide = lambda t: torch.cat([t, torch.full((t.shape[0], pad), float("nan"), dtype=BF16, device="cuda")], 1)[:, :t.shape[1]]
    out, dout = wide(out0), wide(dout0)
    tokens = qkv.shape[0]
    dbuf = torch.full((tokens + 3, 192 + pad), 7.0, dtype=BF16, device="cuda")
    dqkv, dbias = _bwd(qkv[:, :192], out, lse0, dout, kw, table, want_dbias=True, dqkv=dbuf[:tokens, :192])
    assert dqkv.data_ptr() == dbuf.data_ptr() and qkv.stride(0) == 192 + pad and out.stride(0) == 64 + pad
    got = WB.canon(idx, 2, layout, dqkv)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], want[n]), n
    assert bool((dbuf[:, 192:] == 7.0).all()) and bool((dbuf[tokens:] == 7.0).all())        # row padding and the rows behind the live tokens
    assert not bool((dbuf[:tokens, :192] == 7.0).all(0).any())                               # every dq, dk, dv column is written
    bad = WB.check(c, dict(dbias=dbias.double().cpu()), f"dbias {layout} pad {pad}", tensors=("dbias",))
    assert not bad, bad


def test_columns_outside_q_k_v_are_untouched():
    """Head stride 128 with [q | k | v | 32 foreign columns] per head: the foreign block of dqkv keeps its fill."""
    ws = 9
    c = WB.get_case(ws, "plain")
    qkv0, dout, table, kw0 = _case_tensors(c)
    out, lse = _fwd(qkv0, kw0, table)
    want = _got(c, _bwd(qkv0, out, lse, dout, kw0, table)[0], None)
    T = qkv0.shape[0]
    q4 = qkv0.view(T, 2, 3, 32)                                                # (tokens, heads, q | k | v, 32)
    qkv = torch.cat([q4, torch.full((T, 2, 1, 32), float("nan"), dtype=BF16, device="cuda")], 2).reshape(T, 256).contiguous()
    kw = dict(kw0, q_off=0, k_off=32, v_off=64, head_stride=128)
    dbuf = torch.full_like(qkv, 7.0)
    _bwd(qkv, out, lse, dout, kw, table, dqkv=dbuf)
    d4 = dbuf.view(T, 2, 4, 32)
    assert bool((d4[:, :, 3] == 7.0).all())
    got = _got(c, d4[:, :, :3].reshape(T, 192), None)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], want[n]), n


# ------------------------------------------------------------------------------------------- K7: refusals
def test_refusals_leave_the_outputs_untouched():
    from geoguessr_ai_amd import _lib as L
    from tests.test_attention16_win_bwd_cpu import REFUSALS
    lib = L.lib()
    c = WB.get_case(17, "plain")
    qkv, dout, table, kw = _case_tensors(c)
    out, lse = _fwd(qkv, kw, table)
    dqkv = torch.full_like(qkv, float("nan"))
    dbias = torch.full_like(table, float("nan"))
    aux = torch.zeros(64, device="cuda")
    ptrs = dict(qkv=qkv, out=out, dout=dout, dqkv=dqkv, lse=lse, bias_table=table)
    before = lib.gg_attention_flash16_win_bwd_calls()
    for over, dtype, msg in REFUSALS:
        a = L.AttnArgs()
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv.data_ptr(), 192, 0, 32, 64, 96, 32
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w, a.scale = 2, 4, 289, 17, 34, 34, 32 ** -0.5
        a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = out.data_ptr(), 64, lse.data_ptr(), dout.data_ptr(), 64, dqkv.data_ptr()
        if "dbias" not in over and "bias" not in over:          # a full call: the table and the gradient are given
            a.bias_table, a.dbias = table.data_ptr(), dbias.data_ptr()
        for k, v in over.items():
            if k in ("bias", "window_map", "num_windows_dev"):
                v = aux.data_ptr()
            elif k == "dbias":
                v = dbias.data_ptr()
            elif k in ptrs and v is not None:
                v = ptrs[k].data_ptr() + (2 if k in ("lse", "bias_table") else 8)
            setattr(a, k, v)
        assert lib.gg_attention_flash16_win_bwd(C.byref(a), dtype, L.stream()) != 0, (over, dtype)
        err = lib.gg_last_error().decode()
        assert err.startswith("gg_attention_flash16_win_bwd:") and msg in err, err
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv.float()).all()) and bool(torch.isnan(dbias).all()) and lib.gg_attention_flash16_win_bwd_calls() == before


# ------------------------------------------------------------------------------------------- K8: head dim 64 is unchanged
def test_head_dim_64_bits_unchanged_from_the_parent_build(golden_dir):
    """dqkv of gg_attention_flash16_bwd on the N = 17, 65, 129 ``plain`` and ``late`` cases equals, bit for bit, what the build before the kernels gained their
    D / WIN / BIAS / DBIAS template parameters gave (tests/golden/attention16_bwd_parent.npz, tests/golden/make_attention16_bwd_parent.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_attention16_bwd_parent", os.path.join(golden_dir, "make_attention16_bwd_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gold = np.load(os.path.join(golden_dir, "attention16_bwd_parent.npz"))
    got = mod.parent_bits()
    assert sorted(got) == sorted(gold.files) and len(got) == 6
    for name, x in got.items():
        assert x.dtype == gold[name].dtype and np.array_equal(x, gold[name]), name


# ------------------------------------------------------------------------------------------- the model with the switch on
@pytest.fixture(autouse=True)
def _fresh_graph_cache_and_switch():
    lib = _lib()
    lib.gg_graph_clear(); lib.gg_tinyvit_set_attention16_train(0); lib.gg_tinyvit_set_attention16(0)
    yield
    lib.gg_graph_clear(); lib.gg_tinyvit_set_attention16_train(0); lib.gg_tinyvit_set_attention16(0)


def _free(*objs):
    del objs
    gc.collect(); torch.cuda.empty_cache()


def _counters():
    lib = _lib()
    return (lib.gg_attention_flash16_win_calls(), lib.gg_attention_flash16_win_bwd_calls(), lib.gg_attention_flash16_calls(), lib.gg_attention_flash16_bwd_calls())


def _moved(n0):
    return tuple(b - a for a, b in zip(n0, _counters()))


# stage-2 blocks of tests/test_gpu_window_pad.py::MODEL_CASES
BLOCKS = {"21m384_288": 2, "21m512_320": 1}


def _reaches_stage2(trainable):
    """The backward runs stage 2's blocks when a tensor of stage 2 or below trains."""
    return any(n.startswith(("patch_embed.", "stages.0.", "stages.1.", "stages.2.")) for n in trainable)


@pytest.mark.parametrize("case_id,every", [("21m384_288", False), ("21m512_320", False), ("21m512_320", True)])
def test_padded_train_step_with_the_switch_on_meets_the_bf16_gate(centroids, monkeypatch, case_id, every):
    """M1: the bf16 training step of the 576- and the 1024-token model with the process-wide switch on through the gate tests/test_gpu_window_pad.py applies with it
    off (the bf16 bounds of _gate), the off figures printed beside; the forward counter advances by the stage-2 block count, the backward counter by the same count
    where the backward reaches stage 2 (``every``: the 1024-token case, which MODEL_CASES runs under the reference freeze policy, with every parameter trainable);
    the head-dim-64 counters stand."""
    from tests import test_gpu_window_pad as WP
    lib = _lib()
    name, img, depths, N, unfrozen = WP.MODEL_CASES[case_id]
    n0 = _counters()
    only = ("",) if every else None                                           # (every name starts with "")
    off = WP._pad_case(case_id, "bf16", centroids, monkeypatch, only_trainable=only)
    assert _moved(n0) == (0, 0, 0, 0)
    WP._gate(off, "bf16", f"bf16 {name}@{img} attention16_train off")
    WP._free(off)
    lib.gg_tinyvit_set_attention16_train(1)
    n0 = _counters()
    on = WP._pad_case(case_id, "bf16", centroids, monkeypatch, only_trainable=only)
    lib.gg_tinyvit_set_attention16_train(0)
    blocks = BLOCKS[case_id]
    assert _reaches_stage2(on["trainable"]) or not every
    assert _moved(n0) == (blocks, blocks if _reaches_stage2(on["trainable"]) else 0, 0, 0), (_moved(n0), on["trainable"][:3])
    WP._gate(on, "bf16", f"bf16 {name}@{img} attention16_train on")
    WP._free(on)


def _bb(case_id, precision="bf16", seed=11, drop_path_rate=0.1, **more):
    """The backbone of a padded case, every parameter trainable, with the inputs of one step at the C calls."""
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from tests import test_gpu_window_pad as WP
    from tests.test_gpu_precision import _randomize
    name, img, depths, _, _ = WP.MODEL_CASES[case_id]
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(name, pretrained=False, precision=precision, drop_path_rate=drop_path_rate, img_size=img, depths=depths, **more)
    _randomize(base.backbone, seed + 1)
    base = base.cuda().train()
    base.unfreeze_all()
    bb = base.backbone
    B = 2
    x = torch.randn(B, 3, img, img, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    drop = bb.make_drop_scales(B, generator=torch.Generator().manual_seed(11))
    d_out = torch.randn(B, bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    return base, bb, x, drop, d_out


def test_keyword_sets_the_switch_for_its_own_calls_only():
    """M1 (keyword): ``attention16_train=True`` on the adapter: the counters advance in the training forward and in the backward, an inference forward of the same
    backbone does not move them, and the library switch reads 0 afterwards."""
    from tests.test_gpu_recompute import _step
    lib = _lib()
    base, bb, x, drop, d_out = _bb("21m384_288", attention16_train=True)
    assert bb.attention16_train and not bb.attention16
    n0 = _counters()
    out = bb.forward_hip(x, True, drop)
    assert _moved(n0) == (2, 0, 0, 0)
    bb.backward_hip(d_out)
    torch.cuda.synchronize()
    assert _moved(n0) == (2, 2, 0, 0)
    assert lib.gg_tinyvit_set_attention16_train(0) == 0 and lib.gg_tinyvit_set_attention16(0) == 0
    n0 = _counters()
    with torch.no_grad():
        bb.forward_hip(x, False)
    assert _moved(n0) == (0, 0, 0, 0)
    assert torch.isfinite(out).all() and torch.isfinite(bb._flat_grad).all()
    _free(base, bb)


def test_four_unpadded_windows_per_image_against_the_bf16_oracle():
    """M1 (768 pixels): tiny_vit_21m_384 at 768 pixels -- stage 2 is a 48 x 48 map of four unpadded 24 x 24 windows per image -- one image, every parameter
    trainable, loss = sum(out * d_out), against autograd through the bf16-emulating oracle: embedding rel-L2 < 2e-2, every gradient tensor < 2e-1 and the median
    < 6e-2 (the bf16 bounds of tests/test_gpu_window_pad.py::_gate), structural zeros by its noise-floor rule.  Switch-off figures printed beside."""
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from oracle import tinyvit_ref as R
    from tests.test_gpu_precision import _randomize, relerr
    from tests.test_gpu_recompute import _step
    lib = _lib()
    name, img, depths = "tiny_vit_21m_384", 768, (1, 1, 1, 1)
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(name, pretrained=False, precision="bf16", drop_path_rate=0.0, img_size=img, depths=depths)
    _randomize(base.backbone, 4)
    base = base.cuda().train()
    base.unfreeze_all()
    bb = base.backbone
    assert not bb.padded_maps
    st = {k: v.detach().cpu().clone() for k, v in bb.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    x, d_out = torch.randn(1, 3, img, img, generator=g), torch.randn(1, bb.num_features, generator=g)
    cfg = R.config_for(name, drop_path_rate=0.0, img_size=img, depths=depths)
    names = [n for n, _ in bb.named_parameters()]

    def oracle(emulate):
        st_o = {k: (t.clone().requires_grad_(True) if k in names else t.clone()) for k, t in st.items()}
        emb = R.forward(cfg, st_o, x, training=True, emulate_bf16=emulate)
        (emb * d_out).sum().backward()
        return emb.detach(), {k: st_o[k].grad for k in names if st_o[k].grad is not None}
    emb_o, ref = oracle(True)
    floor = 1e-4 * float(np.median([float(t.norm()) for t in ref.values()]))
    # zero by construction (a bias in front of a conv + train-mode BatchNorm): no reference value in the bf16-emulating oracle, only its noise -- _pad_case's rule
    g32 = oracle(False)[1]
    floor32 = 1e-4 * float(np.median([float(t.norm()) for t in g32.values()]))
    zero = sorted(k for k, t in g32.items() if float(t.norm()) <= floor32)
    figs = {}
    for setting in (0, 1):
        lib.gg_tinyvit_set_attention16_train(setting)
        n0 = _counters()
        out, grad, _, _ = _step(bb, x.cuda(), None, d_out.cuda())
        assert _moved(n0) == ((1, 1, 0, 0) if setting else (0, 0, 0, 0))
        rows = []
        for t in bb.table:
            if t["kind"] != 0 or t["name"] not in ref:
                continue
            gt = grad[t["offset"]:t["offset"] + t["numel"]].view(ref[t["name"]].shape)
            if t["name"] in zero:
                noise = float(ref[t["name"]].norm())
                print(f"[21m_384@768, attention16_train {setting}] zero by construction: {t['name']} |g| {float(gt.norm()):.3e}, the oracle's noise {noise:.3e}")
                assert float(gt.norm()) <= 10 * max(noise, floor), (t["name"], float(gt.norm()), noise, floor)
            elif float(ref[t["name"]].norm()) > floor:
                rows.append((t["name"], relerr(gt, ref[t["name"]])))
        rows.sort(key=lambda r: -r[1])
        figs[setting] = (relerr(out, emb_o), rows)
        print(f"\n[21m_384@768 bf16, attention16_train {setting}] embedding rel-L2 {figs[setting][0]:.3e}, gradient rel-L2 over {len(rows)} tensors: worst {rows[0][0]} "
              f"{rows[0][1]:.3e}, median {rows[len(rows) // 2][1]:.3e}")
    lib.gg_tinyvit_set_attention16_train(0)
    e, rows = figs[1]
    assert e < 2e-2
    assert not [r for r in rows if r[1] > 2e-1], rows[:6]
    assert rows[len(rows) // 2][1] < 6e-2
    _free(base, bb)


@pytest.mark.parametrize("case_id", list(BLOCKS))
def test_recompute_gives_the_same_bits_and_replays_through_the_16_bit_forward(case_id):
    """M2: gradient checkpointing on and off with the switch on: the same bits (the attention-bias gradients, whose LDS adds land in no fixed order, to rounding:
    tests/test_gpu_recompute.py::_grad_mismatches).  Under recompute the backward re-forms the stage-2 blocks through the 16-bit forward: the forward counter moves
    again inside the backward."""
    from tests.test_gpu_recompute import _grad_mismatches, _step
    lib = _lib()
    blocks = BLOCKS[case_id]
    base, bb, x, drop, d_out = _bb(case_id)
    b0, c0 = bb._flat_buf.clone(), bb._counters.clone()
    lib.gg_tinyvit_set_attention16_train(1)
    runs = {}
    for rc in (False, True):
        bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
        bb.set_grad_checkpointing(rc)
        n0 = _counters()
        out = bb.forward_hip(x, True, drop)
        assert _moved(n0) == (blocks, 0, 0, 0)
        for p in bb._params.values():
            p.grad = None
        if bb._flat_grad is not None:
            bb._flat_grad.zero_()
        bb.backward_hip(d_out)
        torch.cuda.synchronize()
        replayed = _moved(n0)[0] - blocks
        assert _moved(n0)[1:] == (blocks, 0, 0) and (replayed > 0) == rc, (rc, _moved(n0))
        runs[rc] = (out.clone(), bb._flat_grad.clone(), bb._flat_buf.clone())
        del out
    lib.gg_tinyvit_set_attention16_train(0)
    bb.set_grad_checkpointing(False)
    assert torch.equal(runs[False][0], runs[True][0]) and torch.equal(runs[False][2], runs[True][2])
    assert float(runs[False][1].abs().sum()) > 0 and torch.isfinite(runs[False][1]).all()
    bad = _grad_mismatches(bb, runs[False][1], runs[True][1])
    assert not bad, bad[:6]
    _free(base, bb)


@pytest.mark.parametrize("fwd_on", [0, 1])
def test_switch_that_differs_between_forward_and_backward(centroids, monkeypatch, fwd_on):
    """M3: the forward under one setting and the backward under the other: not refused, each goes through the kernel the switch names when it is enqueued, and the
    step passes M1's gate."""
    from geoguessr_ai_amd.models.tinyvit import TinyVitBackbone
    from tests import test_gpu_window_pad as WP
    lib = _lib()
    case_id = "21m384_288"
    orig = TinyVitBackbone.backward_hip

    def flipped(self, *a, **k):
        lib.gg_tinyvit_set_attention16_train(1 - fwd_on)
        return orig(self, *a, **k)
    monkeypatch.setattr(TinyVitBackbone, "backward_hip", flipped)
    lib.gg_tinyvit_set_attention16_train(fwd_on)
    n0 = _counters()
    case = WP._pad_case(case_id, "bf16", centroids, monkeypatch)
    lib.gg_tinyvit_set_attention16_train(0)
    assert _moved(n0) == ((2, 0, 0, 0) if fwd_on else (0, 2, 0, 0)), _moved(n0)
    WP._gate(case, "bf16", f"bf16 {case_id} forward {'on' if fwd_on else 'off'}, backward {'off' if fwd_on else 'on'}")
    WP._free(case)


def test_frozen_attention_biases_take_no_bias_gradient():
    """M4: a trainable mask that freezes every attention_biases: the kernel is given no dbias -- the frozen ranges of the gradient buffer keep a sentinel -- and
    every other gradient is bit-identical to the all-trainable step's."""
    lib = _lib()
    base, bb, x, drop, d_out = _bb("21m384_288")
    b0, c0 = bb._flat_buf.clone(), bb._counters.clone()
    ab = [t for t in bb.table if t["kind"] == 0 and t["name"].endswith("attention_biases")]
    assert len(ab) >= 3
    lib.gg_tinyvit_set_attention16_train(1)
    runs = {}
    for frozen in (False, True):
        for n, p in bb._params.items():
            p.requires_grad_(not (frozen and n.endswith("attention_biases")))
            p.grad = None
        bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
        out = bb.forward_hip(x, True, drop)
        fg = bb.attach_grads()
        fg.zero_()
        for t in ab:
            fg[t["offset"]:t["offset"] + t["numel"]] = 7.0
        n0 = _counters()
        bb.backward_hip(d_out)
        torch.cuda.synchronize()
        assert _moved(n0)[1] == 2
        runs[frozen] = (out.clone(), bb._flat_grad.clone())
        del out
    lib.gg_tinyvit_set_attention16_train(0)
    assert torch.equal(runs[False][0], runs[True][0])
    g0, g1 = runs[False][1], runs[True][1]
    for t in bb.table:
        if t["kind"] != 0:
            continue
        a, b = g0[t["offset"]:t["offset"] + t["numel"]], g1[t["offset"]:t["offset"] + t["numel"]]
        if t["name"].endswith("attention_biases"):
            assert bool((b == 7.0).all()), t["name"]                            # untouched
            if t["name"].startswith("stages.2."):
                assert not bool((a == 7.0).all()), t["name"]                    # trainable: accumulated into
        else:
            assert torch.equal(a, b), t["name"]
    _free(base, bb)


def test_routes_the_switch_does_not_move():
    """M5: with the process switch forced to 1 an fp32 and an fp32_split step of the 576-token model, a bf16 step of a 224-pixel model (windows of at most 196
    tokens), a bf16 inference forward and a small CLIP bf16 training step equal their switch-off results bit for bit (the attention-bias gradients to rounding:
    _grad_mismatches), and both new counters stand."""
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    from tests.test_gpu_recompute import _grad_mismatches, _step
    lib = L.lib()
    keep = {}

    def tiny(precision):
        def run():
            base, bb, x, drop, d_out = _bb("21m384_288", precision=precision)
            keep[precision] = bb
            out, grad, buf, _ = _step(bb, x, drop, d_out)
            assert float(grad.abs().sum()) > 0
            return out, grad, buf
        return run

    def small():
        torch.manual_seed(2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="bf16", drop_path_rate=0.0, depths=(1, 1, 2, 1), seed=2).cuda().train()
        m.unfreeze_all()
        bb = keep["small"] = m.backbone
        xs = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
        d = torch.randn(2, bb.num_features, generator=torch.Generator().manual_seed(5)).cuda()
        out, grad, buf, _ = _step(bb, xs, None, d)
        return out, grad, buf

    def infer():
        base, bb, x, drop, d_out = _bb("21m384_288")
        base.eval()
        with torch.no_grad():
            return (bb.forward_hip(x, False).clone(),)

    def clip():
        t = CLIPVisionTower("openai/clip-vit-base-patch32", precision="bf16", num_layers=1, seed=3, hidden_size=128, intermediate_size=256, num_heads=2).cuda().train()
        xs = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
        res = t(pixel_values=xs)
        res.pooled_mean.sum().backward()
        torch.cuda.synchronize()
        return (res.last_hidden_state.detach().clone(), t.vision_model._params["encoder.layers.0.self_attn.q_proj.weight"].grad.clone())

    routes = {"fp32": tiny("fp32"), "fp32_split": tiny("fp32_split"), "small": small, "infer": infer, "clip": clip}
    runs = {}
    for setting in (0, 1):
        lib.gg_graph_clear()
        lib.gg_tinyvit_set_attention16_train(setting)
        n0 = _counters()
        for name, fn in routes.items():
            runs[(name, setting)] = fn()
        assert _moved(n0) == (0, 0, 0, 0), (setting, _moved(n0))
    lib.gg_tinyvit_set_attention16_train(0)
    for name in routes:
        a, b = runs[(name, 0)], runs[(name, 1)]
        assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]), name
        if name in ("fp32", "fp32_split", "small"):
            bad = _grad_mismatches(keep[name], a[1], b[1])
            assert not bad, (name, bad[:6])
            assert torch.equal(a[2], b[2]), name                               # running statistics
        elif name == "clip":
            assert torch.equal(a[1], b[1])
    _free(keep)


def test_switch_off_on_off_on_over_captured_graphs():
    """M6: the library switch flipped between training steps of one backbone (two images: launch-bound, the calls are captured and replayed), three steps per
    setting (eager, capture, replay; the graph keys hold the switch): every off step is the bits of a backbone that never saw the switch, the on steps agree with
    each other and differ from off; at least one graph per setting is captured and each is replayed."""
    from tests.test_gpu_recompute import _grad_mismatches, _stats, _step
    lib = _lib()
    ref_base, ref_bb, x, drop, d_out = _bb("21m384_288")
    b0, c0 = ref_bb._flat_buf.clone(), ref_bb._counters.clone()
    base_out, base_grad, _, _ = _step(ref_bb, x, drop, d_out)
    base, bb, _, _, _ = _bb("21m384_288")
    on = None
    cap0, rep0 = _stats()
    for setting in (0, 1, 0, 1):
        lib.gg_tinyvit_set_attention16_train(setting)
        for call in range(3):
            bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
            n0 = _counters()
            out, grad, _, _ = _step(bb, x, drop, d_out)
            moved = _moved(n0)
            # a replay enqueues the captured launches: the host counters stand.  The forward and the backward are graphs of their own (the forward's key holds the
            # address of its freshly allocated output), so either may run its body while the other replays
            assert moved[0] in ((0, 2) if setting else (0,)) and moved[1] in ((0, 2) if setting else (0,)) and moved[2:] == (0, 0), (setting, call, moved)
            if setting == 0:
                assert torch.equal(out, base_out), (setting, call)
                assert not _grad_mismatches(bb, base_grad, grad), (setting, call)
            else:
                on = (out, grad) if on is None else on
                assert torch.equal(out, on[0]) and not _grad_mismatches(bb, on[1], grad), (setting, call)
                assert not torch.equal(out, base_out) and not torch.equal(grad, base_grad)
    cap1, rep1 = _stats()
    lib.gg_tinyvit_set_attention16_train(0)
    print(f"\n[21m384_288 training steps] graphs captured {cap1 - cap0}, replays {rep1 - rep0}")
    assert cap1 - cap0 >= 2 and rep1 - rep0 >= 2
    _free(ref_base, ref_bb, base, bb)
