"""The fixed-order bias gradient (include/gg_attn_dbias.h) on the GPU.

Kernel level (tests/attention_dbias_cases.py has the shapes; operands, fp64 references and gates are tests/attention_cases.py's):
* against fp64 at the gate ``attention_cases.check`` applies to the tensor "dbias" of the same storage type -- every figure printed next to its gate;
* against the atomics path: the existing backward's dbias on the same inputs lies within that same gate of the new kernel's;
* three launches give ``torch.equal`` results, from a NaN-filled, a zero-filled and a finite-garbage scratch alike, and a pre-loaded dbias is accumulated into;
* ``round_bias`` on the 12 x 12 bf16 shape (gg_attention_fwd's forward adds bf16(bias / scale)); qkv as a column slice with ld > 3 C.

Step level (TinyViT-5M-224 at 8 images, every tensor trainable; one padded size; 21M-384 depths (1, 1, 2, 1) in bf16 with attention16_train): with
``deterministic_bias_grad=True`` every gradient of a step -- the attention_biases' too -- is ``torch.equal`` between two steps, between recompute off and on and
between the eager launch and the graph replay; keyword on against off every other gradient is ``torch.equal`` (dq / dk / dv do not depend on dbias) and the
attention_biases agree within the kernel gate's scale; against the fp64 oracle the attention_biases pass tests/test_gpu_masks.py's bound; a mask that freezes
every table launches nothing of the new profiler class."""
import ctypes as C
import gc
import warnings

import pytest
import torch

from tests import attention_cases as AC
from tests import attention_dbias_cases as DC

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def _fresh_graph_cache():
    from geoguessr_ai_amd import _lib as L
    L.lib().gg_graph_clear()
    yield
    L.lib().gg_graph_clear()
    assert L.lib().gg_tinyvit_set_deterministic_dbias(0) == 0, "a test left the process-wide switch on"


# ------------------------------------------------------------------------------------------- kernel level
_FWD = {}


def _forward(name, storage, cls, rounded=False):
    """The case, its device inputs and the forward's (out, lse) the kernel is given: the forward of the YARDSTICK the gate is made from -- for bf16 storage the
    fp64 formula with the documented roundings (attention_cases, "storage": P rounded before P.V, out rounded once, the bias as bf16(bias / scale) for
    ``rounded``), for f32 storage the fp64 forward rounded to f32.  The entry point's inputs include ``out``, and its bf16 rounding inside delta is most of the
    bf16 figure: on 14 x 14 bias_spike the exact fp64 backward reads 7.7e-4 of max |dbias| with bf16(exact out) and 1.1e-4 with the yardstick's out (gate
    4.5e-4), and both this kernel and the atomics path reproduce whichever they are given to 6e-7.  With the yardstick's own forward the figure measures the
    kernel's arithmetic, which is what the gate is about; the step-level tests below run on the library's forwards."""
    key = (name, storage, cls, rounded)
    if key not in _FWD:
        c = DC.case(name, storage, cls)
        qkv, dout, table = c["qkv"].cuda(), c["dout"].cuda(), c["table"].cuda()
        y = AC._yard_tensors(c, "storage", rounded) if storage == "bf16" else c["ref"]
        out = AC._flat(c, y["out"]).to(c["dtype"]).cuda()
        lse = torch.zeros(c["windows"] * c["N"], c["heads"], dtype=F32)
        lse[c["idx"].reshape(-1)] = y["lse"].permute(0, 2, 1).reshape(-1, c["heads"]).float()
        _FWD.clear()                 # one case at a time on the device
        _FWD[key] = (c, qkv, dout, table, out, lse.cuda())
    return _FWD[key]


def _geometry(c):
    return {k: v for k, v in c["kw"].items()}


def _atomics_dbias(c, qkv, dout, table, out, lse, rounded):
    from geoguessr_ai_amd import ops
    if rounded:
        return ops.attention(qkv, bias=table, dout=dout, out=out, lse=lse, want_dbias=True, **c["kw"])[1]
    return ops.attention_flash(qkv, dout=dout, out=out, lse=lse, bias_table=table, want_dbias=True, **c["kw"])[1]


def _check_kernel(name, storage, cls, rounded):
    from geoguessr_ai_amd import ops
    c, qkv, dout, table, out, lse = _forward(name, storage, cls, rounded)
    got = ops.attention_dbias(qkv, out, lse, dout, table, round_bias=rounded, **_geometry(c))
    old = _atomics_dbias(c, qkv, dout, table, out, lse, rounded)
    torch.cuda.synchronize()
    label = f"attention_dbias {name} {storage}{' rounded' if rounded else ''}"
    bad = AC.check(c, {"dbias": got}, label, rounded_bias=rounded, tensors=("dbias",))
    gate = AC.gates(c, rounded)["dbias"]["all"]
    ref = c["ref"]["dbias"]
    e_old = float((old.double().cpu() - ref).abs().max() / ref.abs().max())
    diff = float((old.double().cpu() - got.double().cpu()).abs().max() / ref.abs().max())
    print(f"[{label} {cls}] atomics path vs fp64 {e_old:.1e}; atomics path vs fixed order {diff:.1e} (gate {gate:.1e})")
    assert not bad, bad
    assert diff <= gate, (diff, gate)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name,cls", [(n, k) for n in DC.SHAPES for k in DC.CLASSES[n]])
def test_dbias_against_fp64_and_the_atomics_path(name, cls, storage):
    _check_kernel(name, storage, cls, False)


@pytest.mark.parametrize("cls", AC.classes_for(True, False))
def test_dbias_with_the_rounded_bias_of_the_resident_forward(cls):
    """12 x 12, bf16: gg_attention_fwd adds the bias as bf16(bias / scale) and the backward next to it recomputes P with that value; so does round_bias = 1."""
    _check_kernel("12x12", "bf16", cls, True)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(DC.SHAPES))
def test_dbias_is_repeatable_whatever_the_scratch_held(name, storage):
    from geoguessr_ai_amd import _lib as L, ops
    c, qkv, dout, table, out, lse = _forward(name, storage, "plain")
    geo = _geometry(c)
    a = ops.attention_dbias_args(qkv, out, lse, dout, table, **geo)
    rows = L.lib().gg_attention_dbias_rows(C.byref(a), int(storage == "f32"))
    assert rows == DC.rows(c["kw"]["num_windows"])
    n = rows * table.numel()
    first = ops.attention_dbias(qkv, out, lse, dout, table, **geo)
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0
    for k in range(2):
        assert torch.equal(first, ops.attention_dbias(qkv, out, lse, dout, table, **geo)), ("launch", k + 2)
    g = torch.Generator(device="cuda").manual_seed(1)
    fills = {"nan": torch.full((n,), float("nan"), device="cuda"), "zero": torch.zeros(n, device="cuda"),
             "garbage": 3.0e4 * torch.randn(n, device="cuda", generator=g)}
    for what, scratch in fills.items():
        assert torch.equal(first, ops.attention_dbias(qkv, out, lse, dout, table, scratch=scratch, **geo)), what
    pre = torch.randn(table.shape, device="cuda", generator=g)
    acc = ops.attention_dbias(qkv, out, lse, dout, table, dbias=pre.clone(), **geo)
    assert torch.equal(acc, pre + first), "dbias is accumulated into: pre-loaded table + the gradient, one f32 add per entry"


@pytest.mark.parametrize("storage,pad", [("f32", 4), ("bf16", 8), ("bf16", 24)])
def test_dbias_of_a_column_slice(storage, pad):
    """qkv as a column slice of a wider buffer (ld > 3 C, a column offset) and out / dout with padded rows: the bits of the contiguous call."""
    from geoguessr_ai_amd import ops
    c, qkv, dout, table, out, lse = _forward("7x7", storage, "plain")
    geo = _geometry(c)
    want = ops.attention_dbias(qkv, out, lse, dout, table, **geo)

    def wide(t, off):
        buf = torch.full((t.shape[0], t.shape[1] + off + pad), float("nan"), dtype=t.dtype, device="cuda")
        buf[:, off:off + t.shape[1]] = t
        return buf[:, off:off + t.shape[1]]
    off = 16 if storage == "bf16" else 4
    got = ops.attention_dbias(wide(qkv, off), wide(out, off), lse, wide(dout, 0), table, **geo)
    assert torch.equal(want, got)


# ------------------------------------------------------------------------------------------- step level
def _model(name, precision, deterministic, policy="all", **kw):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from tests.test_gpu_recompute import _model as base
    if not kw and not deterministic:
        return base(name, precision, policy)
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TinyViTAdapter(name, pretrained=False, precision=precision, drop_path_rate=0.1, deterministic_bias_grad=deterministic, **kw)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():        # tests/test_gpu_recompute.py's _model: away from timm's init, every gradient is non-trivial
        for n, p in m.backbone.named_parameters():
            if n.endswith(("bn.weight", "norm.weight")): p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith("attention_biases") or (n.endswith(".bias") and p.dim() == 1): p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith(".weight") and p.dim() == 2: p.copy_(0.05 * torch.randn(p.shape, generator=g))
    m = m.cuda().train()
    if policy != "all":
        from tests import masks
        masks.apply(m.backbone, policy)
    return m


def _inputs(bb, batch):
    S = bb.cfg.img_size
    x = torch.randn(batch, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    drop = bb.make_drop_scales(batch, generator=torch.Generator().manual_seed(11))
    d_out = torch.randn(batch, bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    return x, drop, d_out


def _all_equal(bb, g0, g1, what):
    """EVERY gradient bit for bit, the attention_biases included."""
    bad = [t["name"] for t in bb.table if t["kind"] == 0 and not torch.equal(g0[t["offset"]:t["offset"] + t["numel"]], g1[t["offset"]:t["offset"] + t["numel"]])]
    assert not bad, (what, bad[:6], len(bad))
    tables = [t for t in bb.table if t["kind"] == 0 and t["name"].endswith("attention_biases")]
    assert tables and all(float(g0[t["offset"]:t["offset"] + t["numel"]].abs().max()) > 0 for t in tables), what


def _release(*objs):
    del objs
    gc.collect(); torch.cuda.empty_cache()


STEP_CASES = [("tiny_vit_5m_224", "fp32", {}, 8), ("tiny_vit_5m_224", "fp32_split", {}, 8), ("tiny_vit_5m_224", "bf16", {}, 8),
              ("tiny_vit_5m_224", "fp32", dict(img_size=160), 8),          # tests/tinyvit_pad_ref.PAD_CASES[0]: 7 x 7 windows on padded 20 x 20 and 10 x 10 maps
              ("tiny_vit_21m_384", "bf16", dict(attention16_train=True, depths=(1, 1, 2, 1)), 2)]


def _kw(kw):
    if "img_size" in kw:
        from tests.tinyvit_pad_ref import PAD_CASES
        assert ("tiny_vit_5m_224", kw["img_size"], None, 8) in PAD_CASES
    return dict(kw)


@pytest.mark.parametrize("name,precision,kw,batch", STEP_CASES)
def test_step_is_bit_reproducible_with_the_keyword(name, precision, kw, batch):
    """Three steps from the same state without recompute, three with it (at launch-bound sizes the first of a key runs eagerly, the next is captured, the third
    replays): torch.equal on every gradient of all six."""
    from tests.test_gpu_recompute import _run_both
    m = _model(name, precision, True, **_kw(kw))
    bb = m.backbone
    assert bb.deterministic_bias_grad
    x, drop, d_out = _inputs(bb, batch)
    runs = _run_both(bb, x, drop, d_out, 3)
    base = runs[False][0][1]
    for rc in (False, True):
        for k, s in enumerate(runs[rc]):          # step 0 captures (or runs eagerly), steps 1, 2 replay: the same state, so the same bits
            assert torch.equal(runs[False][0][0], s[0]), (rc, k, "output")
            _all_equal(bb, base, s[1], (name, precision, "recompute" if rc else "stored", k))
    _release(m, bb, runs)


@pytest.mark.parametrize("name,precision,kw,batch", STEP_CASES)
def test_keyword_changes_only_the_bias_gradients(name, precision, kw, batch):
    """Keyword on against off from the same state: every gradient that is not an attention_biases tensor is torch.equal (dq / dk / dv do not depend on whether
    dbias was requested -- the f32 split single-pass kernel excepted, whose two instantiations differ by an ulp and whose with-dbias instantiation the switch
    therefore keeps: csrc/tinyvit.hip, attention_bwd); the attention_biases agree to 1e-5 of their largest magnitude -- the tolerance
    tests/test_gpu_recompute.py allows the atomics between two of their own runs, and the lower end of the f32 kernel gates (3e-6 .. 2.5e-5; bf16 3e-4 .. 1.3e-2).
    Measured on an MI355X: 3.9e-7 .. 4.6e-7 in all five cases."""
    from tests.test_gpu_recompute import _step
    grads = {}
    for on in (False, True):
        m = _model(name, precision, on, **_kw(kw))
        bb = m.backbone
        x, drop, d_out = _inputs(bb, batch)
        out, g, _, _ = _step(bb, x, drop, d_out)
        grads[on] = (out, g, bb.table)
        _release(m)
    assert torch.equal(grads[False][0], grads[True][0])
    worst = 0.0
    for t in grads[True][2]:
        if t["kind"] != 0:
            continue
        a, b = (grads[on][1][t["offset"]:t["offset"] + t["numel"]] for on in (False, True))
        if t["name"].endswith("attention_biases"):
            e = float((a - b).abs().max()) / float(a.abs().max())
            worst = max(worst, e)
            assert e <= 1e-5, (t["name"], e)
        else:
            assert torch.equal(a, b), t["name"]
    print(f"\n[{name} {precision} {kw}] attention_biases, keyword on vs off: worst {worst:.2e} of the tensor's largest magnitude")


def test_eager_and_graph_replay_agree_with_the_keyword():
    """The 5M-224 step at 8 images is launch-bound (it replays a captured graph): the same step with the graph path off gives the same bits."""
    import os
    from tests.test_gpu_recompute import _stats, _step
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    m = _model("tiny_vit_5m_224", "fp32", True)
    bb = m.backbone
    x, drop, d_out = _inputs(bb, 8)
    b0, c0 = bb._flat_buf.clone(), bb._counters.clone()
    cap0, rep0 = _stats()
    steps = []
    for _ in range(3):
        bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
        steps.append(_step(bb, x, drop, d_out))
    cap1, rep1 = _stats()
    assert cap1 > cap0 and rep1 > rep0, "the step was expected to take the graph path"
    env = os.environ.get("GG_GRAPH")
    assert lib.gg_graph_set_mode(0) == 0
    try:
        bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
        eager = _step(bb, x, drop, d_out)
        cap2, rep2 = _stats()
    finally:
        lib.gg_graph_set_mode(-1 if not env else int(int(env) != 0))
    assert (cap2, rep2) == (cap1, rep1), "the eager step took the graph path"
    for s in steps:
        _all_equal(bb, eager[1], s[1], "eager vs graph")
    _release(m)


def test_bias_gradients_pass_the_mask_tests_bound_against_fp64():
    """tests/test_gpu_masks.py's Case (fp32, 5M-224 at 8 images, every tensor trainable) with the keyword on: the attention_biases' rel-L2 error against the fp64
    oracle is within MASK_BOUND, the bound that file applies to every trainable tensor of every mask."""
    from tests import masks as M
    from tests import test_gpu_masks as TM
    from tests.test_gpu_precision import relerr
    c = TM.Case("tiny_vit_5m_224", 8, "fp32", torch.float64)
    c.bb.deterministic_bias_grad = True
    mask = M.apply(c.bb, "all")
    out, fg, frozen = c.pattern_step(mask)
    c.check_values("all+deterministic_bias_grad", mask, out, fg, frozen, 1e-4, 5e-4, 2e-3, bound=TM.MASK_BOUND["tiny_vit_5m_224"])
    n = 0
    for t in c.table:
        if t["name"].endswith("attention_biases"):
            e = relerr(c.bb._params[t["name"]].grad, c.grads_o[t["name"]])
            print(f"  {t['name']}: rel-L2 {e:.3e} (bound {TM.MASK_BOUND['tiny_vit_5m_224']:.1e})")
            assert e <= TM.MASK_BOUND["tiny_vit_5m_224"], (t["name"], e)
            n += 1
    assert n == sum(c.bb.depths[1:])
    _release(c)


def _dbias_launches(fn):
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    calls0 = lib.gg_attention_dbias_calls()
    lib.gg_prof_reset(); lib.gg_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.gg_prof_enable(0)
    cat, n = C.c_int(), 0
    for i in range(lib.gg_prof_count()):
        L.check(lib.gg_prof_record(i, C.byref(cat), None, None, None), "gg_prof_record")
        n += cat.value == L.PROF_CAT_ATTN_DBIAS
    lib.gg_prof_reset()
    return n, lib.gg_attention_dbias_calls() - calls0


def test_frozen_tables_launch_nothing_new():
    """Every tensor trainable: one launch of the new profiler class per block with a table.  The same mask with every attention_biases frozen: none."""
    from tests.test_gpu_recompute import _step
    m = _model("tiny_vit_5m_224", "fp32", True)
    bb = m.backbone
    x, drop, d_out = _inputs(bb, 8)
    n, calls = _dbias_launches(lambda: _step(bb, x, drop, d_out))
    assert n == calls == sum(bb.depths[1:]), (n, calls)
    for name, p in bb.named_parameters():
        if name.endswith("attention_biases"):
            p.requires_grad_(False)
    n, calls = _dbias_launches(lambda: _step(bb, x, drop, d_out))
    assert (n, calls) == (0, 0)
    _release(m)
