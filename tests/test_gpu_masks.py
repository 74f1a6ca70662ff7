"""TinyViT training under arbitrary trainable masks (tests/masks.py) on the GPU.

The mask decides the schedule of gg_tinyvit_forward / gg_tinyvit_backward (which activations are retained, which are ring temporaries, which fused
backward forms run); the rest of the suite runs two masks.  The property: the gradient of a tensor does not depend on which OTHER tensors train, so one
all-tensors backward of the CPU oracle (oracle/tinyvit_ref.py, fp64, loss (embedding * d_out).sum()) serves every mask of an input.  Per mask:

  1. values: the embedding (rel-L2 1e-4, abs 5e-4) and every trainable tensor's gradient (rel-L2 2e-3 above _grad_table's noise floor) -- and
  2. at the measured bound MASK_BOUND: 4 x the worst per-tensor error of the two trusted masks (all trainable, freeze_all_but_last_stage);
  3. frozen means untouched: frozen ranges and inter-tensor padding of the flat gradient buffer keep a bit pattern, frozen p.grad stays None;
  5. recompute on is bit-identical to recompute off;  6. mask A, then B, then A in one backbone: the third step equals the first;
  7. an AdamW step under the mask, then a forward, equals the forward of a fresh backbone loaded from the state dict;  8. the edges.
(4, workspace discipline under the mask, is tests/test_gpu_guards_model.py with the mask as its `policy`.)
The attention-bias tables' gradients are summed with float atomics in LDS: 1e-5 of their magnitude wherever the others are compared bit for bit."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import masks as M
from tests.test_gpu_precision import gemm_launches, relerr
from tests.test_gpu_recompute import _grad_mismatches, _model, _run_both, _step

pytestmark = pytest.mark.gpu

SIZES = (("tiny_vit_5m_224", 8), ("tiny_vit_21m_224", 4))       # 5M's 160-channel stage fails C % 64 == 0 of the fused chain forms, 21M passes it everywhere
DROP_PATH = 0.1
PATTERN = 0x3A83126F                                            # ~1e-3 as f32: adding any gradient to it changes its bits

# Check 2.  Worst per-tensor gradient rel-L2 error against the fp64 oracle of the two masks the project already trusts, fp32 mode, measured on an
# MI355X with this file's inputs (test_trusted_policies_stay_at_their_measured_error prints them and fails if they reach twice these):
TRUSTED_WORST = {("tiny_vit_5m_224", "all"): 6.373e-6, ("tiny_vit_5m_224", "freeze"): 5.032e-6,       # stages.1.downsample.conv1.bn.weight / patch_embed.conv1.bn.weight
                 ("tiny_vit_21m_224", "all"): 1.232e-5, ("tiny_vit_21m_224", "freeze"): 1.226e-5}     # patch_embed.conv1.bn.bias (both)
# the same under fp32_split with every split route forced (measured in the child process of test_fp32_split_masks_with_every_split_route_forced)
SPLIT_TRUSTED_WORST = {("tiny_vit_5m_224", "all"): 7.495e-6, ("tiny_vit_5m_224", "freeze"): 5.446e-6,      # patch_embed.conv2.bn.bias / patch_embed.conv1.bn.weight
                       ("tiny_vit_21m_224", "all"): 9.790e-6, ("tiny_vit_21m_224", "freeze"): 9.368e-6}    # stages.1.blocks.0.mlp.norm.weight / stages.3.blocks.0.attn.attention_biases
# tensors whose EXACT gradient is zero (below 1e-4 of the median gradient norm in the fp64 oracle): the Case asserts this list
EXACT_ZERO = {"tiny_vit_5m_224": (), "tiny_vit_21m_224": ("stages.2.blocks.5.mlp.fc2.bias",)}    # the last fc2.bias of a stage: a constant in front of a conv + BatchNorm
# every other mask: 4 x the larger of the two (route changes between f32-MFMA forms whose accumulation order differs); never derived from the masks under test
MASK_BOUND = {name: 4 * max(TRUSTED_WORST[name, "all"], TRUSTED_WORST[name, "freeze"]) for name, _ in SIZES}
SPLIT_MASK_BOUND = {name: 4 * max(SPLIT_TRUSTED_WORST[name, "all"], SPLIT_TRUSTED_WORST[name, "freeze"]) for name, _ in SIZES}


@pytest.fixture(autouse=True)
def _fresh_graph_cache():
    from geoguessr_ai_amd import _lib as L
    L.lib().gg_graph_clear()
    yield
    L.lib().gg_graph_clear()


def _inputs(bb, batch):
    """Input, injected DropPath scales (keep / (1 - rate), as the oracle forms them from the keep masks) and a random output gradient."""
    g = torch.Generator().manual_seed(5)
    S = bb.cfg.img_size
    x = torch.randn(batch, 3, S, S, generator=g)
    d_out = torch.randn(batch, bb.num_features, generator=g)
    keep = torch.rand(bb.num_drop_slots, batch, generator=g) > 0.3
    for slot in range(bb.num_drop_slots):          # a slot that drops every sample would take its whole branch out of the gradient: keep one
        if not bool(keep[slot].any()):
            keep[slot, slot % batch] = True
    rates = torch.tensor(bb.drop_rates).unsqueeze(1)
    assert float(rates.max()) > 0
    scales = (keep.float() / (1 - rates)).contiguous()
    return x, d_out, keep, scales


def _oracle(name, bb, x, d_out, keep, dtype, emulate_bf16=False):
    """One forward + backward of the CPU oracle with EVERY tensor requiring grad: embedding and the gradient of each parameter tensor."""
    from oracle import tinyvit_ref as R
    cfg = R.config_for(name, drop_path_rate=DROP_PATH)
    st = {}
    for k, v in bb.state_dict().items():
        v = v.detach().cpu().clone()
        st[k] = v.to(dtype).requires_grad_(True) if k in bb._params else (v.to(dtype) if v.is_floating_point() else v)
    emb = R.forward(cfg, st, x.to(dtype), training=True, emulate_bf16=emulate_bf16, drop_masks=[keep[s] for s in range(keep.shape[0])])
    (emb * d_out.to(dtype)).sum().backward()
    grads = {k: st[k].grad.detach() for k in bb._params}
    assert all(g is not None for g in grads.values())
    return emb.detach(), grads


class Case:
    def __init__(self, name, batch, precision, oracle_dtype):
        self.name, self.batch, self.precision = name, batch, precision
        self.m = _model(name, precision, "all", drop_path_rate=DROP_PATH)
        self.bb = bb = self.m.backbone
        x, d_out, keep, scales = _inputs(bb, batch)
        self.emb_o, self.grads_o = _oracle(name, bb, x, d_out, keep, oracle_dtype, emulate_bf16=precision == "bf16")
        self.floor = 1e-4 * float(np.median([float(g.norm()) for g in self.grads_o.values()]))        # _grad_table's noise floor
        # A parameter whose effect is cancelled downstream (a bias in front of a conv + BatchNorm: the last fc2.bias of a stage) has an EXACT gradient of
        # zero.  Which tensors those are is decided by the exact (fp64) oracle; the bf16-emulating oracle holds its own rounding noise there (above the
        # floor: 1.5 rel-L2 against the library's noise), which is not a reference for anything
        exact = self.grads_o if oracle_dtype == torch.float64 else _oracle(name, bb, x, d_out, keep, torch.float64)[1]
        floor64 = 1e-4 * float(np.median([float(g.norm()) for g in exact.values()]))
        self.comparable = {n: float(g.norm()) > floor64 for n, g in exact.items()}
        # how many tensors the exact-zero branch may take, pinned per size (fp64, these inputs): none of 5M's 213, one of 21M's
        quiet = sorted(n for n, ok in self.comparable.items() if not ok)
        assert len(self.comparable) == 213 and quiet == sorted(EXACT_ZERO[name]), (name, quiet)
        self.x, self.d_out, self.drop = x.cuda(), d_out.cuda(), scales.cuda()
        self.b0, self.c0 = bb._flat_buf.clone(), bb._counters.clone()
        self.table = [t for t in bb.table if t["kind"] == 0]

    def reset(self):
        self.bb._flat_buf.copy_(self.b0); self.bb._counters.copy_(self.c0)

    def frozen_index(self, mask):
        """Bool over the flat gradient floats: True outside every trainable tensor (frozen tensors and the padding between tensors)."""
        idx = torch.ones(self.bb.param_floats, dtype=torch.bool, device="cuda")
        for t in self.table:
            if t["name"] in mask:
                idx[t["offset"]:t["offset"] + t["numel"]] = False
        return idx

    def pattern_step(self, mask):
        """One training step with the flat gradient buffer prepared as gg_tinyvit_backward's contract has it: trainable ranges zero (it accumulates),
        everything else a non-zero bit pattern.  Returns (embedding, flat gradient, frozen index)."""
        bb = self.bb
        self.reset()
        for p in bb._params.values():
            p.grad = None
        fg = bb.attach_grads()
        fg.zero_()
        frozen = self.frozen_index(mask)
        fg.view(torch.int32)[frozen] = PATTERN
        out = bb.forward_hip(self.x, True, self.drop)
        bb.backward_hip(self.d_out)
        torch.cuda.synchronize()
        return out.clone(), fg, frozen

    def check_values(self, key, mask, out, fg, frozen, tol_emb_rel, tol_emb_abs, tol_grad, bound=None):
        bb = self.bb
        emb = out.detach().cpu().to(self.emb_o.dtype)
        e_rel, e_abs = relerr(emb, self.emb_o), float((emb - self.emb_o).abs().max())
        rows, quiet = [], 0
        for t in self.table:
            n = t["name"]
            p = bb._params[n]
            if n not in mask:
                assert p.grad is None, (key, n, "frozen, but has a .grad")
                continue
            assert p.grad is not None and p.grad.data_ptr() == fg.data_ptr() + 4 * t["offset"], (key, n)
            gref = self.grads_o[n]
            if self.comparable[n]:
                rows.append((relerr(p.grad, gref), n))
            else:                      # exact gradient zero: rounding noise on both sides, of the reference's own size at most
                quiet += 1
                assert float(p.grad.norm()) < 10 * max(self.floor, float(gref.norm())), (key, n, float(p.grad.norm()), self.floor, float(gref.norm()))
        assert len(rows) + quiet == len(mask) and quiet == len(set(mask) & set(EXACT_ZERO[self.name])), (key, len(rows), quiet, len(mask))   # no tensor left out
        assert rows, (key, "no trainable tensor of this mask has a gradient to compare")
        rows.sort(reverse=True)
        print(f"\n[{self.precision} {self.name} B={self.batch} mask {key}] embedding rel-L2 {e_rel:.3e} max|err| {e_abs:.3e}; {len(rows)} of {len(mask)} "
              f"trainable gradients compared: worst {rows[0][1]} {rows[0][0]:.3e}, median {rows[len(rows) // 2][0]:.3e}"
              + (f" (bound {bound:.1e})" if bound else ""))
        assert torch.isfinite(out).all()
        assert e_rel < tol_emb_rel and (tol_emb_abs is None or e_abs < tol_emb_abs), (key, e_rel, e_abs)
        bad = [r for r in rows if r[0] > tol_grad]
        assert not bad, (key, bad[:8])
        # frozen means untouched (3)
        iv = fg.view(torch.int32)
        touched = (iv[frozen] != PATTERN)
        if bool(touched.any()):
            where = torch.nonzero(frozen)[touched][:, 0]
            names = sorted({t["name"] for t in self.table for w in where[:64].tolist() if t["offset"] <= w < t["offset"] + (t["numel"] + 7) // 8 * 8})
            raise AssertionError((key, "frozen gradient ranges / padding written", int(touched.sum()), names[:6]))
        if bound is not None:
            bad = [r for r in rows if r[0] > bound]
            assert not bad, (key, "above 4 x the trusted masks' worst error", bound, bad[:8])
        return rows[0][0]


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _cases_of_this_module():
    """The models, oracles and workspaces the tests of this file share (one per size and mode) are released when the module is done."""
    yield
    from geoguessr_ai_amd import _lib as L
    L.lib().gg_graph_clear()
    _CASES.clear(); _CLIP.clear()
    gc.collect(); torch.cuda.empty_cache()


def _case(name, batch, precision="fp32"):
    key = (name, batch, precision)
    if key not in _CASES:                  # (kept for the module: the fp64 oracle of a case takes seconds, the models are small)
        _CASES[key] = Case(name, batch, precision, torch.float64 if precision != "bf16" else torch.float32)
    return _CASES[key]


# ------------------------------------------------------------------------------------------- fp32: checks 1, 2, 3
@pytest.mark.parametrize("policy", ["all", "freeze"])
@pytest.mark.parametrize("name,batch", SIZES)
def test_trusted_policies_stay_at_their_measured_error(name, batch, policy):
    """The two masks the rest of the suite runs: their worst per-tensor error against fp64 is where MASK_BOUND comes from."""
    c = _case(name, batch)
    mask = M.apply(c.bb, policy)
    out, fg, frozen = c.pattern_step(mask)
    worst = c.check_values(policy, mask, out, fg, frozen, 1e-4, 5e-4, 2e-3)
    assert worst <= 2 * TRUSTED_WORST[name, policy], (name, policy, worst)          # the recorded figures still describe the code


@pytest.mark.parametrize("key", M.FAMILY_NAMES)
@pytest.mark.parametrize("name,batch", SIZES)
def test_masked_step_matches_the_all_tensors_oracle(name, batch, key):
    c = _case(name, batch)
    mask = M.apply(c.bb, key)
    out, fg, frozen = c.pattern_step(mask)
    c.check_values(key, mask, out, fg, frozen, 1e-4, 5e-4, 2e-3, bound=MASK_BOUND[name])


# ------------------------------------------------------------------------------------------- 5: recompute under the mask
def _assert_same_steps(bb, a, b, what):
    for k, (s0, s1) in enumerate(zip(a, b)):
        assert torch.isfinite(s0[0]).all()
        assert torch.equal(s0[0], s1[0]), (what, k, "output")
        bad = _grad_mismatches(bb, s0[1], s1[1])
        assert not bad, (what, k, bad[:6], len(bad))
        assert torch.equal(s0[2], s1[2]) and torch.equal(s0[3], s1[3]), (what, k, "running statistics / counters")


@pytest.mark.parametrize("key", M.FAMILY_NAMES)
@pytest.mark.parametrize("name,batch", SIZES)
def test_recompute_is_bit_identical_under_the_mask(name, batch, key):
    c = _case(name, batch)
    M.apply(c.bb, key)
    c.reset()
    runs = _run_both(c.bb, c.x, c.drop, c.d_out, 2)
    assert float(runs[False][0][1].abs().sum()) > 0
    _assert_same_steps(c.bb, runs[False], runs[True], key)


# ------------------------------------------------------------------------------------------- 6: switching masks in one backbone
SWITCH = [("norms", "matrices"), ("matrices", "norms"), ("head_norm_only", "stage1_only"), ("random[0]", "random[1]"), ("mbconv_c2", "mbconv_c3_bn")]


def _switch_steps(c, a, b):
    """Two steps per visit: the second of a visit runs from the graph the first captured, and A's last visit finds A's graphs, captured before B ran."""
    bb, res = c.bb, []
    for key in (a, b, a):
        M.apply(bb, key)
        visit = []
        for _ in range(2):
            c.reset()
            visit.append(_step(bb, c.x, c.drop, c.d_out))
        res.append(visit)
    return res


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,batch", SIZES)
def test_switching_masks_in_one_backbone(name, batch, precision):
    """A, then B, then A in the same object with the same input addresses: a stale captured graph, a stale workspace plan or stale temporaries would
    make the third step differ from the first."""
    from geoguessr_ai_amd import _lib as L
    c = _case(name, batch, precision)
    larger = smaller = 0
    for a, b in SWITCH:
        size = {k: L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(c.bb.cfg), batch, 1, M.to_bytes(c.bb.table, M.mask_of(c.bb.table, k))) for k in (a, b)}
        larger += size[a] > size[b]; smaller += size[a] < size[b]
        c.bb._ws.clear()
        s1, s2, s3 = _switch_steps(c, a, b)
        assert not torch.equal(s1[0][1], s2[0][1])                    # B's gradients are other tensors'
        _assert_same_steps(c.bb, s1, s3, (a, b))
        _assert_same_steps(c.bb, [s1[0], s2[0]], [s1[1], s2[1]], (a, b, "second step of a visit"))
    assert larger and smaller, (larger, smaller)


# ------------------------------------------------------------------------------------------- 7: optimizer step under the mask
@pytest.mark.parametrize("key", ["norms", "mlp", "random[3]"])
@pytest.mark.parametrize("name,batch", SIZES)
def test_optimizer_step_under_the_mask_refreshes_what_it_changed(name, batch, key):
    """optim.AdamW moves the mask's tensors and marks only them dirty (gg_tinyvit_refresh_weights_masked): the next forward must equal that of a fresh
    backbone loaded from the resulting state dict (full refresh) -- for masks whose changed tensors are not the freeze policy's 14 matrices."""
    from geoguessr_ai_amd.optim import AdamW
    c = _case(name, batch)
    m = _model(name, "fp32", key, drop_path_rate=DROP_PATH)
    bb = m.backbone
    mask = M.mask_of(bb.table, key)
    before = {n: p.detach().clone() for n, p in bb._params.items()}
    opt = AdamW(m, lr=1e-2)
    _step(bb, c.x, c.drop, c.d_out)
    opt.step()
    torch.cuda.synchronize()
    for n, p in bb._params.items():
        assert torch.equal(p.detach(), before[n]) == (n not in mask), n                 # exactly the mask's tensors moved
    out_t = bb.forward_hip(c.x, True, c.drop).clone()
    state = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    out_e = bb.forward_hip(c.x, False).clone()
    fresh = _model(name, "fp32", key, drop_path_rate=DROP_PATH, seed=1)
    fb = fresh.backbone
    fb.load_state_dict(state)
    ref_t = fb.forward_hip(c.x, True, c.drop).clone()
    fb.load_state_dict(state)
    ref_e = fb.forward_hip(c.x, False).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(out_t).all() and torch.equal(out_t, ref_t), (key, float((out_t - ref_t).abs().max()))
    assert torch.equal(out_e, ref_e), (key, float((out_e - ref_e).abs().max()))
    del m, fresh, bb, fb, opt
    gc.collect(); torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- 8: edges
def test_all_frozen_mask_returns_ok_and_writes_no_gradient_byte():
    """include/gg.h: a mask of all zeros is accepted; gg_tinyvit_backward returns 0 and changes no byte of `grads`."""
    c = _case(*SIZES[0])
    mask = M.apply(c.bb, frozenset())
    out, fg, frozen = c.pattern_step(mask)
    assert bool(frozen.all()) and torch.isfinite(out).all()
    assert bool((fg.view(torch.int32) == PATTERN).all())
    assert all(p.grad is None for p in c.bb._params.values())
    assert relerr(out.cpu().double(), c.emb_o) < 1e-4


@pytest.mark.parametrize("a,b", [("norms", "mlp"), ("random[4]", "random[5]")])
def test_mask_change_between_forward_and_backward_stays_refused(a, b):
    from geoguessr_ai_amd import _lib as L
    c = _case(*SIZES[0])
    M.apply(c.bb, a)
    c.reset()
    c.bb.forward_hip(c.x, True, c.drop)
    M.apply(c.bb, b)
    with pytest.raises(L.GgError, match="requires_grad changed between forward and backward"):
        c.bb.backward_hip(c.d_out)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- bf16: values at the bf16 gate, 3, 5, 6 exact
@pytest.mark.parametrize("key", M.REDUCED)
@pytest.mark.parametrize("name,batch", SIZES)
def test_bf16_masked_step(name, batch, key):
    c = _case(name, batch, "bf16")
    mask = M.apply(c.bb, key)
    out, fg, frozen = c.pattern_step(mask)
    c.check_values(key, mask, out, fg, frozen, 2e-2, None, 0.2)
    c.reset()
    runs = _run_both(c.bb, c.x, c.drop, c.d_out, 2)
    _assert_same_steps(c.bb, runs[False], runs[True], key)


# ------------------------------------------------------------------------------------------- fp32_split with every split route forced (child process)
def _block_linear_weights(mask):
    return [n for n in mask if n.endswith((".attn.qkv.weight", ".attn.proj.weight", ".mlp.fc1.weight", ".mlp.fc2.weight"))]


def _split_child():
    """Runs in a child under GG_DEV_SWITCHES=1 GG_SPLIT_MIN_TILES=1 GG_SPLIT_TN_MIN_M=1 (the switches are read once per process): the two trusted masks
    (where SPLIT_MASK_BOUND comes from), then checks 1-3 on the reduced family, and the split weight-gradient launches: one per trained block Linear,
    none for a frozen one."""
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    linear = (".attn.qkv", ".attn.proj", ".mlp.fc1", ".mlp.fc2")
    for name, batch in SIZES:
        c = _case(name, batch, "fp32_split")
        every = frozenset(n for n in c.bb._params if n.rsplit(".", 1)[0].endswith(linear))
        for policy in ("all", "freeze"):
            L.lib().gg_graph_clear()
            mask = M.apply(c.bb, policy)
            out, fg, frozen = c.pattern_step(mask)
            worst = c.check_values(policy, mask, out, fg, frozen, 1e-4, 5e-4, 2e-3)
            print(f"[fp32_split forced {name} trusted mask {policy}] worst {worst:.3e} (recorded {SPLIT_TRUSTED_WORST[name, policy]:.3e})")
            assert worst <= 2 * SPLIT_TRUSTED_WORST[name, policy], (name, policy, worst)
        for key in M.REDUCED:
            L.lib().gg_graph_clear()
            mask = M.apply(c.bb, key)
            with gemm_launches() as la:
                out, fg, frozen = c.pattern_step(mask)
            c.check_values(key, mask, out, fg, frozen, 1e-4, 5e-4, 2e-3, bound=SPLIT_MASK_BOUND[name])
            lin = _block_linear_weights(mask)
            # the mask without its block Linears, and with EVERY block Linear: nothing else of the schedule depends on them, so the three steps differ by
            # the split weight-gradient launches alone -- one per trained Linear, none for a frozen one (a launch for a frozen Linear in `rest`
            # would make the step with every Linear gain fewer than all of them)
            rest, plus = frozenset(mask - every), frozenset(mask | every)
            counts = {}
            for tag, other in (("rest", rest), ("plus", plus)):
                L.lib().gg_graph_clear()
                M.apply(c.bb, other)
                with gemm_launches() as lo:
                    c.pattern_step(other)
                counts[tag] = lo.split
            n_all = len(_block_linear_weights(every))
            print(f"[fp32_split forced {name} mask {key}] split launches {la.split} (f32-MFMA {la.plain}); without its {len(lin)} block Linears {counts['rest']}; "
                  f"with all {n_all}: {counts['plus']}")
            assert la.split > 0 and la.split - counts["rest"] == len(lin) and counts["plus"] - counts["rest"] == n_all, (key, la.split, counts, len(lin), n_all)
            print(f"{name} {key} -> ok")
    L.lib().gg_graph_clear()


def test_fp32_split_masks_with_every_split_route_forced():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GG_DEV_SWITCHES="1", GG_SPLIT_MIN_TILES="1", GG_SPLIT_TN_MIN_M="1")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_masks"], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    print(r.stdout[-12000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("-> ok") == len(SIZES) * len(M.REDUCED)


# ------------------------------------------------------------------------------------------- CLIP vision tower (csrc/clip.hip)
# The tiny tower of tests/golden/clip_tiny.npz, fp32, loss (pooled mean * d_out).sum(), against ONE all-tensors fp64 backward of oracle/clip_ref.py.
# clip.hip takes any mask, half pairs included (its LayerNorm backward sends the frozen half's sums to a dump row).  Tolerances: those of
# test_superguessr_on_clip_training_matches_reference_golden (embedding and every gradient rel-L2 1e-4; k_proj.bias, whose exact gradient is zero,
# relative to the q_proj.bias gradient of its layer, as tests/clip_golden.py does).  No atomics in this path: every comparison between runs is bit for bit.
CLIP_KEYS = ("biases", "layernorms", "middle_layer", "position_embedding", "class_embedding", "patch_embedding", "layernorm_weights",
             "random[0]", "random[1]", "random[2]")
# worst per-tensor gradient error of the two trusted policies against fp64 (MI355X, these inputs); every mask is asserted at 4 x the larger
CLIP_TRUSTED_WORST = {"all_layers": 7.437e-7, "last_layer": 6.850e-7}       # encoder.layers.0 / .1 self_attn.q_proj.weight
CLIP_MASK_BOUND = 4 * max(CLIP_TRUSTED_WORST.values())
_CLIP = {}


class ClipCase:
    def __init__(self, golden_dir):
        from oracle import clip_ref as CR
        from tests import clip_golden as CG
        from tests.test_gpu_clip import _tiny_tower
        case = CG.load(golden_dir)
        self.tower = _tiny_tower(case, "fp32").cuda().train()
        self.vm = vm = self.tower.vision_model
        self.nl = case["cfg"][2]
        x = torch.from_numpy(np.load(os.path.join(golden_dir, "clip_tiny.npz"))["x"])
        d_out = torch.randn(x.shape[0], case["cfg"][0], generator=torch.Generator().manual_seed(9))
        st = {n: p.detach().cpu().double().requires_grad_(True) for n, p in vm._params.items()}
        emb = CR.forward(CR.ClipVisionConfig(*case["cfg"]), st, x.double())
        (emb * d_out.double()).sum().backward()
        self.emb_o = emb.detach()
        self.grads_o = {n: (t.grad if t.grad is not None else torch.zeros_like(t)) for n, t in st.items()}
        off_path = [n for n, t in st.items() if t.grad is None]
        assert off_path and all(n.startswith("post_layernorm") for n in off_path), off_path
        self.x, self.d_out = x.cuda(), d_out.cuda()
        self.table = list(vm.table)
        names = [t["name"] for t in self.table]
        self.masks = dict(M.clip_family(names, self.nl), all_layers=frozenset(names),
                          last_layer=frozenset(n for n in names if not (n.startswith("encoder.layers.") and int(n.split(".")[2]) < self.nl - 1)))

    def step(self, mask, pattern=True):
        vm = self.vm
        for p in vm._params.values():
            p.grad = None
        fg = vm.attach_grads()
        fg.zero_()
        frozen = torch.ones(vm.param_floats, dtype=torch.bool, device="cuda")
        for t in self.table:
            if t["name"] in mask:
                frozen[t["offset"]:t["offset"] + t["numel"]] = False
        if pattern:
            fg.view(torch.int32)[frozen] = PATTERN
        out, _ = self.tower.forward_hip(self.x, True, False)
        self.tower.backward_hip(self.d_out, None, vm._gen)
        torch.cuda.synchronize()
        return out.clone(), fg, frozen

    def check(self, key, mask, out, fg, frozen, bound=None):
        e_rel = relerr(out, self.emb_o)
        rows = []
        for t in self.table:
            n = t["name"]
            p = self.vm._params[n]
            if n not in mask:
                assert p.grad is None, (key, n)
                continue
            assert p.grad is not None and p.grad.data_ptr() == fg.data_ptr() + 4 * t["offset"], (key, n)
            g, ref = p.grad.detach().cpu().double(), self.grads_o[n]
            if n.startswith("post_layernorm"):                       # not on the path: exactly zero
                assert float(g.abs().max()) == 0.0, (key, n)
                continue
            floor = float(self.grads_o[n.replace("k_proj", "q_proj")].norm()) if n.endswith("k_proj.bias") else 0.0
            rows.append((float((g - ref).norm() / (ref.norm() + floor + 1e-300)), n))
        assert len(rows) == len([n for n in mask if not n.startswith("post_layernorm")]) and rows, (key, len(rows))
        rows.sort(reverse=True)
        print(f"\n[CLIP tiny fp32 mask {key}] pooled rel-L2 {e_rel:.3e}; {len(rows)} trainable gradients: worst {rows[0][1]} {rows[0][0]:.3e}, "
              f"median {rows[len(rows) // 2][0]:.3e}" + (f" (bound {bound:.1e})" if bound else ""))
        assert torch.isfinite(out).all() and e_rel < 1e-4, (key, e_rel)
        assert rows[0][0] < 1e-4, (key, rows[:6])
        assert bool((fg.view(torch.int32)[frozen] == PATTERN).all()), (key, "frozen gradient ranges / padding written")
        if bound is not None:
            assert rows[0][0] <= bound, (key, "above 4 x the trusted policies' worst error", bound, rows[:6])
        return rows[0][0]


def _clip_case(golden_dir):
    if "case" not in _CLIP:
        _CLIP["case"] = ClipCase(golden_dir)
    return _CLIP["case"]


@pytest.mark.parametrize("policy", ["all_layers", "last_layer"])
def test_clip_trusted_policies_stay_at_their_measured_error(golden_dir, policy):
    c = _clip_case(golden_dir)
    mask = M.apply(c.vm, c.masks[policy])
    worst = c.check(policy, mask, *c.step(mask))
    assert worst <= 2 * CLIP_TRUSTED_WORST[policy], (policy, worst)


@pytest.mark.parametrize("key", CLIP_KEYS)
def test_clip_masked_step_matches_the_all_tensors_oracle(golden_dir, key):
    c = _clip_case(golden_dir)
    assert set(CLIP_KEYS) == set(c.masks) - {"all_layers", "last_layer"}
    mask = M.apply(c.vm, c.masks[key])
    c.check(key, mask, *c.step(mask), bound=CLIP_MASK_BOUND)


def test_clip_switching_masks_in_one_tower(golden_dir):
    """A, B, A in one tower, two steps per visit, workspace larger and smaller: the last visit equals the first bit for bit."""
    from geoguessr_ai_amd import _lib as L
    c = _clip_case(golden_dir)
    larger = smaller = 0
    for a, b in (("middle_layer", "class_embedding"), ("class_embedding", "middle_layer"), ("layernorm_weights", "biases"), ("random[0]", "random[1]")):
        size = {k: L.lib().gg_clip_workspace_bytes(C.byref(c.tower.cfg), c.x.shape[0], 1, bytes(int(t["name"] in c.masks[k]) for t in c.table)) for k in (a, b)}
        larger += size[a] > size[b]; smaller += size[a] < size[b]
        c.vm._ws.clear()
        visits = []
        for key in (a, b, a):
            mask = M.apply(c.vm, c.masks[key])
            visits.append([tuple(t.clone() for t in c.step(mask, pattern=False)[:2]) for _ in range(2)])
        assert not torch.equal(visits[0][0][1], visits[1][0][1])
        for first, last in zip(visits[0] + [visits[0][0]], visits[2] + [visits[0][1]]):
            assert torch.equal(first[0], last[0]) and torch.equal(first[1], last[1]), (a, b)
    assert larger and smaller, (larger, smaller)


if __name__ == "__main__":
    _split_child()
