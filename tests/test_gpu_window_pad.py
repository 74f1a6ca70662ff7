"""Padded attention windows on the GPU (include/gg_pad.h, csrc/window_pad.hip; the padded TinyVitBlock of csrc/tinyvit.hip): TinyViT at an input size whose stage maps
the attention window does not divide.

* gg_window_pad / gg_window_crop_add against torch indexing, bit for bit, f32 and bf16 storage; LayerNorm on the all-zero rows the padding creates;
* one training step of four padded models (SuperGuessr head on top, DropPath masks injected) in the three arithmetic modes against the oracle with the padded block
  of tests/tinyvit_pad_ref.py swapped in: fp32 and fp32_split at the fp32 gate of tests/test_gpu_precision.py (_fp32_gate: per-stage taps 2e-4, embedding 1e-4 rel /
  5e-4 abs, loss 1e-5, every gradient tensor 2e-3 with its noise floor), bf16 at the bounds of test_bf16_mode_train_step_matches_bf16_emulating_oracle;
* recompute on / off, a step after the workspace was overwritten with NaN bytes, and a graph replay: bit-identical; a trainable mask; the eval surfaces;
* a native-size step launches no pad / crop kernel (the launch profiler's category GG_CAT_PAD)."""
import ctypes as C
import gc
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tinyvit_pad_ref as P

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as o
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return o


@pytest.fixture(autouse=True)
def _fresh_graph_cache():
    from geoguessr_ai_amd import _lib as L
    L.lib().gg_graph_clear()
    yield
    L.lib().gg_graph_clear()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Cc", [64, 160, 576])
@pytest.mark.parametrize("H,Hp", [(5, 7), (10, 14), (20, 21), (20, 32)])
def test_window_pad_and_crop_add_are_exact(ops, dtype, Cc, H, Hp):
    """y = pad(x) with the output pre-filled with NaN (every byte must be overwritten), and y = res + rowscale[b] * crop(t) for res / rowscale present and null and
    y aliasing res: equal to torch indexing bit for bit (f32 arithmetic, product and sum rounded separately, one rounding to the storage type)."""
    from geoguessr_ai_amd import _lib as L
    for B in (1, 3):
        g = torch.Generator().manual_seed(100 * B + H + Cc)
        x = torch.randn(B, H, H, Cc, generator=g).to(dtype).cuda()
        want = torch.zeros(B, Hp, Hp, Cc, dtype=dtype, device="cuda")
        want[:, :H, :H] = x
        y = torch.full((B, Hp, Hp, Cc), float("nan"), dtype=dtype, device="cuda")
        L.check(L.lib().gg_window_pad(L.ptr(x), L.ptr(y), B, H, H, Hp, Hp, Cc, int(dtype == F32), L.stream()), "gg_window_pad")
        assert torch.equal(_bits(y), _bits(want)), (B, "pad")
        assert torch.equal(_bits(ops.window_pad(x, Hp, Hp)), _bits(want))
        t = torch.randn(B, Hp, Hp, Cc, generator=g).to(dtype).cuda()
        res = torch.randn(B, H, H, Cc, generator=g).to(dtype).cuda()
        rs = torch.tensor([1.25, 0.0, 1.0 / 0.9][:B], dtype=F32, device="cuda")
        crop = t[:, :H, :H].float()
        for has_res in (True, False):
            for has_rs in (True, False):
                ref = crop * rs[:, None, None, None] if has_rs else crop
                if has_res:
                    ref = res.float() + ref
                ref = ref.to(dtype)
                got = ops.window_crop_add(t, H, H, res=res if has_res else None, rowscale=rs if has_rs else None)
                assert torch.equal(_bits(got), _bits(ref)), (B, has_res, has_rs)
        buf = res.clone()                                  # y aliasing res
        out = ops.window_crop_add(t, H, H, res=buf, rowscale=rs, out=buf)
        assert out.data_ptr() == buf.data_ptr() and torch.equal(_bits(buf), _bits((res.float() + crop * rs[:, None, None, None]).to(dtype)))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Cc", [64, 160, 576])
def test_layernorm_on_zero_rows(ops, dtype, Cc):
    """What a pad token is to attn.norm: an all-zero row leaves gg_layernorm_fwd as norm.bias rounded to the storage type, bit for bit (mean 0, variance 0: the
    normalised row is exactly zero), and gg_layernorm_bwd on such rows is finite and adds their dy to d beta."""
    M, Z = 37, (3, 4, 20, 36)                               # zero rows among ordinary ones, the last row included
    g = torch.Generator().manual_seed(Cc)
    x = torch.randn(M, Cc, generator=g).to(dtype)
    x[list(Z)] = 0
    gamma, beta = 1 + 0.2 * torch.randn(Cc, generator=g), 0.3 * torch.randn(Cc, generator=g)
    out, mean, rstd = ops.layernorm_fwd(x.cuda(), gamma.cuda(), beta.cuda())
    torch.cuda.synchronize()
    for r in Z:
        assert torch.equal(_bits(out[r]), _bits(beta.to(dtype).cuda())), r
        assert float(mean[r]) == 0.0 and np.isfinite(float(rstd[r]))
    dy = torch.randn(M, Cc, generator=g).to(dtype)
    dx, dg, db = ops.layernorm_bwd(dy.cuda(), x.cuda(), mean, rstd, gamma.cuda())
    assert torch.isfinite(dx.float()).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()
    want_db = dy.double().sum(0)
    assert float((db.cpu().double() - want_db).abs().max()) <= 1e-5 * float(want_db.abs().max())
    only_zero = dy.clone()
    only_zero[[r for r in range(M) if r not in Z]] = 0      # dy on the zero rows alone: d beta is their sum, d gamma gets nothing (x_hat = 0 there)
    _, dg0, db0 = ops.layernorm_bwd(only_zero.cuda(), x.cuda(), mean, rstd, gamma.cuda())
    want0 = dy[list(Z)].double().sum(0)
    assert float((db0.cpu().double() - want0).abs().max()) <= 1e-5 * float(want0.abs().max()) and float(want0.abs().max()) > 0
    assert float(dg0.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- whole model
# id -> (variant, img_size, depths, panoramas, every parameter trainable)
MODEL_CASES = {
    "5m_160": ("tiny_vit_5m_224", 160, None, 2, True),                      # maps 20 / 10 / 5 -> 21 / 14 / 7; stage-3 BatchNorm over 8 * 25 = 200 samples
    "5m_256": ("tiny_vit_5m_224", 256, None, 1, False),                     # maps 32 / 16 / 8 -> 35 / 28 / 14, reference freeze policy
    "21m384_288": ("tiny_vit_21m_384", 288, (1, 1, 2, 1), 1, True),         # stage 1 divides (36 / 12); stages 2, 3: 18 -> 24, 9 -> 12
    "21m512_320": ("tiny_vit_21m_512", 320, (1, 1, 1, 1), 1, False),        # stage 2: 20 -> one padded 32 x 32 window (the flash route beyond 256 tokens)
}
_ORACLE = {}


def _build(case_id, precision, seed=11, drop_path_rate=0.1, features_only=False):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from tests.test_gpu_precision import _randomize
    name, img, depths, N, unfrozen = MODEL_CASES[case_id]
    kw = dict(drop_path_rate=drop_path_rate, img_size=img)
    if depths is not None:
        kw["depths"] = depths
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = TinyViTAdapter(name, pretrained=False, precision=precision, features_only=features_only, **kw)
    _randomize(base.backbone, seed + 1)
    return base.cuda(), kw


def _oracle_cfg(case_id, kw):
    from oracle import tinyvit_ref as R
    return R.config_for(MODEL_CASES[case_id][0], **kw)


def _pad_case(case_id, precision, centroids, monkeypatch, only_trainable=None, seed=11):
    """tests/test_gpu_precision.py::_train_step_case at an input size that pads: the HIP step, and the oracle's step with the padded block swapped in (computed once per
    (case, arithmetic, trainable set): fp32 and fp32_split start from the same weights and share the fp32 oracle)."""
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from oracle import tinyvit_ref as R
    from oracle import step_ref as S
    from tests.test_gpu_precision import gemm_launches
    name, img, depths, N, unfrozen = MODEL_CASES[case_id]
    base, kw = _build(case_id, precision, seed)
    cfg = _oracle_cfg(case_id, kw)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True).cuda().train()
    bb = base.backbone
    assert bb.padded_maps and bb.img_size == img
    if unfrozen:
        base.unfreeze_all()
    if only_trainable is not None:
        for n, p in bb._params.items():
            p.requires_grad_(n.startswith(only_trainable))
    trainable = [n for n, p in bb.named_parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.randn(N, 4, 3, img, img, generator=g)
    labels = torch.stack([torch.rand(N, generator=g) * 360 - 180, torch.rand(N, generator=g) * 180 - 90], 1)
    keep = (torch.rand(bb.num_drop_slots, 4 * N, generator=g) > 0.3)
    rates = torch.tensor(bb.drop_rates).unsqueeze(1)
    scales = (keep.float() / (1 - rates)).contiguous().cuda()
    assert max(bb.drop_rates) > 0
    bb.make_drop_scales = lambda batch, generator=None: scales
    st = {k: v.detach().cpu().clone() for k, v in bb.state_dict().items()}
    W, b = model.cell_layer.weight.detach().cpu().clone(), model.cell_layer.bias.detach().cpu().clone()
    with gemm_launches() as launches:
        out = model(pixel_values=x.cuda(), labels=labels.cuda(), labels_clf=None)
        out.loss.backward()
        torch.cuda.synchronize()
    emu = precision == "bf16"

    def oracle(emulate):
        key = (case_id, emulate, tuple(trainable), seed)
        if key not in _ORACLE:
            monkeypatch.setattr(R, "_tinyvit_block_m", P.tinyvit_block_padded)
            taps = {}
            st_o = {k: (t.clone().requires_grad_(True) if (t.is_floating_point() and "running" not in k and k in trainable) else t.clone()) for k, t in st.items()}
            Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
            emb_o = R.forward(cfg, st_o, x.reshape(4 * N, 3, img, img), training=True, emulate_bf16=emulate, drop_masks=[keep[s] for s in range(bb.num_drop_slots)], taps=taps)
            emb_o = emb_o.view(N, 4, -1)
            loss_o, logits_o = S.head_loss(emb_o, Wg, bg, torch.from_numpy(centroids), labels, emulate_bf16=emulate)
            loss_o.backward()
            grads = {k: t.grad for k, t in st_o.items() if t.requires_grad and t.grad is not None}
            grads["cell_layer.weight"], grads["cell_layer.bias"] = Wg.grad, bg.grad
            _ORACLE[key] = dict(taps={k: v.detach() for k, v in taps.items()}, emb_o=emb_o.detach(), loss_o=float(loss_o), grads=grads, st=st)
        return _ORACLE[key]
    o = oracle(emu)
    # gradients that are zero by construction (a bias in front of a conv + train-mode BatchNorm: the last fc2.bias of a stage): the fp32 oracle has them below
    # _grad_table's noise floor, and the bf16-emulating oracle holds only its own rounding noise there -- no reference value (see _gate)
    g32 = oracle(False)["grads"]
    floor32 = 1e-4 * float(np.median([float(t.norm()) for t in g32.values()]))
    structural_zero = sorted(k for k, t in g32.items() if float(t.norm()) <= floor32) if emu else []
    for k, v in o["st"].items():                     # the cached oracle ran from these very weights
        assert torch.equal(v, st[k]), k
    return dict(model=model, bb=bb, cfg=cfg, out=out, taps=o["taps"], emb_o=o["emb_o"], loss_o=o["loss_o"], grads=o["grads"], trainable=trainable, N=N, launches=launches,
                img=img, structural_zero=structural_zero)


def _compare_taps(case, dtype, tol, label):
    """tests/test_gpu_precision.py::_compare_taps with the padded blocks' attn.out mapped from the oracle's window order to the padded map's row order."""
    from tests.test_gpu_precision import _tap_names, relerr
    bb, cfg, taps, batch = case["bb"], case["cfg"], case["taps"], 4 * case["N"]
    rows = []
    for oname, hname, nchw in _tap_names(cfg):
        ref = taps[oname]
        if ref.dim() == 4 and nchw:
            ref = ref.permute(0, 2, 3, 1)
        try:
            raw = bb.activation(hname, batch)
        except Exception as exc:                     # a temporary under the freeze policy's plan
            if "not retained" in str(exc):
                continue
            raise
        if oname.endswith("attn.out"):
            s = int(oname.split(".")[1])
            ws, res = cfg.window_sizes[s], case["img"] // (4 * 2 ** s)
            pres = P.padded_side(res, ws)
            assert ref.shape[0] == batch * (pres // ws) ** 2
            ref = P.windows_to_padded_map(ref, batch, pres, ws)
        got = raw.view(dtype)[:ref.numel()].view(ref.shape).float().cpu()
        rows.append((oname, relerr(got, ref)))
    worst = max(rows, key=lambda r: r[1])
    print(f"\n[{label}] {len(rows)} activation taps, worst rel-L2 {worst[0]} {worst[1]:.3e}")
    bad = [(n, e) for n, e in rows if e > tol]
    assert not bad, (label, bad[:6])
    assert any(n.endswith("attn.out") for n, _ in rows)
    return dict(rows)


def _gate(case, precision, label):
    from tests.test_gpu_precision import _grad_table, relerr
    emb = case["out"].embedding.detach().cpu()
    e_abs, e_rel = float((emb - case["emb_o"]).abs().max()), relerr(emb, case["emb_o"])
    l_rel = abs(float(case["out"].loss) - case["loss_o"]) / case["loss_o"]
    print(f"[{label}] embedding max|err| {e_abs:.3e}, rel-L2 {e_rel:.3e}, loss rel {l_rel:.3e}")
    if precision == "bf16":          # the bounds of test_bf16_mode_train_step_matches_bf16_emulating_oracle
        errs = _compare_taps(case, BF, 8e-2, label)
        assert errs["patch_embed"] < 1e-2 and errs["stages.1.downsample.out"] < 2e-2
        assert e_rel < 2e-2 and l_rel < 2e-3
        # A gradient that is zero by construction has no reference value in the bf16-emulating oracle, only that oracle's own rounding noise (in fp32 _grad_table drops
        # such tensors by its noise floor; bf16 noise is above that floor: stages.1.blocks.0.mlp.fc2.bias of the 288-pixel case, in a stage that is NOT padded, came
        # out at rel-L2 1.7 against the oracle's noise).  These tensors are held to the noise-floor rule instead: at most 10 x the reference's own noise.
        zero = case["structural_zero"]
        _grad_table(dict(case, grads={k: v for k, v in case["grads"].items() if k not in zero}), 2e-1, label, median_tol=6e-2)
        floor = 1e-4 * float(np.median([float(t.norm()) for t in case["grads"].values()]))
        for k in zero:
            got, noise = float(case["bb"]._params[k].grad.norm()), float(case["grads"][k].norm())
            print(f"[{label}] zero by construction: {k} |g| {got:.3e}, the oracle's noise {noise:.3e}")
            assert got <= 10 * max(noise, floor), (k, got, noise, floor)
    else:                            # _fp32_gate
        _compare_taps(case, F32, 2e-4, label)
        assert e_abs < 5e-4 and e_rel < 1e-4
        assert l_rel < 1e-5
        _grad_table(case, 2e-3, label)


def _pad_launches():
    """Launches of the category GG_CAT_PAD in the profiler's log (call inside an enabled region, after a synchronize)."""
    from geoguessr_ai_amd import _lib as L
    lib, cat, n = L.lib(), C.c_int(), 0
    for i in range(lib.gg_prof_count()):
        L.check(lib.gg_prof_record(i, C.byref(cat), None, None, None), "gg_prof_record")
        n += (cat.value & 15) == L.PROF_CAT_PAD
    return n


def _free(*objs):
    del objs
    gc.collect(); torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
@pytest.mark.parametrize("case_id", list(MODEL_CASES))
def test_padded_train_step_matches_the_padded_oracle(centroids, monkeypatch, case_id, precision):
    case = _pad_case(case_id, precision, centroids, monkeypatch)
    name, img, depths, N, unfrozen = MODEL_CASES[case_id]
    label = f"{precision} {name}@{img} N={N} {'unfrozen' if unfrozen else 'ref-freeze'} padded {case['bb'].padded_maps}"
    gb = case["grads"].get([k for k in case["grads"] if k.endswith("attn.norm.bias")][-1])
    assert float(gb.abs().max()) > 0                                  # the pad keys / values reach attn.norm.bias
    _gate(case, precision, label)
    _free(case)


def _bb_step(bb, x, drop, d_out, poison=False):
    """One forward + backward at the backbone's C calls (tests/test_gpu_recompute.py::_step); poison: the training workspace is overwritten with NaN bytes first."""
    for p in bb._params.values():
        p.grad = None
    if bb._flat_grad is not None:
        bb._flat_grad.zero_()
    if poison:
        bb._ws[True].fill_(0xFF)
    out = bb.forward_hip(x, True, drop)
    bb.backward_hip(d_out)
    torch.cuda.synchronize()
    res = (out.clone(), bb._flat_grad.clone(), bb._flat_buf.clone())
    del out
    return res


@pytest.mark.parametrize("policy", ["all", "freeze"])
@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
def test_recompute_poisoned_workspace_and_graph_replay_are_bit_identical(centroids, precision, policy):
    """The 160-pixel model, 8 images (launch-bound: the calls are captured and replayed).  Four steps from the same running statistics: the first; one after the
    workspace was overwritten with NaN bytes (nothing may depend on what it held: the pad kernel writes every element of its region); a third, which replays the captured
    graphs; one with activation recompute.  Embedding, the head's loss on it, and every gradient are the same bits (the attention-bias tables' gradients, which the
    attention backward sums with float atomics, to 1e-5 of their magnitude -- tests/test_gpu_recompute.py)."""
    from geoguessr_ai_amd import _lib as L
    from oracle import step_ref as S
    from tests.test_gpu_recompute import _grad_mismatches, _stats
    base, _ = _build("5m_160", precision, seed=5)
    base.train()
    if policy == "freeze":
        base.freeze_all_but_last_stage()
    else:
        base.unfreeze_all()
    bb = base.backbone
    B = 8
    x = torch.randn(B, 3, 160, 160, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    drop = bb.make_drop_scales(B, generator=torch.Generator().manual_seed(11))
    assert drop is not None
    d_out = torch.randn(B, bb.num_features, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    b0, c0 = bb._flat_buf.clone(), bb._counters.clone()

    def run(poison=False):
        bb._flat_buf.copy_(b0); bb._counters.copy_(c0)
        return _bb_step(bb, x, drop, d_out, poison)
    cap0, rep0 = _stats()
    first = run()
    steps = {"poisoned workspace": run(poison=True), "graph replay": run()}
    cap1, rep1 = _stats()
    assert rep1 - rep0 >= 2, (cap0, cap1, rep0, rep1)                 # the third call replays the captured forward and backward
    bb.set_grad_checkpointing(True)
    steps["recompute"] = run()
    steps["recompute, poisoned workspace"] = run(poison=True)
    bb.set_grad_checkpointing(False)
    o0, g0, s0 = first
    assert torch.isfinite(o0).all() and torch.isfinite(g0).all() and float(g0.abs().sum()) > 0
    Wc = torch.randn(16, bb.num_features, generator=torch.Generator().manual_seed(2))
    loss = lambda o: F.cross_entropy(o.cpu() @ Wc.t(), torch.arange(B) % 16)
    for what, (o1, g1, s1) in steps.items():
        assert torch.equal(o0, o1), (what, "embedding")
        assert torch.equal(loss(o0), loss(o1)), (what, "loss")
        bad = _grad_mismatches(bb, g0, g1)
        assert not bad, f"{what}: gradients differ in {bad[:6]} ({len(bad)} tensors)"
        assert torch.equal(s0, s1), (what, "running statistics")
    _free(base, bb)


def test_trainable_mask_on_the_last_padded_block(centroids, monkeypatch):
    """Only the attention of the last padded block and head.norm train (the other blocks' padded inputs are temporaries the backward forms again): the fp32 gate."""
    case = _pad_case("5m_160", "fp32", centroids, monkeypatch, only_trainable=("stages.3.blocks.1.attn.", "head.norm."))
    assert sorted(case["trainable"]) == sorted(["head.norm.bias", "head.norm.weight"] + [f"stages.3.blocks.1.attn.{n}" for n in (
        "attention_biases", "norm.weight", "norm.bias", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias")])
    _gate(case, "fp32", "fp32 tiny_vit_5m_224@160 mask: last padded block's attention + head.norm")
    _free(case)


@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
def test_eval_surfaces_at_160(monkeypatch, precision):
    """Inference at a padded size: TinyViTAdapter's eval forward, features_only, and TinyViTClassifier.forward / pooled_features / forward_features against the oracle,
    at the eval bounds of the native-size tests (fp32 storage: embedding rel-L2 1e-4, tests/test_gpu_precision.py and test_gpu_round2.py; the last map 2e-4,
    test_gpu_tinyvit_classifier.py; bf16: max |err| 4e-2 against the bf16-emulating oracle, 8e-2 and cosine 0.999 against fp32, tests/test_gpu_model.py)."""
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    from oracle import tinyvit_ref as R
    from tests.test_gpu_precision import _randomize, relerr
    monkeypatch.setattr(R, "_tinyvit_block_m", P.tinyvit_block_padded)
    base, kw = _build("5m_160", precision, seed=3, drop_path_rate=0.0)
    cfg = _oracle_cfg("5m_160", kw)
    st = {k: v.detach().cpu().clone() for k, v in base.backbone.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    for k in st:
        if k.endswith("running_mean"):
            st[k] = 0.1 * torch.randn(st[k].shape, generator=g)
        elif k.endswith("running_var"):
            st[k] = 0.5 + torch.rand(st[k].shape, generator=g)
    base.backbone.load_state_dict(st)
    x = torch.randn(3, 3, 160, 160, generator=torch.Generator().manual_seed(1))
    taps = {}
    with torch.no_grad():
        ref = R.forward(cfg, st, x, training=False, taps=taps)
        emu = R.forward(cfg, st, x, training=False, emulate_bf16=True) if precision == "bf16" else None
    pooled_ref = taps["stages.3"].mean(dim=(-2, -1))

    def check(got, want, want_emu, what):
        got = got.float().cpu()
        print(f"[eval {precision} {what}] rel-L2 {relerr(got, want):.3e}, max|err| {float((got - want).abs().max()):.3e}")
        if precision == "bf16":
            assert float((got - want).abs().max()) < 8e-2 and float(F.cosine_similarity(got.flatten().double(), want.flatten().double(), dim=0)) > 0.999
            if want_emu is not None:
                assert float((got - want_emu).abs().max()) < 4e-2
        else:
            assert relerr(got, want) < 1e-4
    base.eval()
    with torch.no_grad():
        check(base(pixel_values=x.cuda()).pooler_output, ref, emu, "adapter")
        with pytest.raises(Exception, match="expects"):                 # another spatial size than img_size keeps raising
            base(pixel_values=torch.zeros(1, 3, 224, 224, device="cuda"))
    fo, _ = _build("5m_160", precision, seed=3, drop_path_rate=0.0, features_only=True)
    fo.backbone.load_state_dict(st)
    fo.eval()
    with torch.no_grad():
        check(fo(pixel_values=x.cuda()).pooler_output, pooled_ref, None, "features_only")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = TinyViTClassifier("tiny_vit_5m_224", num_classes=11, precision=precision, img_size=160, drop_path_rate=0.0, seed=4).cuda().eval()
    clf.backbone.load_state_dict(st)
    assert clf.backbone.padded_maps == ((1, 20, 21), (2, 10, 14), (3, 5, 7))
    with torch.no_grad():
        logits = clf(x.cuda())
        Wf, bf = clf.head.fc.weight.detach().cpu().float(), clf.head.fc.bias.detach().cpu().float()
        assert logits.shape == (3, 11)
        check(logits, F.linear(ref, Wf, bf), None if emu is None else F.linear(emu, Wf, bf), "classifier logits")
        check(clf.pooled_features(x.cuda()), pooled_ref, None, "classifier pooled_features")
        fmap = clf.forward_features(x.cuda())
        assert fmap.shape == taps["stages.3"].shape == (3, 320, 5, 5)
        assert relerr(fmap, taps["stages.3"]) < (8e-2 if precision == "bf16" else 2e-4)
    _free(base, fo, clf)


def test_native_sizes_take_no_pad_or_crop_launch(centroids):
    """padded_maps is empty at every variant's own size, and a native-size training step logs no launch of the pad / crop category -- a padded one logs, per padded
    block, pad + crop in the forward and pad + crop (+ one pad where the padded input was a temporary) in the backward."""
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter, VARIANTS, make_cfg
    lib = L.lib()
    for name in VARIANTS:
        cfg, v, _ = make_cfg(name, precision="fp32")
        assert all((cfg.img_size // (4 * 2 ** s)) % cfg.window_sizes[s] == 0 for s in (1, 2, 3)), name
    counts = {}
    for img in (224, 160):
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision="fp32_split", drop_path_rate=0.1, **({} if img == 224 else dict(img_size=img)))
        m = m.cuda().train()
        m.freeze_all_but_last_stage()
        bb = m.backbone
        assert (bb.padded_maps == ()) == (img == 224)
        x = torch.randn(4, 3, img, img, device="cuda")
        lib.gg_prof_reset(); lib.gg_prof_enable(1)
        out = m(pixel_values=x).pooler_output
        out.sum().backward()
        torch.cuda.synchronize()
        counts[img] = _pad_launches()
        lib.gg_prof_enable(0); lib.gg_prof_reset()
        _free(m, bb)
    print(f"pad / crop launches per step: {counts}")
    assert counts[224] == 0
    # 5M at 160: 2 + 6 + 2 padded blocks; stages 1 and 2 frozen (their xpad is a temporary: 5 launches each), stage 3 trainable (4 each)
    assert counts[160] == 8 * 5 + 2 * 4


def test_embedder_preprocesses_to_the_model_size():
    """TinyViTEmbedding(img_size=...): raw uint8 images are resized to the size the model was built for (with the checkpoint's own crop settings), float pixel_values of
    another size keep raising."""
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        emb = TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", load_checkpoint=False, panorama=False, img_size=160)
    bb = emb.tinyvit_model.backbone
    assert bb.img_size == 160 and bb.padded_maps == ((1, 20, 21), (2, 10, 14), (3, 5, 7))
    raw = torch.randint(0, 256, (2, 3, 200, 300), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    v = emb(raw)
    assert v.shape == (2, 320) and torch.isfinite(v).all()
    one = emb(raw[0])
    assert one.shape == (1, 320) and float((one - v[:1]).abs().max()) < 5e-2 * float(v.abs().max())      # (another batch size may take other GEMM kernels: not bit for bit)
    with pytest.raises(L.GgError, match="expects"):
        emb(torch.zeros(1, 3, 224, 224, device="cuda"))
    _free(emb, bb)
