"""The CLIP vision tower's fp32_split mode (GgClipCfg.act_dtype 3: f32 storage, every GEMM and the attention as f32-accurate split-bf16 products) on the GPU.
The mode earns its place the way TinyViT's did: it passes the fp32 mode's own gates of tests/test_gpu_clip.py at unchanged tolerances, against the same goldens
and the pinned oracle.  Then its two new kernels by themselves (head-dim-64 split attention against fp64, the QuickGELU epilogue classes of the split GEMM
bit for bit against the generic epilogue), recompute / masks / guard bands as in mode 1, and the Python surface."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from tests import clip_golden as CG
from tests import guards as G
from tests import masks as M
from tests.test_gpu_clip import _rel, _tiny_tower
from tests.test_gpu_clip_recompute import _assert_same_step, _off_and_on, _out_grads, _step

pytestmark = pytest.mark.gpu
SPLIT = "fp32_split"
L14 = "openai/clip-vit-large-patch14-336"


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as o
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return o


# ------------------------------------------------------------------------------------------- mode gates (the fp32 tolerances of tests/test_gpu_clip.py)
def test_forward_passes_the_fp32_gate_of_the_transformers_golden(golden_dir):
    case = CG.load(golden_dir)
    g = np.load(os.path.join(golden_dir, "clip_tiny.npz"))
    tower = _tiny_tower(case, SPLIT).cuda().eval()
    assert tower.precision == SPLIT and tower.cfg.act_dtype == 3
    out = tower(pixel_values=torch.from_numpy(g["x"]).cuda())
    y, lh = out.pooled_mean.detach().cpu().numpy(), out.last_hidden_state.detach().cpu().numpy()
    e_y, e_lh = _rel(y, g["y"]), _rel(lh, g["last_hidden_state"])
    print(f"\n[CLIP tiny {SPLIT}] pooled rel-L2 {e_y:.2e} (max abs {np.abs(y - g['y']).max():.2e}), last_hidden rel-L2 {e_lh:.2e}")
    assert e_y < 1e-4 and e_lh < 1e-4
    np.testing.assert_allclose(y, g["y"], rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("policy", ["all_layers", "last_layer"])
def test_training_passes_the_fp32_gate_of_the_reference_golden(golden_dir, centroids, policy):
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    case = CG.load(golden_dir)
    g = case["g"]
    tower = _tiny_tower(case, SPLIT)
    model = SuperGuessr(base_model=tower, panorama=True, should_smooth_labels=True)
    assert model.mode == "transformer" and model.precision == "fp32" and model.split          # (the head stores and checks like fp32)
    if policy == "last_layer":
        for layer in list(tower.vision_model.encoder.layers)[:-1]:
            for p in layer.parameters():
                p.requires_grad = False
    with torch.no_grad():
        model.cell_layer.weight.copy_(case["W"]); model.cell_layer.bias.copy_(case["b"])
    model = model.cuda().train()
    out = model(pixel_values=case["x"].cuda(), labels=case["labels"].cuda(), labels_clf=torch.from_numpy(g["labels_clf"]).cuda())
    out.loss.backward()
    torch.cuda.synchronize()
    loss_rel = abs(float(out.loss.detach()) - float(g["loss"])) / float(g["loss"])
    emb_rel = _rel(out.embedding.detach(), g["embedding"])
    vm = tower.vision_model
    frozen = [n for n, p in vm._params.items() if not p.requires_grad]
    assert bool(frozen) == (policy == "last_layer") and all(vm._params[n].grad is None for n in frozen)
    case_live = dict(case, names=[n for n in case["names"] if n not in frozen])
    errs = CG.grad_errors(case_live, {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in vm._params.items() if n not in frozen})
    worst = max(errs, key=errs.get)
    dW_rel = _rel(model.cell_layer.weight.grad[torch.from_numpy(g["labels_clf"]).cuda()], g["dW_rows"])
    print(f"\n[SuperGuessr on CLIP tiny, {SPLIT}, {policy}] loss rel {loss_rel:.2e}, embedding rel-L2 {emb_rel:.2e}, head dW rows {dW_rel:.2e}, "
          f"{len(errs)} tower gradients: worst {worst} {errs[worst]:.2e}")
    assert loss_rel < 1e-5 and emb_rel < 1e-4 and dW_rel < 1e-4
    assert errs[worst] < 1e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    np.testing.assert_array_equal(out.preds_geocell.cpu().numpy(), g["preds_geocell"])


def _oracle_case(model_name, cfg_tuple, n_pano, seed, trainable_from, centroids):
    """tests/test_gpu_clip.py::_oracle_case for a tower of cfg_tuple's depth in the fp32_split mode."""
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    from oracle import clip_ref as CR
    tower = CLIPVisionTower(model_name, seed=seed, precision=SPLIT, num_layers=cfg_tuple[2])
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in tower.vision_model._params.items():
            if n.endswith(("norm.weight", "norm1.weight", "norm2.weight")):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    st = {k: v.detach().clone() for k, v in tower.named_views().items()}
    cfg = CR.ClipVisionConfig(*cfg_tuple)
    x = torch.randn(n_pano, 4, 3, cfg.image_size, cfg.image_size, generator=g)
    labels = torch.stack([torch.rand(n_pano, generator=g) * 360 - 180, torch.rand(n_pano, generator=g) * 180 - 90], 1)
    W, b = torch.randn(12647, cfg.hidden_size, generator=g) * 0.03, torch.randn(12647, generator=g) * 0.1
    names = [n for n in st if n.startswith("encoder.layers.") and int(n.split(".")[2]) >= trainable_from]
    ref = CR.train_step(cfg, st, W, b, torch.from_numpy(centroids), x, labels, trainable=names)
    return tower, cfg, x, labels, W, b, names, ref


def _finetune(tower, x, labels, W, b, names):
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    model = SuperGuessr(base_model=tower, panorama=True, should_smooth_labels=True)
    for n, p in tower.vision_model._params.items():
        p.requires_grad = n in names
    with torch.no_grad():
        model.cell_layer.weight.copy_(W); model.cell_layer.bias.copy_(b)
    return model.cuda().train()


def test_base_patch32_dimensions_finetune_and_adamw_pass_the_fp32_gate(centroids):
    """ViT-B/32 dimensions (768 wide, 50 tokens), 2 layers, 2 panoramas, last layer trainable, against the pinned oracle at the fp32 gate of
    test_clip_base_patch32_last_layer_finetune_matches_oracle; two AdamW steps then move exactly the trainable range -- the second forward runs on planes
    re-split after the first step (a stale plane would leave the loss where it was)."""
    from geoguessr_ai_amd.optim import AdamW
    tower, cfg, x, labels, W, b, names, ref = _oracle_case("openai/clip-vit-base-patch32", (768, 3072, 2, 12, 224, 32), 2, 5, 1, centroids)
    model = _finetune(tower, x, labels, W, b, names)
    opt = AdamW(model, lr=1e-3)
    before = tower.vision_model.flat_params.clone()
    out = model(pixel_values=x.cuda(), labels=labels.cuda())
    out.loss.backward()
    errs = {n: _rel(tower.vision_model._params[n].grad, ref["grads"][n]) for n in names if not n.endswith("k_proj.bias")}
    worst = max(errs, key=errs.get)
    loss_rel = abs(float(out.loss.detach()) - float(ref["loss"])) / float(ref["loss"])
    emb_rel = _rel(out.embedding.detach(), ref["embedding"])
    print(f"\n[CLIP B/32 x 2 layers {SPLIT}, top layer trainable] loss rel {loss_rel:.2e}, embedding rel-L2 {emb_rel:.2e}, {len(errs)} gradients: worst {worst} {errs[worst]:.2e}")
    assert loss_rel < 1e-5 and emb_rel < 1e-4 and errs[worst] < 2e-4
    assert _rel(model.cell_layer.weight.grad, ref["grads"]["cell_layer.weight"]) < 1e-4
    opt.step(); opt.zero_grad()
    out2 = model(pixel_values=x.cuda(), labels=labels.cuda())
    out2.loss.backward(); opt.step()
    torch.cuda.synchronize()
    after = tower.vision_model.flat_params
    (lo, hi), = tower.vision_model.trainable_ranges()
    assert torch.equal(after[:lo], before[:lo]) and torch.equal(after[hi:], before[hi:]) and not torch.equal(after[lo:hi], before[lo:hi])
    assert float(out2.loss.detach()) < float(out.loss.detach())
    # the planes the second forward read are those of the stepped weights: a full rebuild of the cache changes no bit of a third forward
    model.eval()
    with torch.no_grad():
        a = tower(pixel_values=x[0].cuda()).pooled_mean.clone()
        tower.vision_model.mark_params_dirty()
        b_ = tower(pixel_values=x[0].cuda()).pooled_mean
    G.assert_bit_identical(a, b_, "the refresh after the optimizer step against a further rebuild of the weight cache")


def test_large_patch14_336_dimensions_finetune_passes_the_fp32_gate(centroids):
    """ViT-L/14-336 dimensions (1024 wide, 577 tokens = 9 key tiles + 1 token, patch 14: contraction 588 padded to 592), 2 layers, 2 panoramas, top layer
    trainable, at the fp32 gate of test_clip_large_patch14_336_forward_and_finetune_fp32."""
    tower, cfg, x, labels, W, b, names, ref = _oracle_case(L14, (1024, 4096, 2, 16, 336, 14), 2, 3, 1, centroids)
    model = _finetune(tower, x, labels, W, b, names)
    out = model(pixel_values=x.cuda(), labels=labels.cuda())
    out.loss.backward()
    emb_rel = _rel(out.embedding.detach(), ref["embedding"])
    errs = {n: _rel(tower.vision_model._params[n].grad, ref["grads"][n]) for n in names if not n.endswith("k_proj.bias")}
    worst = max(errs, key=errs.get)
    loss_rel = abs(float(out.loss.detach()) / float(ref["loss"]) - 1)
    print(f"\n[CLIP L/14-336 x 2 layers {SPLIT}] embedding rel-L2 {emb_rel:.2e}, loss rel {loss_rel:.2e}, top-layer gradients worst {worst} {errs[worst]:.2e}")
    assert emb_rel < 1e-4 and loss_rel < 1e-5 and errs[worst] < 2e-4


# ------------------------------------------------------------------------------------------- the attention kernels against fp64
NH, HD, NIMG = 2, 64, 2
_ATTN = {}


def _attn_case(N, spike=False):
    """Inputs (CLIP's [q | k | v] blocks), the fp64 reference (out, lse, dq, dk, dv), computed once per token count."""
    key = (N, spike)
    if key not in _ATTN:
        g = torch.Generator().manual_seed(100 + N)
        qkv = torch.randn(NIMG * N, 3 * NH * HD, generator=g)
        dout = torch.randn(NIMG * N, NH * HD, generator=g)
        if spike:      # the row maximum of query 5 grows tile after tile: keys 20, 70, 140, 195 (tiles 0 .. 3) line up with it ever more strongly
            qkv = qkv * 0.2
            qkv[5, :HD] = 2.0
            for k_, s in ((20, 0.5), (70, 1.0), (140, 1.5), (195, 2.0)):
                qkv[k_, NH * HD:NH * HD + HD] = s
        x = qkv.double().reshape(NIMG, N, 3, NH, HD).requires_grad_(True)
        q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
        s = q @ k.transpose(-1, -2) * HD ** -0.5
        lse = torch.logsumexp(s, -1)
        out = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(NIMG * N, NH * HD)
        out.backward(dout.double())
        dx = x.grad.reshape(NIMG * N, 3, NH * HD)
        _ATTN[key] = dict(qkv=qkv, dout=dout, out=out.detach(), lse=lse.detach().transpose(1, 2).reshape(NIMG * N, NH), dq=dx[:, 0], dk=dx[:, 1], dv=dx[:, 2])
    return _ATTN[key]


def _attn_run(ops, c, N, split):
    kw = dict(num_windows=NIMG, tokens_per_window=N, num_heads=NH, head_dim=HD, q_off=0, k_off=NH * HD, v_off=2 * NH * HD, head_stride=HD, split=split)
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    out, lse = ops.attention_flash(qkv, want_lse=True, **kw)
    dqkv, _ = ops.attention_flash(qkv, dout=dout, out=out, lse=lse, **kw)
    dqkv2, _ = ops.attention_flash(qkv, dout=dout, out=out, lse=lse, **kw)
    torch.cuda.synchronize()
    d = dqkv.reshape(-1, 3, NH * HD)
    return dict(out=out, lse=lse, dq=d[:, 0], dk=d[:, 1], dv=d[:, 2]), dqkv, dqkv2


def _attn_errs(got, c):
    return {k: float((got[k].double().cpu() - c[k]).abs().max() / c[k].abs().max()) for k in ("out", "lse", "dq", "dk", "dv")}


# 16, 17: one tile with and without a remainder; 50: ViT-B/32; 64, 65: the tile boundary; 256, 257: where the f32 kernels change from one pass to two (the
# split kernels run two passes at every length: no boundary of their own); 577: ViT-L/14-336 = 9 * 64 + 1
@pytest.mark.parametrize("N", [16, 17, 50, 64, 65, 256, 257, 577])
def test_split_attention_against_fp64(ops, N):
    """Forward and backward of gg_attention_flash_fwd / _bwd with dtype 3 against an fp64 reference: out, lse, dq, dk, dv each within 1e-5 of the reference's
    largest magnitude (the f32 gate).  The f32-MFMA kernels (dtype 1) run on the same inputs: both errors are printed (DESIGN.md 5 holds the table).  Two
    backwards of one forward give identical bits.

    Measured on an MI355X: split 1.2e-7 ... 9.1e-7, f32 9.2e-8 ... 1.4e-6 over all cases and tensors (the table is in DESIGN.md 5)."""
    c = _attn_case(N)
    got, dqkv, dqkv2 = _attn_run(ops, c, N, True)
    f32, _, _ = _attn_run(ops, c, N, False)
    es, ef = _attn_errs(got, c), _attn_errs(f32, c)
    print(f"\n[attention hd64 N={N}] " + "  ".join(f"{k}: split {es[k]:.2e} f32 {ef[k]:.2e}" for k in es))
    for k in es:
        assert torch.isfinite(got[k]).all() and es[k] <= 1e-5, (k, es[k])
    G.assert_bit_identical(dqkv, dqkv2, "two backwards of one forward")


def test_split_attention_online_softmax_rescale_branch(ops):
    """The running maximum of one query's row grows across four key tiles (the rescale path of the forward, taken three times), as
    tests/test_gpu_precision.py::test_flash_online_softmax_rescale_branch drives it for the f32 kernels: like that test, this one gates the forward, where the
    branch is (out and lse at the 1e-5 of the cases above).  The backward has no running maximum; its figures on this input are printed for both kernels and
    not gated: with a score of 32 the exponent's argument is ~46 in the exp2 domain, whose f32 ulp (3.8e-6) is the relative error of P whatever forms the
    product, and dS = P (dP - delta) cancels on the row's one dominant key.  Measured on an MI355X: split dq 4.8e-06, dk 1.1e-05, dv 5.6e-07 of the
    reference's largest magnitude."""
    N = 200
    c = _attn_case(N, spike=True)
    got, _, _ = _attn_run(ops, c, N, True)
    f32, _, _ = _attn_run(ops, c, N, False)
    es, ef = _attn_errs(got, c), _attn_errs(f32, c)
    print(f"\n[attention hd64 rescale N={N}] " + "  ".join(f"{k}: split {es[k]:.2e} f32 {ef[k]:.2e}" for k in es))
    for k in ("out", "lse"):
        assert es[k] <= 1e-5, (k, es[k])


def test_split_attention_refuses_what_it_does_not_implement(ops):
    from geoguessr_ai_amd import _lib as L
    qkv = torch.randn(2 * 49, 3 * 2 * 32).cuda()
    out0 = None
    with pytest.raises(L.GgError, match="dtype 3"):
        out0 = ops.attention_flash(qkv, num_windows=2, tokens_per_window=49, num_heads=2, head_dim=32, q_off=0, k_off=64, v_off=128, head_stride=32, split=True)
    assert out0 is None
    qkv = torch.randn(49, 3 * 64).cuda()
    with pytest.raises(L.GgError, match="dtype 3"):
        ops.attention_flash(qkv, num_windows=1, tokens_per_window=49, num_heads=1, head_dim=64, q_off=0, k_off=64, v_off=128, head_stride=64, window_size=7,
                            map_h=7, map_w=7, split=True)


# ------------------------------------------------------------------------------------------- QuickGELU epilogue classes of the split GEMM
def _split_gemm(A, Wp, N, K, *, bias=None, act=0, want_pre=False, dact_pre=None, dact=0, planes=False):
    from geoguessr_ai_amd import _lib as L
    M = A.shape[0]
    a = L.Split3Args()
    out = torch.full((M, N), float("nan"), device="cuda")
    pre = torch.full((M, N), float("nan"), device="cuda") if want_pre else None
    cp = torch.empty((3, M, N), dtype=torch.bfloat16, device="cuda") if planes else None
    a.b_planes, a.ldb, a.M, a.N, a.K = Wp.data_ptr(), K, M, N, K
    a.C, a.ldc = out.data_ptr(), N
    if planes:
        a.c_planes, a.ldp = cp.data_ptr(), N
    a.bias = bias.data_ptr() if bias is not None else None
    a.act = act
    a.preact = pre.data_ptr() if want_pre else None
    if dact_pre is not None:
        a.dact_preact, a.dact = dact_pre.data_ptr(), dact
    L.check(L.lib().gg_gemm_nt_split3_af32(C.byref(a), A.data_ptr(), A.stride(0), 0, L.stream()), "gg_gemm_nt_split3_af32")
    torch.cuda.synchronize()
    return out, pre


@pytest.mark.parametrize("K", [64, 768])
@pytest.mark.parametrize("form", ["fc1", "fc2_dgrad"])
def test_quickgelu_epilogue_classes_are_bit_identical_to_the_generic_epilogue(form, K):
    """M = 257 (off the tile), N = 136 (a multiple of 8, not of 96 or 128), K = 64 (the 128-row kernel) and 768 (the 256-row kernel): C and the saved
    pre-activation of the compile-time class equal, bit for bit, those of the same call with c_planes also requested (which takes the generic row epilogue),
    and both are within 1e-5 relative of the fp64 product."""
    from geoguessr_ai_amd import _lib as L
    M, N = 257, 136
    g = torch.Generator().manual_seed(7 + K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    bias, saved = torch.randn(N, generator=g) * 0.3, torch.randn(M, N, generator=g) * 2
    Wd = W.cuda().contiguous()
    Wp = torch.empty((3, N, K), dtype=torch.bfloat16, device="cuda")
    L.check(L.lib().gg_split3_bf16(Wd.data_ptr(), N, K, K, Wp.data_ptr(), L.stream()), "gg_split3_bf16")
    acc = A.double() @ W.double().T
    qg = lambda z: z * torch.sigmoid(1.702 * z)
    if form == "fc1":
        kw = dict(bias=bias.cuda(), act=2, want_pre=True)
        ref_pre = acc + bias.double()
        ref = qg(ref_pre)
    else:
        kw = dict(dact_pre=saved.cuda(), dact=2)
        z = saved.double()
        sg = torch.sigmoid(1.702 * z)
        ref_pre, ref = None, acc * (sg * (1 + 1.702 * z * (1 - sg)))
    c_ec, p_ec = _split_gemm(A.cuda(), Wp, N, K, **kw)
    c_gen, p_gen = _split_gemm(A.cuda(), Wp, N, K, planes=True, **kw)
    G.assert_bit_identical(c_ec, c_gen, f"{form} K={K}: C")
    e = _rel(c_ec, ref)
    print(f"\n[split GEMM QuickGELU {form} K={K}] C rel-L2 vs fp64 {e:.2e}")
    assert torch.isfinite(c_ec).all() and e < 1e-5 and _rel(c_gen, ref) < 1e-5
    if form == "fc1":
        G.assert_bit_identical(p_ec, p_gen, f"{form} K={K}: preact")
        assert _rel(p_ec, ref_pre) < 1e-5 and _rel(p_gen, ref_pre) < 1e-5


# ------------------------------------------------------------------------------------------- recompute, masks, guard bands
def _tiny_masks(tower):
    names = [t["name"] for t in tower.vision_model.table]
    nl = tower.cfg.num_layers
    top = frozenset(n for n in names if n.startswith(f"encoder.layers.{nl - 1}."))
    emb = frozenset(n for n in names if n.startswith(("embeddings.", "pre_layrnorm.")))
    return dict(all=frozenset(names), last_layer=top, embeddings_and_top=emb | top)


@pytest.mark.parametrize("key", ["all", "last_layer", "embeddings_and_top"])
def test_recompute_is_bit_identical_on_the_tiny_tower(golden_dir, key):
    case = CG.load(golden_dir)
    tower = _tiny_tower(case, SPLIT).cuda().train()
    x = torch.from_numpy(np.load(os.path.join(golden_dir, "clip_tiny.npz"))["x"]).cuda()
    d_out, d_last = _out_grads(tower, x.shape[0])
    mask = M.apply(tower.vision_model, _tiny_masks(tower)[key])
    off, on = _off_and_on(tower, x, d_out, d_last)
    _assert_same_step(tower, mask, off, on, f"tiny {SPLIT} {key}")


def test_recompute_is_bit_identical_at_large_patch14_336_dimensions():
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    tower = CLIPVisionTower(L14, precision=SPLIT, seed=3, num_layers=2).cuda().train()
    assert tower.num_tokens == 577
    x = torch.randn(2, 3, 336, 336, generator=torch.Generator().manual_seed(4)).cuda()
    d_out, d_last = _out_grads(tower, 2)
    mask = M.apply(tower.vision_model, frozenset(t["name"] for t in tower.vision_model.table))
    off, on = _off_and_on(tower, x, d_out, d_last)
    _assert_same_step(tower, mask, off, on, f"L/14-336 x 2 layers {SPLIT}")
    del tower, off, on
    gc.collect(); torch.cuda.empty_cache()


def test_step_in_guarded_workspace_cache_and_gradient_buffer(golden_dir):
    """One forward + backward on a workspace and a weight cache of exactly the library's sizes and a flat gradient buffer, each between guard bands; the
    workspace and the cache start as NaN (then as finite garbage): the bands stay intact and the results equal a clean run's, bit for bit."""
    from tests.test_gpu_guards_model import _clip_install
    case = CG.load(golden_dir)
    x = torch.from_numpy(np.load(os.path.join(golden_dir, "clip_tiny.npz"))["x"]).cuda()
    batch = x.shape[0]
    clean = _tiny_tower(case, SPLIT).cuda().train()
    d_out, d_last = _out_grads(clean, batch)
    want = _step(clean, x, d_out, d_last)
    assert float(want[2].abs().sum()) > 0
    for fill, zero in (("nan", False), ("finite", False)):
        tower = _tiny_tower(case, SPLIT).cuda().train()
        vm = tower.vision_model
        S = G.GuardSet(fill)
        ws, wc = _clip_install(tower, S, batch, True, zero)
        fg = S.scratch("flat gradient buffer", vm.param_floats * 4, row_bytes=4 * tower.cfg.intermediate_size, zero=True)
        vm._flat_grad = fg.view[0].view(torch.float32)
        got = _step(tower, x, d_out, d_last)
        assert vm._ws[True].data_ptr() == ws.ptr and vm._wcache.data_ptr() == wc.ptr and vm._flat_grad.data_ptr() == fg.ptr
        S.check()
        for u, v, what in zip(got, want, ("pooled", "last_hidden", "flat gradient")):
            assert torch.isfinite(u).all(), what
            G.assert_bit_identical(u, v, f"{fill} fill: {what}")
        del tower, vm, S, ws, wc, fg
        gc.collect(); torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- surface
def test_embedding_wrapper_matches_the_fp32_tower():
    """CLIPEmbedding(precision="fp32_split") under no_grad against the fp32 tower with the same weights: rel-L2 1e-5 (the TinyViT inference gate of
    test_fp32_split_inference_embeddings_match_the_fp32_mode)."""
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPEmbedding
    kw = dict(num_layers=3)
    e1 = CLIPEmbedding("openai/clip-vit-base-patch32", device="cuda", precision="fp32", **kw)
    e3 = CLIPEmbedding("openai/clip-vit-base-patch32", device="cuda", precision=SPLIT, **kw)
    assert e3.clip_model.precision == SPLIT and e1.clip_model.precision == "fp32"
    x = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(2)).cuda()
    a, b = e1(x), e3(x)
    rel = _rel(b, a)
    print(f"\n[CLIPEmbedding B/32 x 3 layers] fp32_split vs fp32 pooled embedding rel-L2 {rel:.2e}")
    assert torch.isfinite(b).all() and rel < 1e-5


def test_gg_precision_environment_reaches_the_tower(monkeypatch):
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPVisionTower
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    monkeypatch.setenv("GG_PRECISION", SPLIT)
    tower = CLIPVisionTower("openai/clip-vit-base-patch32", num_layers=1)
    assert tower.precision == SPLIT and tower.backbone.precision == SPLIT
    model = SuperGuessr(base_model=tower, panorama=True)
    assert model.precision == "fp32" and model.split
    tower = tower.cuda().eval()
    with torch.no_grad():
        out = tower(pixel_values=torch.randn(1, 3, 224, 224).cuda())
    assert torch.isfinite(out.pooled_mean).all()


def test_fp16_training_refusal_is_unchanged(golden_dir):
    from geoguessr_ai_amd import _lib as L
    case = CG.load(golden_dir)
    g = np.load(os.path.join(golden_dir, "clip_tiny.npz"))
    tower = _tiny_tower(case, "fp16").cuda()
    with pytest.raises(L.GgError, match="inference-only"):
        tower(pixel_values=torch.from_numpy(g["x"]).cuda())
