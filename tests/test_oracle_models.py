"""Oracle self-checks: CLIP restatement pinned to transformers; TinyViT restatement (parity
UNPINNED, timm absent) checked by invariants from SURVEY.md App. A.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import clip_ref as C
from oracle import tinyvit_ref as R


def test_clip_matches_transformers_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "clip_tiny.npz"))
    hs, inter, L, nh, img, ps = [int(v) for v in g["cfg"]]
    cfg = C.ClipVisionConfig(hs, inter, L, nh, img, ps)
    st = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    assert {n for n, _ in C.param_spec(cfg)} == set(st.keys())
    for n, shp in C.param_spec(cfg):
        assert tuple(st[n].shape) == shp, n
    y = C.forward(cfg, st, torch.from_numpy(g["x"]))
    np.testing.assert_allclose(y.numpy(), g["y"], rtol=1e-4, atol=2e-5)


def test_clip_param_counts():
    b32 = C.ClipVisionConfig()
    n = sum(int(np.prod(s)) for _, s in C.param_spec(b32))
    assert n == 87456000, n                       # 87.46 M
    assert b32.num_tokens == 50
    l14 = C.ClipVisionConfig(1024, 4096, 24, 16, 336, 14)
    assert l14.num_tokens == 577


def test_tinyvit_param_totals_and_macs():
    c21 = R.config_for("tiny_vit_21m_224")
    c5 = R.config_for("tiny_vit_5m_224")
    assert R.num_params(c21) == 20621568 and R.num_params(c5) == 5071764       # App. A.4
    assert abs(R.macs_per_image(c21)["total"] / 1e6 - 4250) < 1.0
    assert abs(R.macs_per_image(c5)["total"] / 1e6 - 1255) < 1.0
    per_stage = {}
    for n, s, k in R.param_spec(c21):
        if k == "param":
            key = n.split(".blocks")[0].split(".downsample")[0] if n.startswith("stages") else n.split(".")[0]
            per_stage[key] = per_stage.get(key, 0) + int(np.prod(s))
    assert per_stage == {"patch_embed": 43056, "stages.0": 157824, "stages.1": 952716,
                         "stages.2": 10913184, "stages.3": 8553636, "head": 1152}
    n_bn = sum(1 for n, _, _ in R.param_spec(c21) if n.endswith("bn.weight"))
    assert n_bn == 27                                                          # App. A.3
    # trainable under freeze_all_but_last_stage + 12647-cell head
    tr = per_stage["patch_embed"] + per_stage["stages.3"] + per_stage["head"] + 12647 * 576 + 12647
    assert tr == 15895163


def test_tinyvit_forward_backward_and_eval_folding():
    cfg = R.config_for("tiny_vit_5m_224")
    st = R.init_state(cfg, 1, randomize_norms=True)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    y = R.forward(cfg, st, x, training=False)
    assert y.shape == (2, 320) and torch.isfinite(y).all()
    assert abs(float(y.mean())) < 0.5      # LayerNorm'd output with small affine perturbation
    # eval-mode BN == conv with folded scale/shift
    p = "patch_embed.conv1"
    w, g_, b_, mu, var = (st[f"{p}.conv.weight"], st[f"{p}.bn.weight"], st[f"{p}.bn.bias"],
                          st[f"{p}.bn.running_mean"], st[f"{p}.bn.running_var"])
    s = g_ / torch.sqrt(var + cfg.bn_eps)
    a = torch.nn.functional.conv2d(x, w * s[:, None, None, None], b_ - mu * s, 2, 1)
    c = R._Ctx(cfg, st, False, False, False, None)
    np.testing.assert_allclose(R._convnorm(c, x, p, 2, 1).numpy(), a.numpy(), rtol=1e-4, atol=1e-5)
    # training forward differentiates w.r.t. every parameter
    stg = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v) for k, v in st.items()}
    out = R.forward(cfg, stg, x, training=True)
    out.square().mean().backward()
    missing = [k for k, v in stg.items() if v.requires_grad and v.grad is None]
    assert not missing, missing


def test_tinyvit_window_partition_equals_blockwise_attention():
    """stage-1 windows (28x28 map, ws 7): permuting whole windows permutes the output."""
    cfg = R.config_for("tiny_vit_5m_224")
    st = R.init_state(cfg, 2, randomize_norms=True)
    c = R._Ctx(cfg, st, False, False, False, None)
    C1 = cfg.embed_dims[1]
    x = torch.randn(1, 28, 28, C1)
    y = R._tinyvit_block_m(c, x, "stages.1.blocks.0", cfg.num_heads[1], 7, None, 0)
    xs = torch.roll(x, shifts=(7, 14), dims=(1, 2))
    ys = R._tinyvit_block_m(c, xs, "stages.1.blocks.0", cfg.num_heads[1], 7, None, 0)
    # attention is window-local but local_conv (3x3 dw) couples neighbours across window borders;
    # compare the attention residual only (tap x1)
    taps_a, taps_b = {}, {}
    ca = R._Ctx(cfg, st, False, False, False, taps_a); cb = R._Ctx(cfg, st, False, False, False, taps_b)
    R._tinyvit_block_m(ca, x, "stages.1.blocks.0", cfg.num_heads[1], 7, None, 0)
    R._tinyvit_block_m(cb, xs, "stages.1.blocks.0", cfg.num_heads[1], 7, None, 0)
    np.testing.assert_allclose(torch.roll(taps_a["stages.1.blocks.0.x1"], (7, 14), (1, 2)).numpy(),
                               taps_b["stages.1.blocks.0.x1"].numpy(), rtol=1e-4, atol=1e-5)
    assert y.shape == ys.shape


@pytest.mark.parametrize("C,nh,ws", [(192, 6, 7), (384, 12, 14), (64, 2, 3)])
def test_tinyvit_attention_core_matches_transformers_levit(C, nh, ws):
    """A component pin for the otherwise unpinned TinyViT oracle (timm is not installed): timm's TinyViT ``Attention`` is LeViT's attention -- the same
    per-head [q|k|v] split of one fused projection, ``q k^T * key_dim^-0.5 + attention_biases[:, attention_bias_idxs]`` with the offsets numbered in first-seen
    order, softmax, P.V, head merge -- and ``transformers`` ships LeViT (``LevitAttention``), an implementation this repository did not write.  Its qkv projection is
    Linear + BatchNorm1d: in eval mode with running_mean 0, gamma = sqrt(running_var + eps), beta = b that is exactly Linear with bias b.  The tensor it hands to its
    output projection (captured in front of its Hardswish) must equal the oracle's ``attn.out`` tap for the same weights and the same (already normalised) input."""
    from transformers.models.levit.modeling_levit import LevitAttention
    from oracle import tinyvit_ref as R
    g = torch.Generator().manual_seed(C + ws)
    hd = C // nh
    assert hd == 32
    ref = LevitAttention(C, hd, nh, 1, ws)
    ref.eval()                                      # (its train() override returns None)
    W = torch.randn(3 * C, C, generator=g) * C ** -0.5
    b = torch.randn(3 * C, generator=g) * 0.1
    bias_tab = torch.randn(nh, ws * ws, generator=g) * 0.5
    with torch.no_grad():
        ref.queries_keys_values.linear.weight.copy_(W)
        bn = ref.queries_keys_values.batch_norm
        bn.running_mean.zero_(); bn.running_var.copy_(torch.rand(3 * C, generator=g) + 0.5)
        bn.weight.copy_(torch.sqrt(bn.running_var + bn.eps)); bn.bias.copy_(b)
        assert ref.attention_biases.shape == bias_tab.shape            # one entry per (|dy|, |dx|) offset: ws * ws
        ref.attention_biases.copy_(bias_tab)
    seen = {}
    ref.activation.register_forward_pre_hook(lambda m, inp: seen.__setitem__("o", inp[0].detach().clone()))
    xn = torch.randn(5, ws * ws, C, generator=g)
    with torch.no_grad():
        ref(xn)
    # the oracle's block on the same weights (its proj is irrelevant here: identity)
    cfg = R.config_for("tiny_vit_21m_224")
    p = "blk"
    st = {f"{p}.attn.qkv.weight": W, f"{p}.attn.qkv.bias": b, f"{p}.attn.attention_biases": bias_tab,
          f"{p}.attn.proj.weight": torch.eye(C), f"{p}.attn.proj.bias": torch.zeros(C)}
    taps = {}
    c = R._Ctx(cfg, st, False, False, False, taps)
    with torch.no_grad():
        R._attention_core(c, xn, p, nh, ws)
    got = taps[f"{p}.attn.out"]
    assert got.shape == seen["o"].shape
    assert torch.equal(ref.attention_bias_idxs, R.attention_bias_idxs(ws))
    assert torch.allclose(got, seen["o"], rtol=1e-5, atol=2e-6), float((got - seen["o"]).abs().max())


def test_clip_training_step_matches_reference_golden(golden_dir, centroids):
    """``oracle.clip_ref.train_step`` (torch autograd over the restated tower + ``step_ref.head_loss``) against the REFERENCE's SuperGuessr run
    on a transformers CLIPVisionModel base (tests/golden/clip_train.npz): loss, (N,4,C) embedding, every parameter gradient."""
    from tests import clip_golden as CG
    case = CG.load(golden_dir)
    g = case["g"]
    cfg = C.ClipVisionConfig(*case["cfg"])
    r = C.train_step(cfg, case["weights"], case["W"], case["b"], torch.from_numpy(centroids), case["x"], case["labels"])
    np.testing.assert_allclose(float(r["loss"]), float(g["loss"]), rtol=1e-6)
    np.testing.assert_allclose(r["embedding"].numpy(), g["embedding"], rtol=1e-4, atol=2e-5)
    np.testing.assert_array_equal(r["logits"].argmax(-1).numpy(), g["preds_geocell"])
    errs = CG.grad_errors(case, r["grads"])
    assert len(errs) == 39 and max(errs.values()) < 1e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    np.testing.assert_allclose(r["grads"]["cell_layer.weight"].numpy()[g["labels_clf"]], g["dW_rows"], rtol=1e-4, atol=1e-9)
