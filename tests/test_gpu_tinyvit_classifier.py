"""TinyViTClassifier (models/tinyvit_classifier.py) and the finetune_tinyvit loop on the GPU: the whole training step against the CPU oracle
(oracle/tinyvit_ref.py + torch Linear + cross_entropy) at the project's fp32 gate (tests/test_gpu_precision.py::_fp32_gate: loss 1e-5 relative, every
gradient tensor 2e-3 rel-L2, embedding 1e-4) in the fp32 and fp32_split modes, the bf16 mode at the tolerances of
test_bf16_mode_train_step_matches_bf16_emulating_oracle, the state-dict contract, the feature export, a head-only optimizer trace against
torch.optim.AdamW + CosineAnnealingLR, and the train / evaluate / extract loop."""
import functools
import math
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_precision import _randomize, relerr
from tests.test_gpu_recompute import _grad_mismatches

pytestmark = pytest.mark.gpu
NAME, NCLS = "tiny_vit_5m_224", 7


def _classifier(precision, seed=31, num_classes=NCLS, **kw):
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TinyViTClassifier(NAME, num_classes=num_classes, precision=precision, seed=seed, **kw)
    _randomize(m.backbone, seed + 1)                   # away from timm's init (zero conv3 BatchNorm gammas, zero biases): every gradient is non-trivial
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        m.head.fc.weight.copy_(0.05 * torch.randn(m.head.fc.weight.shape, generator=g))
        m.head.fc.bias.copy_(0.1 * torch.randn(m.head.fc.bias.shape, generator=g))
    return m.cuda()


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(2, 3, 224, 224, generator=g), torch.tensor([3, 5])


def _policy(model, policy):
    if policy == "ref-freeze":
        model.freeze_all_but_last_stage()
    return model


@functools.lru_cache(maxsize=None)
def _oracle_step(policy, emulate_bf16):
    """One CPU step from the state of _classifier(seed 31): computed once per (policy, arithmetic), shared by the modes that start from the same weights."""
    from oracle import tinyvit_ref as R
    m = _policy(_classifier("fp32"), policy)
    trainable = [n for n, p in m.backbone.named_parameters() if p.requires_grad]
    st = {k: v.detach().cpu().clone() for k, v in m.backbone.state_dict().items()}
    st = {k: (t.requires_grad_(True) if (t.is_floating_point() and "running" not in k and k in trainable) else t) for k, t in st.items()}
    W = m.head.fc.weight.detach().cpu().clone().requires_grad_(True)
    b = m.head.fc.bias.detach().cpu().clone().requires_grad_(True)
    x, y = _inputs()
    cfg = R.config_for(NAME)
    q = (lambda t: t.to(torch.bfloat16).float()) if emulate_bf16 else (lambda t: t)
    emb = R.forward(cfg, st, x, training=True, emulate_bf16=emulate_bf16)
    logits = F.linear(q(emb), q(W), b)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = {k: t.grad for k, t in st.items() if t.requires_grad and t.grad is not None}
    grads["head.fc.weight"], grads["head.fc.bias"] = W.grad, b.grad
    return dict(emb=emb.detach(), logits=logits.detach(), loss=float(loss), grads=grads, trainable=trainable)


def _device_step(precision, policy, **kw):
    m = _policy(_classifier(precision, **kw), policy).train()
    x, y = _inputs()
    emb = m.backbone(x.cuda())
    logits = m.forward_head(emb)
    loss, rank = m.loss_and_metrics(logits, y.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return m, emb.detach(), logits.detach(), loss.detach(), rank


def _param(m, name):
    return m.head.fc.weight if name == "head.fc.weight" else m.head.fc.bias if name == "head.fc.bias" else m.backbone._params[name]


def _grad_table(m, ref, tol, label, median_tol=None, exact=None):
    """tests/test_gpu_precision.py::_grad_table for the classifier: per-tensor rel-L2.  A parameter whose effect is cancelled downstream -- the last
    ``mlp.fc2.bias`` of stages 1 and 2 sits in front of PatchMerging's 1 x 1 conv + train-mode BatchNorm, which removes any per-channel constant -- has a
    gradient of exactly zero in exact arithmetic; what either side holds is its own rounding noise, and a relative error between two noises means nothing.
    Those tensors are recognised in the EXACT-arithmetic oracle (``exact``: the fp32 step; ``ref`` itself when that is the fp32 step), where the noise is
    ~1e-8 and falls under the floor 1e-4 x the median gradient norm, never by what the device returns.  For them the device's gradient must be noise too:
    at most 10 x the larger of the floor and the norm the compared oracle itself holds for that tensor (the bf16-emulating oracle's noise is 2^-9-sized,
    not 1e-8-sized).  Every other tensor is held to ``tol``."""
    exact = ref if exact is None else exact
    floor_exact = 1e-4 * float(np.median([float(g.norm()) for g in exact["grads"].values()]))
    floor = 1e-4 * float(np.median([float(g.norm()) for g in ref["grads"].values()]))
    rows, cancelled = [], []
    for name, gref in ref["grads"].items():
        p = _param(m, name)
        assert p.grad is not None, name
        if float(exact["grads"][name].norm()) > floor_exact:
            rows.append((name, relerr(p.grad, gref)))
        else:
            bound = 10 * max(floor, float(gref.norm()))
            cancelled.append((name, float(p.grad.norm()), float(gref.norm()), bound))
            assert float(p.grad.norm()) < bound, (name, float(p.grad.norm()), float(gref.norm()), floor)
    rows.sort(key=lambda r: -r[1])
    head = {n: e for n, e in rows if n.startswith("head.fc")}
    print(f"[{label}] per-tensor gradient rel-L2 over {len(rows)} tensors: worst {rows[0][0]} {rows[0][1]:.3e}, median {rows[len(rows) // 2][1]:.3e}, head.fc {head}")
    for name, got, want, bound in cancelled:
        print(f"[{label}] analytically zero gradient {name}: device norm {got:.3e}, oracle norm {want:.3e}, bound {bound:.3e}")
    assert all(n.endswith("mlp.fc2.bias") for n, *_ in cancelled), cancelled         # only the biases BatchNorm cancels may take this branch
    assert set(head) == {"head.fc.weight", "head.fc.bias"}
    bad = [r for r in rows if r[1] > tol]
    assert not bad, (label, bad[:8])
    if median_tol is not None:
        assert rows[len(rows) // 2][1] < median_tol, (label, rows[len(rows) // 2])
    assert all(m.backbone._params[n].grad is None for n in m.backbone._params if n not in ref["trainable"])


@pytest.mark.parametrize("precision,policy", [("fp32", "all"), ("fp32_split", "all"), ("fp32", "ref-freeze"), ("fp32_split", "ref-freeze")])
def test_classifier_step_passes_the_fp32_gate(precision, policy):
    ref = _oracle_step(policy, False)
    m, emb, logits, loss, rank = _device_step(precision, policy)
    label = f"classifier {precision} {policy}"
    e_emb, l_rel = relerr(emb, ref["emb"]), abs(float(loss) - ref["loss"]) / ref["loss"]
    print(f"\n[{label}] embedding rel-L2 {e_emb:.3e}, logits rel-L2 {relerr(logits, ref['logits']):.3e}, loss {float(loss):.6f} (oracle {ref['loss']:.6f}, rel {l_rel:.3e})")
    assert e_emb < 1e-4 and l_rel < 1e-5
    _grad_table(m, ref, 2e-3, label)
    zl = ref["logits"].gather(1, _inputs()[1].view(-1, 1))
    assert rank.cpu().tolist() == (ref["logits"] > zl).sum(1).tolist()
    n_train = sum(1 for p in m.backbone.parameters() if p.requires_grad)
    assert (n_train == len(m.backbone._params)) == (policy == "all") and n_train > 0


def test_classifier_step_with_grad_checkpointing_is_bit_equal():
    m0, emb0, logits0, loss0, _ = _device_step("fp32", "all")
    m1, emb1, logits1, loss1, _ = _device_step("fp32", "all", grad_checkpointing=True)
    assert m1.backbone.grad_checkpointing and not m0.backbone.grad_checkpointing
    assert torch.equal(emb0, emb1) and torch.equal(logits0, logits1) and torch.equal(loss0, loss1)
    assert _grad_mismatches(m0.backbone, m0.backbone.flat_grads(), m1.backbone.flat_grads()) == []
    assert float(m0.backbone.flat_grads().abs().sum()) > 0
    for a, b in ((m0.head.fc.weight, m1.head.fc.weight), (m0.head.fc.bias, m1.head.fc.bias)):
        assert float(a.grad.abs().sum()) > 0 and torch.equal(a.grad, b.grad)
    _grad_table(m1, _oracle_step("all", False), 2e-3, "classifier fp32 all, grad_checkpointing")


def test_classifier_bf16_step_matches_bf16_emulating_oracle():
    """Tolerances of test_bf16_mode_train_step_matches_bf16_emulating_oracle: embedding rel-L2 2e-2, loss 2e-3 relative, every gradient tensor 2e-1 with
    the median below 6e-2 -- here with EVERY parameter trainable (that test runs under the reference freeze policy), so the two fc2 biases whose gradient
    BatchNorm cancels to exactly zero are among the tensors: see _grad_table."""
    ref = _oracle_step("all", True)
    m, emb, logits, loss, _ = _device_step("bf16", "all")
    e_emb, l_rel = relerr(emb, ref["emb"]), abs(float(loss) - ref["loss"]) / ref["loss"]
    print(f"\n[classifier bf16 all] embedding rel-L2 {e_emb:.3e}, loss {float(loss):.6f} (oracle {ref['loss']:.6f}, rel {l_rel:.3e})")
    assert e_emb < 2e-2 and l_rel < 2e-3
    _grad_table(m, ref, 2e-1, "classifier bf16 all", median_tol=6e-2, exact=_oracle_step("all", False))


def test_state_dict_is_timms_and_a_foreign_head_is_skipped():
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    m = _classifier("fp32")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        adapter = TinyViTAdapter(NAME, pretrained=False, precision="fp32")
    assert set(m.state_dict()) == {k[len("backbone."):] for k in adapter.state_dict()} | {"head.fc.weight", "head.fc.bias"}
    assert all(v.is_cuda for v in m.state_dict().values())
    other = _classifier("fp32", seed=77, num_classes=11)
    w0, b0 = m.head.fc.weight.detach().clone(), m.head.fc.bias.detach().clone()
    r = m.load_state_dict(other.state_dict(), strict=False)
    assert sorted(r.missing_keys) == ["head.fc.bias", "head.fc.weight"] and not r.unexpected_keys
    assert torch.equal(m.backbone.flat_params, other.backbone.flat_params) and torch.equal(m.backbone._flat_buf, other.backbone._flat_buf)
    assert torch.equal(m.head.fc.weight, w0) and torch.equal(m.head.fc.bias, b0)
    with pytest.raises(RuntimeError, match="head.fc"):
        m.load_state_dict(other.state_dict(), strict=True)
    x = _inputs()[0].cuda()
    m.eval(); other.eval()
    with torch.no_grad():        # the loaded encoder is the one that runs (the weight cache was rebuilt)
        assert torch.equal(m.backbone(x), other.backbone(x))
        assert m(x).shape == (2, NCLS) and other(x).shape == (2, 11)


@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
def test_feature_export(precision):
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    m = _classifier(precision)
    x = _inputs()[0].cuda()
    with pytest.raises(L.GgError, match="eval"):
        m.train().pooled_features(x)
    m.eval()
    logits = m(x)
    fmap = m.forward_features(x)
    pooled = m.pooled_features(x)
    assert fmap.shape == (2, 320, 7, 7) and fmap.dtype == torch.float32 and pooled.shape == (2, 320)
    e = relerr(pooled, fmap.mean(dim=(2, 3)))
    print(f"\n[feature export {precision}] pooled vs mean(forward_features) rel-L2 {e:.3e}")
    assert e < 1e-6                                                  # the same f32 mean of 49 values, summed in another order
    assert torch.equal(m(x), logits)                                 # the export leaves the classifier's own forward alone
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        adapter = TinyViTAdapter(NAME, pretrained=False, features_only=True, precision=precision).cuda().eval()
    adapter.backbone.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("head.fc")})
    with torch.no_grad():
        assert torch.equal(adapter(pixel_values=x).pooler_output, pooled)
    if precision == "fp32":                                          # layout and values of the map against the oracle's last-stage tap
        from oracle import tinyvit_ref as R
        taps = {}
        st = {k: v.detach().cpu() for k, v in m.backbone.state_dict().items()}
        with torch.no_grad():
            R.forward(R.config_for(NAME), st, _inputs()[0], training=False, taps=taps)
        assert taps["stages.3"].shape == fmap.shape and relerr(fmap, taps["stages.3"]) < 2e-4


def test_head_only_trace_matches_torch_adamw_with_cosine_annealing():
    """Backbone frozen in eval mode, 3 epochs x 2 steps: head.fc after EVERY step against torch.optim.AdamW(wd 0.05) + CosineAnnealingLR on the CPU, fed the
    embeddings read back from the device; tolerance of tests/test_gpu_kernels.py::test_adamw_matches_torch (rtol 1e-6, atol 1e-7)."""
    from geoguessr_ai_amd.finetune_tinyvit import cosine_lr
    from geoguessr_ai_amd.optim import AdamW
    epochs, lr = 3, 5e-4
    m = _classifier("fp32").freeze_backbone(eval_mode=True).train()
    assert not m.backbone.training and m.training and not any(p.requires_grad for p in m.backbone.parameters())
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(2, 3, 224, 224, generator=g).cuda(), torch.randint(0, NCLS, (2,), generator=g)) for _ in range(2)]
    flat0 = m.backbone.flat_params.clone()
    W = torch.nn.Parameter(m.head.fc.weight.detach().cpu().clone())
    b = torch.nn.Parameter(m.head.fc.bias.detach().cpu().clone())
    ref_opt = torch.optim.AdamW([W, b], lr=lr, weight_decay=0.05)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(ref_opt, T_max=epochs)
    opt = AdamW(m, lr=lr, weight_decay=0.05)
    assert len(opt.loose) == 2
    worst = 0.0
    for epoch in range(epochs):
        opt.param_groups[0]["lr"] = cosine_lr(epoch, epochs, lr)
        for x, y in batches:
            opt.zero_grad()
            emb = m.backbone(x)
            loss, _ = m.loss_and_metrics(m.forward_head(emb), y.cuda())
            loss.backward()
            opt.step()
            ref_opt.zero_grad()
            ref_loss = F.cross_entropy(F.linear(emb.detach().cpu(), W, b), y)
            ref_loss.backward()
            ref_opt.step()
            assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
            for got, want in ((m.head.fc.weight, W), (m.head.fc.bias, b)):
                d = (got.detach().cpu() - want.detach()).abs()
                worst = max(worst, float(d.max()))
                assert bool((d <= 1e-7 + 1e-6 * want.detach().abs()).all()), (epoch, float(d.max()))
        sched.step()
    print(f"\n[head-only trace] worst |head.fc - torch| over 6 steps {worst:.3e}")
    assert torch.equal(m.backbone.flat_params, flat0) and float((W.detach() - m.head.fc.weight.detach().cpu()).abs().max()) < 1e-6


def test_train_evaluate_extract_loop(tmp_path):
    from geoguessr_ai_amd import finetune_tinyvit as FT
    class_to_id = FT.build_class_map(["NO", "SE", "DK"])
    g = torch.Generator().manual_seed(13)
    batches = [{"pixel_values": torch.randn(2, 3, 224, 224, generator=g).cuda(), "labels": torch.tensor(lab).cuda()} for lab in ([0, 2], [1, 2])]
    m = _classifier("fp32_split", num_classes=3)
    out = FT.train(m, batches, batches, epochs=2, lr=5e-4, weight_decay=0.05, out_dir=str(tmp_path), class_to_id=class_to_id, args=dict(epochs=2, model_name=NAME))
    assert len(out["history"]) == 2 and out["history"][0]["lr"] == 5e-4 and abs(out["history"][1]["lr"] - 2.5e-4) < 1e-12
    assert all(math.isfinite(h["loss"]) and h["loss"] > 0 for h in out["history"])
    ck = torch.load(os.path.join(str(tmp_path), "best.pt"), map_location="cpu")
    assert set(ck) == {"model", "class_to_id", "args"} and ck["class_to_id"] == class_to_id and ck["args"]["model_name"] == NAME
    assert set(ck["model"]) == set(m.state_dict())
    m2, c2 = FT.load_model_for_features(out["best_ckpt"], NAME, precision="fp32_split")
    m2 = m2.cuda()
    assert c2 == class_to_id and m2.num_classes == 3 and not m2.training
    emb = FT.extract_embeddings(m2, batches)
    assert emb.shape == (4, 320) and emb.dtype == np.float32
    assert np.array_equal(emb, torch.cat([m2.pooled_features(b["pixel_values"]) for b in batches]).cpu().numpy())
    df = FT.embeddings_frame(emb, [dict(location_id=i, filepath=f"{i}.jpg", lat=1.0 * i, lon=2.0 * i, country="NO") for i in range(4)])
    assert list(df.columns[:5]) == ["location_id", "filepath", "lat", "lon", "country"] and list(df.columns[5:8]) == ["emb_0", "emb_1", "emb_2"] and df.shape == (4, 325)
    metrics = FT.evaluate(m2, batches)
    with torch.no_grad():
        logits = torch.cat([m2(b["pixel_values"]) for b in batches]).cpu()
    labels = torch.cat([b["labels"] for b in batches]).cpu()
    top1 = 100.0 * float((logits.argmax(1) == labels).float().mean())
    top3 = 100.0 * float((logits.topk(3, 1).indices == labels.view(-1, 1)).any(1).float().mean())        # k = min(5, C) = 3
    assert 0.0 <= metrics["val_top1"] <= 100.0 and metrics == {"val_top1": top1, "val_top5": top3}
    assert metrics["val_top1"] == out["best_top1"]                   # the reloaded best checkpoint scores what the loop recorded for it
