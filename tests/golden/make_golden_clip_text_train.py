"""Writes tests/golden/clip_text_train_grads_*.npz from transformers' own CLIPModel (CPU, seeded): the fixture of text-tower training.  Run by hand:
    python tests/golden/make_golden_clip_text_train.py

Model, weights and inputs are those of clip_text_tiny.npz (loaded through tests/clip_text_golden.py; the stored loss must be reproduced exactly).
* Gradients: ONE backward with every parameter trainable, every tensor's gradient stored as `grad.<HF name>` (a tensor's gradient does not depend on which other
  tensors train, so this serves every mask).  Split by tower and layer so that each file stays below 1 MiB: _text_l0, _text_l1, _text_rest (embeddings,
  final_layer_norm), _vision_l0, _vision_l1, _vision_rest, _head (projections, logit_scale).
* _trace: three AdamW steps with everything trainable under PRETRAIN's optimizer settings (make_golden_clip_text.py) with gradient clipping -- loss, norm
  (before clipping) and logit_scale per step, the final text_projection.weight and text_model.embeddings.token_embedding.weight -- once from the f32 model
  (`trace32_*`) and once from model.double() (`trace64_*`): their difference is the reference's own rounding yardstick."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from tests import clip_text_golden as G          # noqa: E402
from make_golden_clip_text import PRETRAIN, build          # noqa: E402


def group(name):
    for tower, tag in (("text_model", "text"), ("vision_model", "vision")):
        if name.startswith(tower + "."):
            if ".encoder.layers." in name:
                return f"{tag}_l{name.split('.encoder.layers.')[1].split('.')[0]}"
            return f"{tag}_rest"
    return "head"


def trace(model, ids, pix, mask, tag, store):
    for p in model.parameters():
        p.requires_grad = True
    params = list(model.parameters())
    opt = torch.optim.AdamW(params, lr=PRETRAIN["lr"], betas=PRETRAIN["betas"], eps=PRETRAIN["eps"], weight_decay=PRETRAIN["weight_decay"])
    losses, scales, norms = [], [], []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = model(input_ids=ids, pixel_values=pix.to(model.logit_scale.dtype), attention_mask=mask, return_loss=True).loss
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, PRETRAIN["max_grad_norm"])))
        opt.step()
        losses.append(float(loss.detach()))
        scales.append(float(model.logit_scale))
    assert norms[0] > 1.0, f"clipping must be active on step 1 (norm {norms[0]})"
    store.update({f"{tag}_loss": np.array(losses, np.float64), f"{tag}_norm": np.array(norms, np.float64), f"{tag}_logit_scale": np.array(scales, np.float64),
                  f"{tag}_text_projection": model.text_projection.weight.detach().numpy().copy(),
                  f"{tag}_token_embedding": model.text_model.embeddings.token_embedding.weight.detach().numpy().copy()})
    print(tag, "loss", losses, "norm", norms, "logit_scale", scales)


def main():
    z = G.load()
    sd = G.decode_state_dict(z)
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    pix = torch.from_numpy(z["pixel_values"])
    torch.manual_seed(0)
    model = build(63)
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
    for p in model.parameters():
        p.requires_grad = True
    out = model(input_ids=ids, pixel_values=pix, attention_mask=mask, return_loss=True)
    assert np.float32(out.loss.item()) == z["loss"], (out.loss.item(), z["loss"])
    out.loss.backward()
    files = {}
    for n, p in model.named_parameters():
        files.setdefault(group(n), {})["grad." + n] = p.grad.detach().numpy().astype(np.float32).copy()
    n_text = sum(v.size for g, d in files.items() if g.startswith("text") for v in d.values())
    print("text-side gradient floats:", n_text)
    # id statistics the GPU test relies on
    flat = ids.flatten().tolist()
    assert flat.count(0) == 5 and 1 in flat
    tr = {}
    model.load_state_dict(sd, strict=False)
    model.zero_grad(set_to_none=True)
    trace(model, ids, pix, mask, "trace32", tr)
    m64 = build(63)
    m64.load_state_dict(sd, strict=False)
    trace(m64.double(), ids, pix, mask, "trace64", tr)
    files["trace"] = tr
    for g, d in files.items():
        path = os.path.join(HERE, f"clip_text_train_grads_{g}.npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(f"{os.path.basename(path)}: {size / 1e6:.3f} MB, {len(d)} arrays")
        assert size < (1 << 20), path


if __name__ == "__main__":
    main()
