"""Writes tests/golden/clip_text_tiny.npz from transformers' own CLIPModel (CPU, fp32, seeded): the fixture of the contrastive pre-training stage
(text tower, projection heads, contrastive loss, three optimizer steps).  Run by hand:  python tests/golden/make_golden_clip_text.py

Model: text 128 / 256 / 2 layers / 2 heads, vocab 64, 77 positions, eos_token_id 63 (not 2: the "first position equal to eos" rule); vision 128 / 256 / 2 / 2,
image 32, patch 8; projection 64.  A second text config with eos_token_id = 2 (the argmax rule) shares the weights.

Storage: the large weight matrices are drawn ON a grid of 2^-11 (|k| <= 127) and stored as int8 (`q.<name>`, value = k * 2^-11, exact in fp32); everything
else is float32 (`w.<name>`).  Gradients of matrices beyond 8192 elements are written, whole, to a second file, clip_text_tiny_grads.npz (both files stay below 1 MiB).  `decode_state_dict` (tests/clip_text_golden.py) turns both back into the state dict."""
import os

import numpy as np
import torch
from transformers import CLIPConfig, CLIPModel

HERE = os.path.dirname(os.path.abspath(__file__))
SCALE = 2.0 ** -11
PRETRAIN = dict(betas=(0.9, 0.98), eps=1e-6, weight_decay=1e-3, lr=1e-3, max_grad_norm=1.0)      # PRETRAIN_ARGS' optimizer; lr raised so that three steps show in f32


def build(eos_token_id):
    cfg = CLIPConfig(
        text_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, vocab_size=64, max_position_embeddings=77,
                         eos_token_id=eos_token_id, bos_token_id=0, pad_token_id=1, hidden_act="quick_gelu", projection_dim=64),
        vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=8,
                           hidden_act="quick_gelu", projection_dim=64),
        projection_dim=64)
    cfg._attn_implementation = "eager"
    return CLIPModel(cfg).float().eval()


def main():
    torch.manual_seed(0)
    model = build(63)
    g = torch.Generator().manual_seed(1234)
    store, big = {}, {}
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.numel() > 1024:
                k = torch.clamp(torch.round(torch.randn(p.shape, generator=g) * 0.05 / SCALE), -127, 127)
                p.copy_(k * SCALE)
                store["q." + name] = k.numpy().astype(np.int8)
            else:
                if p.dim() == 1 and "norm" in name:
                    p.copy_((1.0 + 0.1 * torch.randn(p.shape, generator=g)) if name.endswith("weight") else 0.1 * torch.randn(p.shape, generator=g))
                elif p.dim() == 1:
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
                store["w." + name] = p.detach().numpy().astype(np.float32).copy()
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}

    # 5 x 9 ids, right-padded (pad id 1) at different lengths; row 1 has EOS at position 1, row 4 is full length.  Ordinary tokens 2..61; 62 < 63 = EOS.
    lens = [6, 2, 4, 8, 9]
    ids = torch.ones(5, 9, dtype=torch.int64)
    mask = torch.zeros(5, 9, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids[b, 0] = 0
        if n > 2:
            ids[b, 1:n - 1] = torch.randint(2, 62, (n - 2,), generator=g)
        ids[b, n - 1] = 63
        mask[b, :n] = 1
    # the eos_token_id = 2 twin: same rows with the EOS written as the vocabulary's highest id -- already the case (63 is the row maximum): argmax finds it
    pix = torch.randn(5, 3, 32, 32, generator=g)
    store.update(input_ids=ids.numpy(), attention_mask=mask.numpy(), pixel_values=pix.numpy().astype(np.float32), eos_pos=np.array([n - 1 for n in lens], np.int32))

    with torch.no_grad():
        out = model(input_ids=ids, pixel_values=pix, attention_mask=mask, return_loss=True)
        out_nomask = model(input_ids=ids, pixel_values=pix, return_loss=True)
        assert float((out.text_embeds - out_nomask.text_embeds).abs().max()) == 0.0, "right-padding must not reach the pooled row"
        twin = build(2)
        twin.load_state_dict(sd0)
        out2 = twin(input_ids=ids, pixel_values=pix, attention_mask=mask, return_loss=True)
        assert float((out2.text_embeds - out.text_embeds).abs().max()) == 0.0, "argmax rule and first-eos rule must pool the same rows here"
        tout = model.text_model(input_ids=ids, attention_mask=mask)          # the tower itself: pooler_output before the projection
        vout = model.vision_model(pixel_values=pix)
        assert tout.pooler_output.shape == (5, 128) and vout.pooler_output.shape == (5, 128)
    store.update(text_last_hidden=tout.last_hidden_state.numpy(), text_pooled=tout.pooler_output.numpy(),
                 image_pooled=vout.pooler_output.numpy(), text_embeds=out.text_embeds.numpy(), image_embeds=out.image_embeds.numpy(),
                 logits_per_image=out.logits_per_image.numpy(), logits_per_text=out.logits_per_text.numpy(), loss=np.float32(out.loss.item()))

    masks = {
        "ref": lambda n: "visual_projection" in n or n == "logit_scale",
        "ref_text": lambda n: "visual_projection" in n or n == "logit_scale" or "text_projection" in n,
        "ref_vis": lambda n: "visual_projection" in n or n == "logit_scale" or n.startswith("vision_model.encoder.layers.1.") or n.startswith("vision_model.post_layernorm"),
    }
    for mname, sel in masks.items():
        model.zero_grad(set_to_none=True)
        for n, p in model.named_parameters():
            p.requires_grad = bool(sel(n))
        model(input_ids=ids, pixel_values=pix, attention_mask=mask, return_loss=True).loss.backward()
        for n, p in model.named_parameters():
            if p.requires_grad:
                gr = p.grad.detach()
                if gr.numel() <= 8192:
                    store[f"grad.{mname}.{n}"] = gr.numpy().astype(np.float32).copy()
                else:      # the big matrices go to a file of their own (each file stays below 1 MiB)
                    big[f"grad.{mname}.{n}"] = gr.numpy().astype(np.float32).copy()

    # three optimizer steps under the reference's mask
    model.load_state_dict(sd0)
    model.zero_grad(set_to_none=True)
    for n, p in model.named_parameters():
        p.requires_grad = bool(masks["ref"](n))
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=PRETRAIN["lr"], betas=PRETRAIN["betas"], eps=PRETRAIN["eps"], weight_decay=PRETRAIN["weight_decay"])
    losses, scales, norms = [], [], []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        loss = model(input_ids=ids, pixel_values=pix, attention_mask=mask, return_loss=True).loss
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, PRETRAIN["max_grad_norm"])))
        opt.step()
        losses.append(float(loss.detach()))
        scales.append(float(model.logit_scale))
    assert norms[0] > 1.0, f"clipping must be active on step 1 (norm {norms[0]})"
    store.update(trace_loss=np.array(losses, np.float64), trace_logit_scale=np.array(scales, np.float64), trace_norm=np.array(norms, np.float64),
                 trace_visual_projection=model.visual_projection.weight.detach().numpy().copy())
    path = os.path.join(HERE, "clip_text_tiny.npz")
    np.savez_compressed(path, **store)
    np.savez_compressed(os.path.join(HERE, "clip_text_tiny_grads.npz"), **big)
    print("clip_text_tiny_grads.npz:", os.path.getsize(os.path.join(HERE, "clip_text_tiny_grads.npz")) / 1e6, "MB,", len(big), "tensors")
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB; loss {losses}, logit_scale {scales}, norms {norms}")


if __name__ == "__main__":
    main()
