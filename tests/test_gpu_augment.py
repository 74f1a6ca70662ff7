"""The device-side training transform (include/gg_aug.h, csrc/augment.hip, finetune_tinyvit/augment.py) on the GPU: dst_u8 BYTE-IDENTICAL to Pillow's own outputs
(tests/golden/augment_pil.npz) for every stored case and to the numpy restatement (tests/augment_ref.py, itself held to the golden in tests/test_augment_cpu.py) on
fresh random records; dst bit-identical to torch's float32 normalisation; batch invariance, workspace reuse, refusals, and one end-to-end fine-tune epoch from raw
uint8 images.  Sizes: sources 50x50, 61x83, 96x64, S = 32, B <= 6."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_pil.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def sources():
    g = golden()
    return [g["src0"], g["src1"], g["src2"]]


def run(srcs, recs, S, flt, workspace=None, fill_workspace=None, want_u8=True, sentinel=None, expect_error=None, workspace_bytes=None):
    """One gg_aug_batch call through the C ABI on tightly packed (ragged) sources.  Returns (dst (B,3,S,S) f32, dst_u8 (B,S,S,3) u8) as CPU tensors."""
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.finetune_tinyvit.augment import RECORD_DTYPE
    L.require_gpu()
    recs = np.array(recs, RECORD_DTYPE)                    # a copy: it is wiped below
    B = len(srcs)
    sizes = [3 * s.shape[0] * s.shape[1] for s in srcs]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    packed = torch.from_numpy(np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in srcs])).cuda()
    heights, widths = np.array([s.shape[0] for s in srcs], np.int32), np.array([s.shape[1] for s in srcs], np.int32)
    dst = torch.full((B, 3, S, S), float("nan") if sentinel is None else sentinel, dtype=torch.float32, device="cuda")
    dst_u8 = torch.full((B, S, S, 3), 0xA5, dtype=torch.uint8, device="cuda") if want_u8 else None
    a = L.AugArgs()
    a.src, a.src_bytes = packed.data_ptr(), packed.numel()
    a.offsets, a.heights, a.widths = offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data
    a.B, a.S, a.filter = B, S, flt
    a.mean, a.std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    a.records = recs.ctypes.data
    need = L.lib().gg_aug_workspace_bytes(C.byref(a))
    if workspace is None:
        workspace = torch.full((max(need, 256),), 0 if fill_workspace is None else fill_workspace, dtype=torch.uint8, device="cuda")
    a.dst, a.dst_u8 = dst.data_ptr(), dst_u8.data_ptr() if want_u8 else None
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() if workspace_bytes is None else workspace_bytes
    rc = L.lib().gg_aug_batch(C.byref(a), L.stream())
    recs[...] = np.zeros((), RECORD_DTYPE)                 # the library does not read the host table after the call returns
    torch.cuda.synchronize()
    if expect_error is not None:
        msg = L.lib().gg_last_error().decode()
        assert rc != 0 and expect_error in msg, (rc, msg)
        assert need == -1 or workspace_bytes is not None
        assert bool(torch.isnan(dst).all()) and bool((dst_u8 == 0xA5).all())          # outputs untouched
        return None
    L.check(rc, "gg_aug_batch")
    return dst.cpu(), dst_u8.cpu() if want_u8 else None


def blank(n):
    from geoguessr_ai_amd.finetune_tinyvit.augment import RECORD_DTYPE
    rec = np.zeros(n, RECORD_DTYPE)
    rec["ops"]["m"][...] = [1, 0, 0, 0, 1, 0]
    rec["ops"]["resample"] = 3
    rec["ops"]["factor"] = 1.0
    return rec


def golden_record(g, i):
    rec = blank(1)[0]
    rec["top"], rec["left"], rec["h"], rec["w"] = (int(v) for v in g["case_box"][i])
    rec["flip"], rec["num_layers"] = int(g["case_flip"][i]), int(g["case_layers"][i])
    for l in range(int(g["case_layers"][i])):
        o = rec["ops"][l]
        o["op"], o["applied"], o["iarg"], o["factor"] = int(g["case_op"][i]), 1, int(g["case_iarg"][i]), g["case_factor"][i]
        o["m"], o["resample"], o["fill"] = g["case_m"][i], int(g["case_resample"][i]), g["fill"]
    return rec


def test_every_golden_case_is_byte_identical_to_pillow():
    """All 102 stored cases (12 crop / resize / flip, 90 op slots), in batches of up to 6 images that share the resize filter."""
    g, srcs = golden(), sources()
    S, n = int(g["S"]), len(g["case_op"])
    bad = []
    for flt in (2, 3):
        idx = [i for i in range(n) if int(g["case_filter"][i]) == flt]
        for k in range(0, len(idx), 6):
            chunk = idx[k:k + 6]
            recs = np.stack([golden_record(g, i) for i in chunk])
            _, u8 = run([srcs[int(g["case_src"][i])] for i in chunk], recs, S, flt)
            for j, i in enumerate(chunk):
                d = int((u8[j].numpy() != g["out"][i]).sum())
                if d:
                    bad.append((i, int(g["case_op"][i]), d))
    assert not bad, f"(case, op, differing bytes): {bad}"


def ragged_batch():
    srcs = sources()
    g = np.random.default_rng(77)
    return srcs + [g.integers(0, 256, (64, 96, 3), dtype=np.uint8), np.ascontiguousarray(srcs[1][::-1, :, ::-1])]


def sampled(srcs, S, n, seed, interpolation="random"):
    from geoguessr_ai_amd.finetune_tinyvit.augment import sample_params
    return sample_params([s.shape[:2] for s in srcs], S, f"rand-m9-mstd0.5-inc1-n{n}", np.random.default_rng(seed), MEAN, interpolation)


def reference(srcs, recs, S, flt):
    return np.stack([R.apply_record(s, r, S, flt) for s, r in zip(srcs, recs)])


@pytest.mark.parametrize("layers,flt,seed", [(2, 3, 1), (2, 2, 2), (0, 3, 3), (1, 2, 4), (4, 3, 5), (4, 2, 6)])
def test_random_records_match_the_restatement_and_torch_normalisation(layers, flt, seed):
    """Fresh random records over a ragged batch of 5 (every op slot forced to `applied` on the 4-layer cases so that the ops really run)."""
    srcs, S = ragged_batch(), 32
    recs = sampled(srcs, S, layers, seed)
    if layers == 4:
        recs["ops"]["applied"] = 1
    want = reference(srcs, recs, S, flt)
    dst, u8 = run(srcs, recs, S, flt)
    assert np.array_equal(u8.numpy(), want), [int((u8[b].numpy() != want[b]).sum()) for b in range(len(srcs))]
    x = u8.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    ref = (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    assert torch.equal(dst, ref)
    assert np.array_equal(dst.numpy(), R.normalise(want, MEAN, STD))


def test_every_op_runs_next_to_every_other_in_one_batch():
    """15 images' worth of single-op records (three batches of 5, one op each, both resample codes across the batch) against the restatement: op dispatch per image."""
    from geoguessr_ai_amd.finetune_tinyvit import augment as A
    srcs, S = ragged_batch(), 32
    for k in range(3):
        recs = sampled(srcs, S, 1, 40 + k)
        for b in range(5):
            name = A.RAND_INCREASING_OPS[5 * k + b]
            o = recs[b]["ops"][0]
            o["op"], o["applied"], o["resample"] = A.OP_IDS[name], 1, 2 + (b & 1)
            for key, v in A.level_to_arg(name, 7.5, -1.0 if b & 1 else 1.0, S).items():
                o[key] = v
        want = reference(srcs, recs, S, 3)
        _, u8 = run(srcs, recs, S, 3)
        assert np.array_equal(u8.numpy(), want), k


def test_unapplied_slots_pass_through_and_the_flip_mirrors():
    srcs, S = ragged_batch(), 32
    recs = sampled(srcs, S, 2, 11)
    recs["ops"]["applied"] = 0
    recs["flip"] = [0, 1, 0, 1, 1]
    _, u8 = run(srcs, recs, S, 3)
    plain = np.stack([R.crop_resize_flip(s, int(r["top"]), int(r["left"]), int(r["h"]), int(r["w"]), S, 3, False) for s, r in zip(srcs, recs)])
    for b in range(5):
        assert np.array_equal(u8[b].numpy(), plain[b][:, ::-1] if recs["flip"][b] else plain[b]), b
    recs["flip"] = 1 - recs["flip"]
    _, u8b = run(srcs, recs, S, 3)
    assert np.array_equal(u8b.numpy(), u8.numpy()[:, :, ::-1])


def test_an_image_does_not_depend_on_its_batch():
    srcs, S = ragged_batch(), 32
    recs = sampled(srcs, S, 2, 21)
    recs["ops"]["applied"] = 1
    recs[3]["ops"][0]["op"], recs[3]["ops"][1]["op"] = R.EQUALIZE, R.CONTRAST           # the two ops with batch-wide scratch (bins, grey sum)
    dst, u8 = run(srcs, recs, S, 3)
    dst1, u81 = run(srcs[3:4], recs[3:4].copy(), S, 3)
    assert torch.equal(u8[3], u81[0]) and torch.equal(dst[3], dst1[0])


def test_a_reused_workspace_gives_what_fresh_ones_give():
    from geoguessr_ai_amd import _lib as L
    srcs, S = ragged_batch(), 32
    ra, rb = sampled(srcs, S, 2, 31), sampled(srcs[::-1], S, 4, 32)
    ra["ops"]["applied"] = 1
    rb["ops"]["applied"] = 1
    ra[0]["ops"][0]["op"], rb[0]["ops"][0]["op"], rb[1]["ops"][1]["op"] = R.AUTO_CONTRAST, R.EQUALIZE, R.CONTRAST
    fresh_a = run(srcs, ra, S, 3, fill_workspace=0xFF)
    fresh_b = run(srcs[::-1], rb, S, 2, fill_workspace=0x47)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    again_a = run(srcs, ra, S, 3, workspace=ws)
    again_b = run(srcs[::-1], rb, S, 2, workspace=ws)
    again_a2 = run(srcs, ra, S, 3, workspace=ws)
    for x, y in ((fresh_a, again_a), (fresh_b, again_b), (fresh_a, again_a2)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    assert np.array_equal(fresh_a[1].numpy(), reference(srcs, ra, S, 3)) and np.array_equal(fresh_b[1].numpy(), reference(srcs[::-1], rb, S, 2))


def test_bad_records_are_refused_by_name_with_the_outputs_untouched():
    srcs, S = ragged_batch(), 32
    good = sampled(srcs, S, 2, 51)
    good["ops"]["applied"] = 1
    good[2]["ops"][1]["op"] = R.SHEAR_X

    def bad(edit):
        r = good.copy()
        edit(r)
        return r

    def box(r): r[1]["top"] = 61 - int(r[1]["h"]) + 1
    def wide(r): r[4]["left"], r[4]["w"] = 80, 4
    def op(r): r[0]["ops"][1]["op"] = 15
    def neg(r): r[0]["ops"][0]["op"] = -1
    def resample(r): r[2]["ops"][1]["resample"] = 1
    def layers(r): r[3]["num_layers"] = 5
    for edit, msg in ((box, "record 1: the box"), (wide, "record 4: the box"), (op, "record 0 slot 1: unknown op id 15"), (neg, "record 0 slot 0: unknown op id -1"),
                      (resample, "record 2 slot 1: resample must be 2 or 3, got 1"), (layers, "record 3: num_layers=5")):
        run(srcs, bad(edit), S, 3, expect_error=msg)
    run(srcs, good, S, 4, expect_error="filter must be 2")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    from geoguessr_ai_amd import _lib as L
    run(srcs, good, S, 3, workspace=ws, workspace_bytes=1024, expect_error="the workspace has 1024 bytes, the batch needs")
    assert run(srcs, good, S, 3, workspace=ws) is not None


def test_transform_feeds_one_fine_tune_epoch_from_raw_images(tmp_path):
    """DeviceTrainTransform on 8 raw images of two sizes -> augmented -> train for one epoch of one batch of tiny_vit_5m_224: finite loss, best.pt written; an
    explicit `params` replays the batch bit for bit."""
    import warnings
    from geoguessr_ai_amd import finetune_tinyvit as FT
    from geoguessr_ai_amd.models.tinyvit_classifier import TinyViTClassifier
    g = np.random.default_rng(5)
    images = [g.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(4)] + [g.integers(0, 256, (300, 260, 3), dtype=np.uint8) for _ in range(4)]
    tfm = FT.DeviceTrainTransform(img_size=224, seed=3)
    pv, u8 = tfm(images, return_u8=True)
    assert pv.shape == (8, 3, 224, 224) and pv.dtype == torch.float32 and pv.is_cuda and u8.shape == (8, 224, 224, 3)
    params = tfm.last_params
    assert len(params) == 8 and all(0 <= r["top"] and r["top"] + r["h"] <= im.shape[0] and r["left"] + r["w"] <= im.shape[1] for r, im in zip(params, images))
    want = R.apply_record(images[5], params[5], 224, 3)
    assert np.array_equal(u8[5].cpu().numpy(), want)
    pv2 = tfm(torch.from_numpy(np.stack(images[:4])).permute(0, 3, 1, 2), params=params[:4])
    assert torch.equal(pv2, pv[:4])
    raw = [{"images": images, "labels": torch.tensor([0, 1, 2, 0, 1, 2, 0, 1])}]
    val = [{"pixel_values": pv, "labels": raw[0]["labels"].cuda()}]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = TinyViTClassifier("tiny_vit_5m_224", num_classes=3, precision="fp32_split", seed=1).cuda()
    out = FT.train(model, FT.augmented(raw, tfm), val, epochs=1, out_dir=str(tmp_path))
    assert len(out["history"]) == 1 and math.isfinite(out["history"][0]["loss"]) and out["history"][0]["loss"] > 0
    assert os.path.exists(os.path.join(str(tmp_path), "best.pt"))
