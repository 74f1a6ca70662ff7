"""The JPEG decode with many lanes inside one scan (include/gg_jscan.h, DeviceJpegDecoder(split_bytes=...)) on the GPU: every file of both fixtures, singly and in one
batch, at split_bytes 8, 64 and 512 against Pillow's pixels and against gg_jpeg_decode's bytes; whatever the workspace held; the slow counts against the host
program's (tests/jscan_main.cpp, the lanes' very statements on a CPU) and, at 512 bytes, under a tenth of the sub-segments; truncated and damaged files with the
sequential decoder's status, zeroed, their neighbours intact; and the consumers -- decoder, eval transform, embedder -- against split_bytes = 0."""
import numpy as np
import pytest
import torch

from tests import jpeg_ref as J
from tests.test_jpeg_cpu import load_fixture, truncated
from tests.test_jscan_cpu import build_jscan_exe, host_counts, load_split_fixture

pytestmark = pytest.mark.gpu
TV_MEAN, TV_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SPLITS = [8, 64, 512]


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def both():
    """Both fixtures as one list: files, Pillow's pixels, descriptions, and where the new fixture begins"""
    fx, sx = load_fixture(), load_split_fixture()
    return {"files": fx["files"] + sx["files"], "rgb": fx["rgb"] + sx["rgb"], "desc": fx["desc"] + sx["desc"], "new": len(fx["files"])}


@pytest.fixture(scope="module")
def exe():
    return build_jscan_exe()


def decode_raw(L, files, split, ws_fill=0xA5):
    """One decode call on buffers of this test's own -- gg_jscan_decode, or gg_jpeg_decode for split 0 --, the workspace at exactly the queried size and holding
    ws_fill bytes, the output holding 0xA5 -> images, status, slow (None for split 0)"""
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    plan = JpegPlan(files, split_bytes=split)
    plan.require_accepted()
    host = torch.empty(plan.stream_bytes, dtype=torch.uint8)
    plan.fill(host.data_ptr())
    stream_buf = host.cuda()
    ws = torch.full((plan.workspace_bytes,), ws_fill, dtype=torch.uint8, device="cuda")
    out = torch.full((plan.output_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((plan.B,), -1, dtype=torch.int32, device="cuda")
    slow = torch.full((plan.B,), -1, dtype=torch.int32, device="cuda") if split else None
    if split:
        L.check(L.lib().gg_jscan_decode(plan.handle, stream_buf.data_ptr(), stream_buf.numel(), out.data_ptr(), out.numel(), status.data_ptr(), slow.data_ptr(),
                                        ws.data_ptr(), ws.numel(), L.stream()), "gg_jscan_decode")
    else:
        L.check(L.lib().gg_jpeg_decode(plan.handle, stream_buf.data_ptr(), stream_buf.numel(), out.data_ptr(), out.numel(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                       L.stream()), "gg_jpeg_decode")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    imgs = [o[i.out_offset:i.out_offset + 3 * i.height * i.width].reshape(i.height, i.width, 3) for i in plan.info]
    gaps = np.ones(len(o), bool)
    for i in plan.info:
        gaps[i.out_offset:i.out_offset + 3 * i.height * i.width] = False
    assert (o[gaps] == 0xA5).all()                                           # the alignment gaps between the images are not touched
    subs = plan.subsegments
    plan.close()
    return imgs, status.cpu().numpy(), (slow.cpu().numpy() if split else None), subs


@pytest.fixture(scope="module")
def sequential(L, both):
    """gg_jpeg_decode's bytes of every file, one batch, computed once"""
    imgs, status, _, _ = decode_raw(L, both["files"], 0)
    assert not status.any()
    return imgs


@pytest.mark.parametrize("split", SPLITS)
def test_every_file_singly_and_in_one_batch_equals_pillow_and_the_sequential_decoder(L, both, sequential, exe, split):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    files = both["files"]
    dec = DeviceJpegDecoder("cuda", split_bytes=split)
    p = dec.decode(files)
    assert p.status.cpu().tolist() == [0] * len(files) and p.slow.dtype == torch.int32 and p.slow.shape == (len(files),)
    for i, got in enumerate(dec.unpack(p)):
        g = got.cpu().numpy()
        assert np.array_equal(g, both["rgb"][i]) and np.array_equal(g, sequential[i]), (split, i, both["desc"][i])
    want = host_counts(exe, files, split)                                    # the host program's counts, exactly
    assert p.slow.cpu().tolist() == [w[1] for w in want] and [w[0] for w in want] == [0] * len(files)
    for i, f in enumerate(files):
        q = dec.decode([f])
        assert int(q.status[0]) == 0 and int(q.slow[0]) == want[i][1] and np.array_equal(dec.unpack(q)[0].cpu().numpy(), both["rgb"][i]), (split, i, both["desc"][i])
    if split == 512:                                                         # the speculative lanes, and not only the slow path, produced the result
        from geoguessr_ai_amd.training.jpeg import JpegPlan
        plan = JpegPlan(files, split_bytes=512)
        for i in range(both["new"], len(files)):
            assert plan.subsegments[i] == want[i][2] >= 4 and 10 * int(p.slow[i]) <= plan.subsegments[i], (both["desc"][i], plan.subsegments[i], int(p.slow[i]))
        plan.close()


@pytest.mark.parametrize("split", SPLITS)
def test_the_result_does_not_depend_on_what_the_workspace_held(L, both, sequential, split):
    runs = [decode_raw(L, both["files"], split, fill) for fill in (0xFF, 0x00)]
    for imgs, status, slow, _ in runs:
        assert not status.any() and (slow >= 0).all()
        for i, (got, want) in enumerate(zip(imgs, sequential)):
            assert np.array_equal(got, want), (split, i, both["desc"][i])
    assert np.array_equal(runs[0][2], runs[1][2])


def damaged(f, seed):
    """f with one byte of its entropy-coded data changed so that no marker appears (the plan would end the scan there) and the sequential decode fails"""
    from tests.test_jscan_cpu import _segments
    rng = np.random.default_rng(seed)
    b, e = J.parse(f)["segments"][0]
    for _ in range(200):
        at, v = int(rng.integers(b + 16, e - 16)), int(rng.integers(0, 255))
        if f[at - 1] == 0xFF or f[at] == 0xFF:
            continue
        g = f[:at] + bytes([v]) + f[at + 1:]
        p, segs = _segments(g)
        coef = np.zeros((segs[0][1] * p["bpm"], 64), np.int16)
        blocks = [p["hs"] * p["vs"], 1, 1][:p["ncomp"]]
        if len(segs) == len(_segments(f)[1]) and J.segment_coefficients(segs[0][0], segs[0][1], p["ncomp"], blocks, p["dc"], p["ac"], coef) != 0:
            return g
    raise AssertionError("no damaging byte found")


@pytest.mark.parametrize("split", [64, 512])
def test_truncated_and_damaged_files_have_the_sequential_status_and_are_zeroed(L, both, sequential, exe, split):
    n, files = both["new"], both["files"]
    bad = {1: truncated(files[n + 0]), 3: truncated(files[n + 3]), 4: truncated(files[20]),
           6: damaged(files[n + 2], 1), 8: damaged(files[n + 4], 2), 9: damaged(files[n + 7], 3)}
    good = {0: n + 1, 2: 30, 5: n + 8, 7: n + 5, 10: 50}
    batch = [bad[b] if b in bad else files[good[b]] for b in range(11)]
    _, seq_status, _, _ = decode_raw(L, batch, 0)
    imgs, status, slow, _ = decode_raw(L, batch, split)
    assert status.tolist() == seq_status.tolist() and [s != 0 for s in status.tolist()] == [b in bad for b in range(11)], (status, seq_status)
    want = host_counts(exe, batch, split)
    assert status.tolist() == [w[0] for w in want] and slow.tolist() == [w[1] for w in want]
    for b in range(11):
        if b in bad:
            assert imgs[b].size > 0 and not imgs[b].any(), b
        else:
            assert np.array_equal(imgs[b], sequential[good[b]]), b
    again, status2, _, _ = decode_raw(L, batch, split, 0x00)                 # the zeros do not come from what the workspace held
    assert status2.tolist() == status.tolist() and all(np.array_equal(a, b) for a, b in zip(again, imgs))


def test_decoder_transform_and_embedder_give_what_split_bytes_0_gives(L, both):
    import warnings
    from geoguessr_ai_amd import finetune_tinyvit as FT
    from geoguessr_ai_amd.finetune_tinyvit.augment import DeviceTrainTransform, sample_params
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    from geoguessr_ai_amd.training.preprocess import DeviceEvalTransform, images_to_pixel_values
    files = both["files"][both["new"]:]
    d0, d1 = DeviceJpegDecoder("cuda"), DeviceJpegDecoder("cuda", split_bytes=512)
    a, b = d0.decode(files), d1.decode(files)
    assert a.slow is None and b.slow is not None and a.sizes == b.sizes and np.array_equal(a.offsets, b.offsets)
    assert all(torch.equal(x, y) for x, y in zip(d0.unpack(a), d1.unpack(b)))            # the images' own bytes: the gaps between them belong to nobody
    t0, t1 = DeviceEvalTransform(32, TV_MEAN, TV_STD, "timm", 0.95), DeviceEvalTransform(32, TV_MEAN, TV_STD, "timm", 0.95, jpeg_split_bytes=512)
    x0, x1 = t0(files), t1(files)
    assert t1._decoder.split_bytes == 512 and t0._decoder.split_bytes == 0 and torch.equal(x0, x1)
    assert torch.equal(x0, images_to_pixel_values(files, 32, TV_MEAN, TV_STD, "cuda", crop_pct=0.95, batched=True, jpeg_split_bytes=512))
    sizes = [(r.shape[0], r.shape[1]) for r in both["rgb"][both["new"]:]]
    params = sample_params(sizes, 32, "rand-m9-mstd0.5-inc1", np.random.default_rng(3), TV_MEAN, "bicubic")
    assert torch.equal(DeviceTrainTransform(32, seed=0)(files, params=params), DeviceTrainTransform(32, seed=0, jpeg_split_bytes=512)(files, params=params))
    raw = [{"images": files, "labels": list(range(len(files)))}]
    ev = FT.eval_transformed(raw, DeviceEvalTransform(32, TV_MEAN, TV_STD, "timm", 0.95), jpeg_split_bytes=512)
    assert ev.transform.jpeg_split_bytes == 512 and torch.equal(list(ev)[0]["pixel_values"], x0) and ev.transform._decoder.split_bytes == 512
    au0, au1 = FT.augmented(raw, DeviceTrainTransform(32, seed=7)), FT.augmented(raw, DeviceTrainTransform(32, seed=7), jpeg_split_bytes=512)
    assert torch.equal(list(au0)[0]["pixel_values"], list(au1)[0]["pixel_values"]) and au1.transform._decoder.split_bytes == 512
    embs = []
    for split in (0, 512):
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            emb = TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", load_checkpoint=False, panorama=True, img_size=32, batch_transform=True, jpeg_split_bytes=split)
        embs.append(emb(files[:5]))
        assert emb._eval_transform()._decoder.split_bytes == split
    assert embs[0].shape == (5, 320) and torch.isfinite(embs[0]).all() and torch.equal(embs[0], embs[1])
    with pytest.raises(ValueError, match="needs batch_transform=True"):
        TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", load_checkpoint=False, img_size=32, jpeg_split_bytes=512)
