"""The device JPEG decoder (include/gg_jpeg.h, geoguessr_ai_amd.training.jpeg) on the GPU: Pillow's own results (tests/golden/jpeg_pil.npz) byte for byte, singly and
in one batch; a batch against its single calls whatever the workspace held; truncated files (the ones tests/test_jpeg_cpu.py passes through the host program)
zeroed with their neighbours intact; and the consumers -- both transforms and both embedders -- fed file bytes against the same fed PIL images."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests.test_jpeg_cpu import fill_byte_files, load_fixture, truncated, truncation_files

pytestmark = pytest.mark.gpu
TV_MEAN, TV_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CL_MEAN, CL_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def singles(L, fx):
    """Every golden decoded in a call of its own, computed once: [(H, W, 3) uint8 arrays]"""
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    dec = DeviceJpegDecoder("cuda")
    out = []
    for f in fx["files"]:
        p = dec.decode([f])
        assert p.offsets.tolist() == [0] and int(p.status[0]) == 0
        out.append(dec.unpack(p)[0].cpu().numpy())
    return out


def decode_raw(L, files, ws_fill):
    """One gg_jpeg_decode call on buffers of this test's own: the workspace at exactly the queried size and holding ws_fill bytes, the output holding 0xA5."""
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    plan = JpegPlan(files)
    plan.require_accepted()
    host = torch.empty(plan.stream_bytes, dtype=torch.uint8)
    plan.fill(host.data_ptr())
    stream_buf = host.cuda()
    ws = torch.full((plan.workspace_bytes,), ws_fill, dtype=torch.uint8, device="cuda")
    out = torch.full((plan.output_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((plan.B,), -1, dtype=torch.int32, device="cuda")
    L.check(L.lib().gg_jpeg_decode(plan.handle, stream_buf.data_ptr(), stream_buf.numel(), out.data_ptr(), out.numel(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                   L.stream()), "gg_jpeg_decode")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    imgs = [o[i.out_offset:i.out_offset + 3 * i.height * i.width].reshape(i.height, i.width, 3) for i in plan.info]
    gaps = np.ones(len(o), bool)
    for i in plan.info:
        gaps[i.out_offset:i.out_offset + 3 * i.height * i.width] = False
    assert (o[gaps] == 0xA5).all()                                           # the alignment gaps between the images are not touched
    plan.close()
    return imgs, status.cpu().numpy()


def test_every_golden_singly_and_in_one_batch_equals_pillow(L, fx, singles):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    for i, (got, want) in enumerate(zip(singles, fx["rgb"])):
        assert got.shape == want.shape and np.array_equal(got, want), (i, fx["desc"][i], int((got != want).sum()))
    dec = DeviceJpegDecoder("cuda")
    files = [fx["files"][0], bytearray(fx["files"][1]), memoryview(fx["files"][2])] + fx["files"][3:]
    p = dec.decode(files)
    assert p.packed.is_cuda and p.packed.dtype == torch.uint8 and p.status.cpu().tolist() == [0] * len(files) and all(o % 256 == 0 for o in p.offsets)
    for i, (got, want) in enumerate(zip(dec.unpack(p), fx["rgb"])):
        assert p.sizes[i] == want.shape[:2] and np.array_equal(got.cpu().numpy(), want), (i, fx["desc"][i])
    again = dec.decode(files[::-1])                                          # the decoder's staging buffer and workspace are reused
    for got, want in zip(dec.unpack(again), fx["rgb"][::-1]):
        assert np.array_equal(got.cpu().numpy(), want)


def test_batch_equals_its_single_calls_whatever_the_workspace_held(L, fx, singles):
    for fill in (0xFF, 0x00):
        imgs, status = decode_raw(L, fx["files"], fill)
        assert status.tolist() == [0] * len(imgs)
        for i, (got, want) in enumerate(zip(imgs, singles)):
            assert np.array_equal(got, want), (fill, i, fx["desc"][i])


def test_larger_images_more_than_one_workgroup_and_many_unique_tables(L):
    """Fresh files a few hundred pixels wide (many blocks per image, restart rows, optimised tables per file) against Pillow, and 400 files with tables of their
    own in one batch: more unique Huffman tables than the LDS path takes, so the kernel that reads them through the cache runs."""
    from PIL import Image
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    rng = np.random.default_rng(5)
    files, want = [], []

    def add(a, **kw):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", **kw)
        files.append(buf.getvalue())
        want.append(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))

    yy, xx = np.mgrid[0:240, 0:301]
    base = np.stack([xx * 0.8, yy, 255 - xx * 0.5 - yy * 0.3], 2)
    big = (base + rng.integers(-30, 30, base.shape)).clip(0, 255).astype(np.uint8)
    add(big, quality=90, subsampling="4:2:0")
    add(big, quality=75, subsampling="4:2:2", restart_marker_rows=1)
    add(big[:, :, 0], quality=95, optimize=True)
    add(np.ascontiguousarray(big.transpose(1, 0, 2)), quality=100, subsampling="4:4:4", restart_marker_blocks=7)
    dec = DeviceJpegDecoder("cuda")
    for got, w in zip(dec.unpack(dec.decode(files)), want):
        assert np.array_equal(got.cpu().numpy(), w)
    files, want = [], []
    for t in range(400):
        add(rng.integers(0, 256, (17 + t % 5, 19 + t % 7, 3)).astype(np.uint8), quality=30 + t % 60, optimize=True, subsampling=("4:2:0", "4:4:4")[t % 2])
    assert len({f[f.index(b"\xff\xc4"):f.index(b"\xff\xda")] for f in files}) > 128          # each differs from the rest in at least one table
    for got, w in zip(dec.unpack(dec.decode(files)), want):
        assert np.array_equal(got.cpu().numpy(), w)


def test_truncated_files_are_zeroed_and_their_neighbours_intact(L, fx, singles):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    t0, t1 = [truncated(f) for f in truncation_files(fx)]
    files = [fx["files"][10], t0, fx["files"][30], fx["files"][31], t1, fx["files"][50]]
    dec = DeviceJpegDecoder("cuda")
    p = dec.decode(files, check=False)
    st = p.status.cpu().tolist()
    assert [s != 0 for s in st] == [False, True, False, False, True, False], st
    imgs = [x.cpu().numpy() for x in dec.unpack(p)]
    assert imgs[1].size > 0 and not imgs[1].any() and not imgs[4].any()
    for b, i in ((0, 10), (2, 30), (3, 31), (5, 50)):
        assert np.array_equal(imgs[b], singles[i])
    for fill in (0xFF, 0x00):                                                # the zeros do not come from what the workspace held
        raw, status = decode_raw(L, files, fill)
        assert status.tolist() == st and not raw[1].any() and not raw[4].any() and np.array_equal(raw[2], singles[30])
    with pytest.raises(L.GgError, match="image 1 failed to decode"):
        dec.decode(files)
    with pytest.raises(L.GgError, match=r"image 2 is refused: progressive \(SOF2\)"):
        dec.decode([files[0], files[2], fx["refuse"][fx["refuse_name"].index("progressive (SOF2)")]])


def test_fill_bytes_in_front_of_markers_and_stuffed_bytes(L, fx):
    """FF fill bytes (one, and runs longer than the reader's window) in front of every restart marker, EOI and stuffed FF 00: Pillow decodes the same picture, and
    so does the device (tests/test_jpeg_cpu.py holds the same files against Pillow itself and the host program)."""
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    filled, plain = fill_byte_files(fx)
    dec = DeviceJpegDecoder("cuda")
    want = {f: fx["rgb"][fx["files"].index(f)] for f in set(plain)}
    for got, g in zip(dec.unpack(dec.decode(filled)), plain):
        assert np.array_equal(got.cpu().numpy(), want[g])


def _big_enough(fx, side):
    from PIL import Image
    idx = [i for i, r in enumerate(fx["rgb"]) if min(r.shape[:2]) >= side][:12]
    return [fx["files"][i] for i in idx], [Image.open(io.BytesIO(fx["files"][i])) for i in idx]


def test_eval_transform_from_file_bytes_equals_from_pil_images(L, fx):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    from geoguessr_ai_amd.training.preprocess import DeviceEvalTransform, images_to_pixel_values
    files, pil = _big_enough(fx, 32)
    assert len(files) == 12 and len({im.size for im in pil}) > 1 and {im.mode for im in pil} == {"RGB", "L"}
    for pipeline, mean, std, pct in (("timm", TV_MEAN, TV_STD, 0.95), ("clip", CL_MEAN, CL_STD, 1.0), ("torchvision", TV_MEAN, TV_STD, 1.0)):
        tfm = DeviceEvalTransform(32, mean, std, pipeline, pct)
        a, a8 = tfm(files, return_u8=True)
        b, b8 = tfm(pil, return_u8=True)
        assert torch.equal(a8, b8) and torch.equal(a, b), pipeline
        c = tfm(DeviceJpegDecoder("cuda").decode(files))                     # the decoder's PackedImages, consumed where it lies
        assert torch.equal(a, c)
        d = images_to_pixel_values(files, 32, mean, std, "cuda", crop_pct=pct, pipeline=pipeline, batched=True)
        assert torch.equal(a, d)
    assert torch.equal(tfm(files[0]), tfm([pil[0]]))                         # one file's bytes on their own
    with pytest.raises(L.GgError):
        images_to_pixel_values(files, 32, TV_MEAN, TV_STD, "cuda")           # the per-image default path keeps refusing byte strings


def test_train_transform_from_file_bytes_equals_from_pil_images_under_fixed_draws(L, fx):
    from geoguessr_ai_amd import finetune_tinyvit as FT
    from geoguessr_ai_amd.finetune_tinyvit.augment import DeviceTrainTransform, sample_params
    files, pil = _big_enough(fx, 32)
    sizes = [(im.size[1], im.size[0]) for im in pil]
    params = sample_params(sizes, 32, "rand-m9-mstd0.5-inc1", np.random.default_rng(3), TV_MEAN, "bicubic")
    tfm = DeviceTrainTransform(32, seed=0)
    a, a8 = tfm(files, params=params, return_u8=True)
    b, b8 = tfm(pil, params=params, return_u8=True)
    assert torch.equal(a8, b8) and torch.equal(a, b)
    x = list(FT.augmented([{"images": files, "labels": list(range(12))}], DeviceTrainTransform(32, seed=7)))
    y = list(FT.augmented([{"images": pil, "labels": list(range(12))}], DeviceTrainTransform(32, seed=7)))
    assert torch.equal(x[0]["pixel_values"], y[0]["pixel_values"])
    from geoguessr_ai_amd.training.preprocess import DeviceEvalTransform
    ev = DeviceEvalTransform(32, TV_MEAN, TV_STD, "timm", 0.95)
    x = list(FT.eval_transformed([{"images": files, "labels": list(range(12))}], ev))
    assert torch.equal(x[0]["pixel_values"], ev(pil))


def test_embedders_give_identical_embeddings_from_bytes_and_from_pil_images(L, fx):
    import warnings
    from PIL import Image
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPEmbedding
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    files, pil = _big_enough(fx, 32)
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        emb = TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", load_checkpoint=False, panorama=True, img_size=32, batch_transform=True)
    a, b = emb(files[:5]), emb(pil[:5])
    assert a.shape == (5, 320) and torch.isfinite(a).all() and torch.equal(a, b)
    p = emb(files[0:2], image_2=files[2:4], image_3=files[4:6], image_4=files[6:8])
    q = emb(pil[0:2], image_2=pil[2:4], image_3=pil[4:6], image_4=pil[6:8])
    assert p.shape == (2, 4, 320) and torch.equal(p, q)
    rng = np.random.default_rng(9)
    big, big_pil = [], []
    for s, kw in (((240, 301), dict(quality=90, subsampling="4:2:0")), ((275, 250), dict(quality=80, subsampling="4:4:4")), ((224, 224), dict(quality=95, subsampling="4:2:2"))):
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, s + (3,), dtype=np.uint8)).save(buf, "JPEG", **kw)
        big.append(buf.getvalue()); big_pil.append(Image.open(io.BytesIO(buf.getvalue())))
    clip = CLIPEmbedding("openai/clip-vit-base-patch32", device="cuda", precision="fp32", num_layers=3, batch_transform=True)
    a, b = clip(big), clip(big_pil)
    assert a.shape == (3, 768) and torch.isfinite(a).all() and torch.equal(a, b)
