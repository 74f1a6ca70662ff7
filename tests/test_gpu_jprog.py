"""The progressive JPEG decode (include/gg_jprog.h, DeviceJpegDecoder(progressive=True)) on the GPU: Pillow's own results (tests/golden/jpeg_prog_pil.npz) byte for
byte, singly and in one batch; a mixed batch with baseline files against its single calls whatever the workspace held, and against gg_jpeg_decode; one large flat
file (the longest EOB run a scan of its size reaches), a few-hundred-pixel file with restart rows, 400 files with tables of their own (the kernel that reads the
tables through the cache); truncated files zeroed with their neighbours intact; and the consumers -- the three transforms and an embedder -- fed progressive file
bytes against the same fed the baseline twins and PIL images."""
import io

import numpy as np
import pytest
import torch

from tests import jpeg_ref as J
from tests import jprog_ref as R
from tests.test_jpeg_cpu import load_fixture
from tests.test_jprog_cpu import load_prog_fixture, pil_file, pil_rgb, truncated_in_last_scan, truncation_files

pytestmark = pytest.mark.gpu
TV_MEAN, TV_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def px():
    return load_prog_fixture()


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def singles(L, px):
    """Every golden decoded in a call of its own, computed once: [(H, W, 3) uint8 arrays]"""
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    dec = DeviceJpegDecoder("cuda", progressive=True)
    out = []
    for f in px["files"]:
        p = dec.decode([f])
        assert p.offsets.tolist() == [0] and int(p.status[0]) == 0
        out.append(dec.unpack(p)[0].cpu().numpy())
    return out


def decode_raw(L, files, ws_fill, entry="gg_jprog_decode"):
    """One decode call on buffers of this test's own: the workspace at exactly the queried size and holding ws_fill bytes, the output holding 0xA5."""
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    plan = JpegPlan(files, progressive=entry == "gg_jprog_decode")
    plan.require_accepted()
    host = torch.empty(plan.stream_bytes, dtype=torch.uint8)
    plan.fill(host.data_ptr())
    stream_buf = host.cuda()
    ws = torch.full((plan.workspace_bytes,), ws_fill, dtype=torch.uint8, device="cuda")
    out = torch.full((plan.output_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((plan.B,), -1, dtype=torch.int32, device="cuda")
    L.check(getattr(L.lib(), entry)(plan.handle, stream_buf.data_ptr(), stream_buf.numel(), out.data_ptr(), out.numel(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                    L.stream()), entry)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    imgs = [o[i.out_offset:i.out_offset + 3 * i.height * i.width].reshape(i.height, i.width, 3) for i in plan.info]
    gaps = np.ones(len(o), bool)
    for i in plan.info:
        gaps[i.out_offset:i.out_offset + 3 * i.height * i.width] = False
    assert (o[gaps] == 0xA5).all()                                           # the alignment gaps between the images are not touched
    plan.close()
    return imgs, status.cpu().numpy()


def test_every_prog_golden_singly_and_in_one_batch_equals_pillow(L, px, singles):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    for i, (got, want) in enumerate(zip(singles, px["rgb"])):
        assert got.shape == want.shape and np.array_equal(got, want), (i, px["desc"][i], int((got != want).sum()))
    dec = DeviceJpegDecoder("cuda", progressive=True)
    files = [px["files"][0], bytearray(px["files"][1]), memoryview(px["files"][2])] + px["files"][3:]
    p = dec.decode(files)
    assert p.packed.is_cuda and p.packed.dtype == torch.uint8 and p.status.cpu().tolist() == [0] * len(files) and all(o % 256 == 0 for o in p.offsets) and p.slow is None
    for i, (got, want) in enumerate(zip(dec.unpack(p), px["rgb"])):
        assert p.sizes[i] == want.shape[:2] and np.array_equal(got.cpu().numpy(), want), (i, px["desc"][i])
    again = dec.decode(files[::-1])                                          # the decoder's staging buffer and workspace are reused
    for got, want in zip(dec.unpack(again), px["rgb"][::-1]):
        assert np.array_equal(got.cpu().numpy(), want)


def test_mixed_batch_equals_its_single_calls_whatever_the_workspace_held(L, px, fx, singles):
    base = fx["files"][:20] + [f for f, x in zip(fx["files"], fx["desc"]) if "restart" in x][:6]
    base_rgb = fx["rgb"][:20] + [r for r, x in zip(fx["rgb"], fx["desc"]) if "restart" in x][:6]
    files, want, is_base, rest = [], [], [], iter(zip(base, base_rgb))
    for n, (f, r) in enumerate(zip(px["files"], singles)):                   # two baseline files among every three progressive ones, while there are some
        files.append(f); want.append(r); is_base.append(False)
        nxt = next(rest, None) if n % 3 != 1 else None
        if nxt is not None:
            files.append(nxt[0]); want.append(nxt[1]); is_base.append(True)
    assert sum(is_base) == len(base) == 26
    plain, st = decode_raw(L, base, 0xFF, "gg_jpeg_decode")
    assert st.tolist() == [0] * len(base)
    for fill in (0xFF, 0x00):
        imgs, status = decode_raw(L, files, fill)
        assert status.tolist() == [0] * len(imgs)
        k = 0
        for i, (got, w) in enumerate(zip(imgs, want)):
            assert np.array_equal(got, w), (fill, i)
            if is_base[i]:
                assert np.array_equal(got, plain[k]), (fill, i)              # a baseline file: gg_jpeg_decode's bytes
                k += 1


def test_large_flat_file_restart_rows_and_many_unique_tables(L):
    """One 1024 x 1024 flat grey file: 16384 blocks, so Pillow codes an EOB run with 14 extra bits in its AC scans, the largest form one scan of this size reaches.
    Fresh files a few hundred pixels wide, restart rows among them.  And 400 files with tables of their own (a progressive file of Pillow's always has) in one
    batch: more unique Huffman tables than the LDS path takes, so the kernel that reads them through the cache runs."""
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder, JpegPlan
    rng = np.random.default_rng(5)
    dec = DeviceJpegDecoder("cuda", progressive=True)
    flat = pil_file(np.full((1024, 1024, 3), 97, np.uint8), "grey", 90, progressive=True)
    p = R.parse(flat)
    for s in p["scans"]:                                                     # every AC scan is one symbol: an EOB run of 16384 blocks, run length class 14
        if s["Ss"] > 0:
            b, e = s["segments"][0]
            assert e - b == 2 and J._Bits(flat[b:e]).symbol(J._code_table(*s["ac"])) == 0xE0
    assert sum(s["Ss"] > 0 for s in p["scans"]) == 4
    got = dec.unpack(dec.decode([flat]))[0].cpu().numpy()
    assert got.shape == (1024, 1024, 3) and np.array_equal(got, pil_rgb(flat))
    yy, xx = np.mgrid[0:240, 0:301]
    base = np.stack([xx * 0.8, yy, 255 - xx * 0.5 - yy * 0.3], 2)
    big = (base + rng.integers(-30, 30, base.shape)).clip(0, 255).astype(np.uint8)
    files = [pil_file(big, "4:2:0", 90, progressive=True), pil_file(big, "4:2:2", 75, progressive=True, restart_marker_rows=1), pil_file(big, "grey", 95, progressive=True),
             pil_file(np.ascontiguousarray(big.transpose(1, 0, 2)), "4:4:4", 75, progressive=True, restart_marker_blocks=7), pil_file(big, "4:2:0", 90)]
    for got, f in zip(dec.unpack(dec.decode(files)), files):
        assert np.array_equal(got.cpu().numpy(), pil_rgb(f))
    files = [pil_file(rng.integers(0, 256, (17 + t % 5, 19 + t % 7, 3)).astype(np.uint8), ("4:2:0", "4:4:4")[t % 2], 30 + t % 60, progressive=True) for t in range(400)]
    plan = JpegPlan(files, progressive=True)
    assert plan.rounds == 3 and sum(plan.scans) == 4000
    plan.close()
    assert len({f[f.index(b"\xff\xc4"):f.index(b"\xff\xda")] for f in files}) > 128          # each differs from the rest in at least one table
    for got, f in zip(dec.unpack(dec.decode(files)), files):
        assert np.array_equal(got.cpu().numpy(), pil_rgb(f))


def test_truncated_prog_files_are_zeroed_and_their_neighbours_intact(L, px, singles):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    t0, t1 = [truncated_in_last_scan(f) for f in truncation_files(px)]
    files = [px["files"][10], t0, px["files"][30], px["files"][31], t1, px["files"][50]]
    dec = DeviceJpegDecoder("cuda", progressive=True)
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
    bad = px["refuse"][px["refuse_name"].index("incomplete progression")]
    with pytest.raises(L.GgError, match="image 2 is refused: incomplete progression"):
        dec.decode([files[0], files[2], bad])


def test_with_the_switch_off_a_progressive_file_raises_as_before(L, px, fx):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder
    from geoguessr_ai_amd.training.preprocess import DeviceEvalTransform
    with pytest.raises(L.GgError, match=r"image 1 is refused: progressive \(SOF2\)"):
        DeviceJpegDecoder("cuda").decode([fx["files"][0], px["files"][0]])
    with pytest.raises(L.GgError, match=r"image 0 is refused: progressive \(SOF2\)"):
        DeviceEvalTransform(32, TV_MEAN, TV_STD, "timm", 0.95)([px["files"][5]])


@pytest.fixture(scope="module")
def triples():
    """Twelve fresh images of differing sizes as progressive files, their baseline twins (the same quantised coefficients: tests/test_jprog_cpu.py) and PIL images"""
    from PIL import Image
    rng = np.random.default_rng(77)
    prog, twin, pil = [], [], []
    for t in range(12):
        h, w = 33 + 5 * t, 70 - 3 * t
        a = (np.add.outer(np.arange(h) * 2, np.arange(w) * 3)[:, :, None] + rng.integers(0, 90, (h, w, 3))).clip(0, 255).astype(np.uint8)
        mode, q = ["4:4:4", "4:2:2", "4:2:0", "grey"][t % 4], 60 + 3 * t
        prog.append(pil_file(a, mode, q, progressive=True)); twin.append(pil_file(a, mode, q, optimize=True))
        pil.append(Image.open(io.BytesIO(prog[-1])))
    return prog, twin, pil


def test_the_three_transforms_from_progressive_bytes_baseline_twins_and_pil_images(L, triples):
    from geoguessr_ai_amd.finetune_tinyvit.augment import DeviceTrainTransform, sample_params
    from geoguessr_ai_amd.training.preprocess import DeviceEvalTransform, DevicePanoramaTransform, images_to_pixel_values
    prog, twin, pil = triples
    ev = DeviceEvalTransform(32, TV_MEAN, TV_STD, "timm", 0.95, jpeg_progressive=True)
    a, a8 = ev(prog, return_u8=True)
    b, b8 = ev(twin, return_u8=True)
    c, c8 = ev(pil, return_u8=True)
    assert torch.equal(a8, b8) and torch.equal(a8, c8) and torch.equal(a, b) and torch.equal(a, c)
    mixed = [prog[i] if i % 2 else twin[i] for i in range(12)]               # both kinds in one call
    assert torch.equal(ev(mixed), a)
    assert torch.equal(images_to_pixel_values(prog, 32, TV_MEAN, TV_STD, "cuda", crop_pct=0.95, batched=True, jpeg_progressive=True), a)
    sizes = [(im.size[1], im.size[0]) for im in pil]
    params = sample_params(sizes, 32, "rand-m9-mstd0.5-inc1", np.random.default_rng(3), TV_MEAN, "bicubic")
    tr = DeviceTrainTransform(32, seed=0, jpeg_progressive=True)
    a, a8 = tr(prog, params=params, return_u8=True)
    b, b8 = tr(twin, params=params, return_u8=True)
    c, c8 = tr(pil, params=params, return_u8=True)
    assert torch.equal(a8, b8) and torch.equal(a8, c8) and torch.equal(a, b) and torch.equal(a, c)

    def rows(items):
        return [items[0:4], [items[4], None, items[5], items[6]], items[7:11]]
    pano = DevicePanoramaTransform((24, 20), TV_MEAN, TV_STD, required_size=32, jpeg_progressive=True)
    a, b, c = pano(rows(prog)), pano(rows(twin)), pano(rows([np.asarray(im.convert("RGB")) for im in pil]))
    assert a.shape == (3, 4, 3, 24, 20) and torch.equal(a, b) and torch.equal(a, c)


def test_an_embedder_gives_identical_embeddings_from_progressive_bytes_and_from_pil_images(L, triples):
    import warnings
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    prog, twin, pil = triples
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        emb = TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", load_checkpoint=False, panorama=True, img_size=32, batch_transform=True, jpeg_progressive=True)
    a, b, c = emb(prog[:5]), emb(pil[:5]), emb(twin[:5])
    assert a.shape == (5, 320) and torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError, match="jpeg_progressive needs batch_transform=True"):
        TinyViTEmbedding(model_name="tiny_vit_5m_224", device="cuda", load_checkpoint=False, img_size=32, jpeg_progressive=True)
