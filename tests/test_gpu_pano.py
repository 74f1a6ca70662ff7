"""The panorama fine-tune's input path (include/gg_pano.h, csrc/pano_transform.hip, training/preprocess.py::DevicePanoramaTransform, training/coordinator.py) on the GPU:
the resized uint8 images BYTE-IDENTICAL to Pillow's and pixel_values within atol 1e-5 of torch's F.interpolate + normalise (tests/golden/pano_pil.npz; the gate of
test_preprocess_bilinear_matches_reference_golden), slot handling and independence of the batch, the offsets and the workspace's earlier contents bit for bit, file
bytes through the transform's own decoder, every refusal, and train_model / evaluate_model fed rows of file bytes.  Every image is at most 70 pixels a side."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import pano_ref as R
from tests.pano_cases import MEAN, ROOT, STD, PanoTables, load_cases, pano_batch

pytestmark = pytest.mark.gpu
CASES = load_cases()


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def jpeg():
    """The decoder's fixture: (files as bytes, Pillow's pixels of each)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    n = sum(1 for k in g.files if k.startswith("file_"))
    return [g[f"file_{i}"].tobytes() for i in range(n)], [g[f"rgb_{i}"] for i in range(n)]


# ------------------------------------------------------------------------------------------------- 1, 2. the fixture
@pytest.mark.parametrize("i", range(len(CASES)))
def test_golden_case_u8_identical_and_pixel_values_within_1e5(L, i):
    """One call per case and normalisation setting: the resized uint8 image is Pillow's byte for byte, dst within atol 1e-5 of torch's."""
    c = CASES[i]
    for normalize, want in ((True, c["norm"]), (False, c["plain"])):
        dst, u8 = pano_batch(L, [c["src"]], [0], c["rs"], c["target"], normalize)
        assert u8[0].shape == c["u8"].shape and np.array_equal(u8[0], c["u8"]), (i, int((u8[0] != c["u8"]).sum()))
        worst = float(np.abs(dst[0] - want).max())
        print(f"case {i} normalize={normalize}: worst |dst - torch| {worst:.3e}")
        assert worst <= 1e-5
        assert np.array_equal(pano_batch(L, [c["src"]], [0], c["rs"], c["target"], normalize, want_u8=False)[0], dst)          # dst does not depend on the uint8 hook


# ------------------------------------------------------------------------------------------------- 3. slots
def _singles(L, srcs, rs, target, normalize=True):
    return [pano_batch(L, [s], [0], rs, target, normalize)[0][0] for s in srcs]


def test_slots_equal_their_single_image_calls_bit_for_bit(L):
    srcs = [CASES[i]["src"] for i in (0, 1, 2, 4, 6, 7, 8)]
    rs, target = 8, (12, 20)
    one = _singles(L, srcs, rs, target)
    missing = pano_batch(L, [srcs[0]], [-1], rs, target)[0][0]
    assert np.array_equal(missing, R.view(None, rs, target, MEAN, STD)[1])
    assert np.array_equal(pano_batch(L, [], [-1, -1], rs, target, want_u8=False)[0], np.stack([missing, missing]))          # num_images = 0
    assert (pano_batch(L, [srcs[0]], [-1], rs, target, normalize=False)[0] == 0).all()

    def check(slots):
        dst, _ = pano_batch(L, srcs, slots, rs, target)
        for s, img in enumerate(np.asarray(slots).reshape(-1)):
            assert np.array_equal(dst[s], missing if img < 0 else one[img]), (slots, s)
    check([[-1, 0, 1, 2], [-1, -1, -1, -1], [3, 4, 5, -1]])          # N = 3, V = 4: the first slot, a whole panorama and the last slot missing
    check([6, 5, 4, 3, 2, 1, 0])                                     # V = 1, in another order
    check([[2, 2], [0, 2]])                                          # one image in two slots (and images no slot uses)
    # sizes that take the ragged store (Wt % 4 != 0) and the vector store
    for target in ((5, 9), (7, 8), (3, 1)):
        one_t = _singles(L, srcs[:3], rs, target)
        dst, _ = pano_batch(L, srcs[:3], [2, -1, 0, 1], rs, target)
        assert np.array_equal(dst[0], one_t[2]) and np.array_equal(dst[2], one_t[0]) and np.array_equal(dst[3], one_t[1])
        for s in range(3):
            assert np.abs(one_t[s] - R.view(srcs[s], rs, target, MEAN, STD)[1]).max() <= 1e-5


# ------------------------------------------------------------------------------------------------- 4. one batch, unaligned offsets, dirty workspace
@pytest.mark.parametrize("rs,target", [(8, (5, 9)), (0, (12, 12)), (12, (16, 16))])
def test_all_sources_in_one_batch_at_unaligned_offsets(L, rs, target):
    srcs = [c["src"] for c in CASES]
    one = [pano_batch(L, [s], [0], rs, target) for s in srcs]
    slots = list(range(len(srcs)))
    for fill in (0xFF, 0x00):
        dst, u8 = pano_batch(L, srcs, slots, rs, target, gap=1, lead=3, ws_fill=fill, u8_gap=5)
        for s in slots:
            assert np.array_equal(dst[s], one[s][0][0]) and np.array_equal(u8[s], one[s][1][0]), (rs, target, fill, s)
    for s, src in enumerate(srcs):                                    # and they are the restatement's: Pillow's bytes for every source at this size
        want_u8, want = R.view(src, rs, target, MEAN, STD)
        assert np.array_equal(one[s][1][0], want_u8) and np.abs(one[s][0][0] - want).max() <= 1e-5, s


# ------------------------------------------------------------------------------------------------- 5. file bytes
def test_file_bytes_through_the_transform(L, jpeg):
    from geoguessr_ai_amd.training.preprocess import DevicePanoramaTransform
    files, rgb = jpeg
    items = files[:1] + [None] + files[1:] + [None, None]
    assert len(items) % 4 == 0 and len(files) == 77
    panoramas = [items[i:i + 4] for i in range(0, len(items), 4)]
    rs, target = 16, (12, 10)
    got = {}
    for split in (0, 64):
        tfm = DevicePanoramaTransform(target, MEAN, STD, required_size=rs, jpeg_split_bytes=split)
        pv, u8 = tfm(panoramas, return_u8=True)
        assert pv.shape == (len(panoramas), 4, 3) + target and pv.dtype == torch.float32 and len(u8) == len(files)
        got[split] = (pv.cpu().numpy(), [u.cpu().numpy() for u in u8])
        assert torch.equal(tfm(panoramas), pv)                        # the workspace is reused; the result is the same
    assert np.array_equal(got[0][0], got[64][0]) and all(np.array_equal(a, b) for a, b in zip(got[0][1], got[64][1]))
    pv, u8 = got[0][0].reshape(-1, 3, *target), got[0][1]
    worst, k = 0.0, 0
    for s, item in enumerate(items):
        want_u8, want = R.view(None if item is None else rgb[k], rs, target, MEAN, STD)
        if item is not None:
            assert np.array_equal(u8[k], want_u8), k
            k += 1
        worst = max(worst, float(np.abs(pv[s] - want).max()))
    print(f"worst |pixel_values - restatement| over {len(items)} slots {worst:.3e}")
    assert worst <= 1e-5
    # a flat list of views gives (N, 3, Ht, Wt); raw images take the same path as their files' pixels
    flat = DevicePanoramaTransform(target, MEAN, STD, required_size=rs)([rgb[40], None, rgb[12]])
    assert flat.shape == (3, 3) + target
    assert np.array_equal(flat.cpu().numpy(), np.stack([pv[items.index(files[40])], pv[1], pv[items.index(files[12])]]))


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_every_refusal_by_name_leaves_dst_untouched(L):
    from tests.test_pano_cpu import _refusals
    lib = L.lib()
    dst = torch.full((4, 3, 12, 12), float("nan"), device="cuda")
    u8 = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    src = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    u8_off = np.array([0, 1000, 2000], np.int64)
    tables = _refusals(L, CASES)
    good = PanoTables(L, [CASES[0]["src"], CASES[1]["src"], CASES[8]["src"]], (0, 1, 2, -1), 8, (12, 12))
    need = lib.gg_pano_workspace_bytes(C.byref(good.args))
    assert 0 < need <= ws.numel() and good.host.size <= src.numel()
    T = lambda **kw: PanoTables(L, good.srcs, (0, 1, 2, -1), 8, (12, 12), **kw)
    ok = dict(src=src.data_ptr(), dst=dst.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    tables += [(T(**dict(ok, src=None)), b"null src / dst / workspace"), (T(**dict(ok, dst=None)), b"null src / dst / workspace"),
               (T(**dict(ok, workspace=None)), b"null src / dst / workspace"), (T(**dict(ok, workspace_bytes=need - 1)), b"the workspace has"),
               (T(**dict(ok, workspace=ws.data_ptr() + 4)), b"8-byte aligned"), (T(**dict(ok, dst_u8=u8.data_ptr())), b"dst_u8 without u8_offsets"),
               (T(**dict(ok, dst_u8=u8.data_ptr(), u8_offsets=u8_off.ctypes.data, dst_u8_bytes=2000 + 3 * 10 * 8 - 1)), b"resized image 2 (10 x 8 at byte 2000)")]
    for t, msg in tables:
        for k, v in ok.items():
            if getattr(t.args, k) in (None, 0) and msg != b"null src / dst / workspace":
                setattr(t.args, k, v)
        assert lib.gg_pano_batch(C.byref(t.args), L.stream()) < 0 and msg in lib.gg_last_error(), (msg, lib.gg_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()) and bool((u8 == 0x5A).all()) and not bool(ws.any())
    with pytest.raises(L.GgError, match="is refused: progressive"):
        from geoguessr_ai_amd.training.preprocess import DevicePanoramaTransform
        g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
        DevicePanoramaTransform((12, 12))([[g["file_4"].tobytes(), g["refuse_1"].tobytes()]])          # the decoder's refusals pass through by name


# ------------------------------------------------------------------------------------------------- 7. the loop
def test_train_and_evaluate_on_rows_of_file_bytes(L, jpeg):
    """train_model(transform=...) over rows whose `images` are file bytes equals, bit for bit, the same loop fed the pixel_values the transform produced by hand.
    The attention biases are frozen in both runs: their gradients are summed with float atomics (csrc/attention.hip), so with them trainable two runs of the SAME
    loop on the SAME pixel_values already differ in the last bit (9.462424278 against 9.462423325 for the second batch's loss), which is not what this test is about."""
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.training.coordinator import panorama_batches
    from geoguessr_ai_amd.training.preprocess import DevicePanoramaTransform
    from geoguessr_ai_amd.training.train_eval_loop import evaluate_model, train_model
    files, _ = jpeg
    views = [[files[16 + 4 * n + v] for v in range(4)] for n in range(4)]          # 48 x 40, 50 x 33 and 70 x 3 files, four chroma layouts
    views[1][2] = None
    labels = torch.tensor([[10.75, 59.91], [-73.98, 40.75], [2.35, 48.86], [139.69, 35.68]], device="cuda")
    tfm = DevicePanoramaTransform((224, 224), MEAN, STD, required_size=32)
    by_hand = tfm(views)
    assert by_hand.shape == (4, 4, 3, 224, 224)
    args = types.SimpleNamespace(learning_rate=1e-4, per_device_train_batch_size=2, per_device_eval_batch_size=2, num_train_epochs=1, logging_steps=1, seed=0)

    def run(train, val, transform):
        torch.manual_seed(0)
        base = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, drop_path_rate=0.0)
        model = SuperGuessr(base, panorama=True, should_smooth_labels=True).cuda()
        for name, p in model.named_parameters():
            p.requires_grad_(p.requires_grad and not name.endswith("attention_biases"))
        assert sum(p.requires_grad for p in model.parameters()) > 40
        logs, seen = [], []

        def metrics(res):
            seen.append([np.array(r) for r in res])
            return {"Geocell_accuracy": float((res[1] == res[4]).mean())}
        train_model(model, {"train": train, "val": val}, False, args, metrics, should_profile=False, log_fn=lambda tag, v, step: logs.append((tag, float(v), step)),
                    save_path="", transform=transform)
        metric = evaluate_model(model, val, metrics, args, transform=transform)
        return logs, seen, metric, [p.detach().clone() for p in model.parameters()]
    raw = {"images": views, "labels": labels}
    pre = {"pixel_values": by_hand, "labels": labels}
    a, b = run(raw, raw, tfm), run(pre, pre, None)
    assert a[0] == b[0] and any(t == "Loss/train" for t, _, _ in a[0]) and any(t == "Loss/val" for t, _, _ in a[0]) and all(np.isfinite(v) for _, v, _ in a[0])
    assert a[2] == b[2] and len(a[1]) == len(b[1]) == 2
    for x, y in zip(a[1], b[1]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert len(a[3]) == len(b[3]) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
    # the rows of the coordinator loop: the same pixel_values per batch, (lon, lat) labels, the nearest centroid as the class
    rows = [{"images": views[n], "lat": float(labels[n, 1]), "lon": float(labels[n, 0])} for n in range(4)]
    cent = torch.tensor([[0.0, 50.0], [-75.0, 40.0], [140.0, 35.0]])
    batches = list(panorama_batches(rows, 3, tfm, centroids=cent))
    assert [tuple(x["pixel_values"].shape) for x in batches] == [(3, 4, 3, 224, 224), (1, 4, 3, 224, 224)]
    assert torch.equal(torch.cat([x["pixel_values"] for x in batches]), by_hand) and torch.equal(torch.cat([x["labels"] for x in batches]), labels)
    assert torch.cat([x["labels_clf"] for x in batches]).tolist() == [0, 1, 0, 2]
    assert "labels_clf" not in next(iter(panorama_batches(rows, 4, tfm)))
