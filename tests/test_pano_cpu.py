"""CPU-only checks of the panorama fine-tune's input path (include/gg_pano.h, training/preprocess.py::DevicePanoramaTransform, training/coordinator.py): the fixture
made by Pillow and torch (tests/golden/pano_pil.npz, tests/golden/make_golden_pano.py) against the numpy restatement tests/pano_ref.py, the geometry against
raw_image_geometry and the library's own, the header as C and the struct layout against the ctypes binding, what gg_pano_workspace_bytes and gg_pano_batch refuse on the
host, the slot table built from nested lists, and the loop's defaults.  Nothing here needs a GPU; everything here fails without the header, the symbols and the
classes."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import pano_ref as R
from tests.pano_cases import MEAN, ROOT, STD, PanoTables, load_cases


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.fixture(scope="module")
def cases():
    return load_cases()


def test_fixture_holds_the_cases_and_equals_the_numpy_restatement(cases):
    """Stage 1 byte for byte, the float result within atol 1e-5 (the gate of test_preprocess_bilinear_matches_reference_golden), with and without normalisation."""
    want = [(17, 33, 8, (12, 12)), (33, 17, 8, (5, 9)), (70, 3, 3, (6, 6)), (9, 9, 12, (12, 12)), (64, 48, 16, (16, 21)), (64, 48, 16, (21, 16)), (40, 40, 40, (16, 16)),
            (1, 1, 1, (2, 3)), (61, 47, 0, (23, 29))]
    assert [(c["src"].shape[0], c["src"].shape[1], c["rs"], c["target"]) for c in cases] == want
    worst = 0.0
    for c in cases:
        u8, norm = R.view(c["src"], c["rs"], c["target"], MEAN, STD)
        _, plain = R.view(c["src"], c["rs"], c["target"])
        assert np.array_equal(u8, c["u8"]), c["i"]
        assert norm.shape == plain.shape == (3,) + c["target"] == c["norm"].shape
        worst = max(worst, float(np.abs(norm - c["norm"]).max()), float(np.abs(plain - c["plain"]).max()))
    print(f"worst |restatement - torch| {worst:.3e}")
    assert worst <= 1e-5
    # the paths the cases are there for: an image nothing resamples, the identity interpolation on a square and on a non-square image, an up-scale, no resize stage
    assert cases[2]["u8"].shape == (70, 3, 3) and np.array_equal(cases[2]["u8"], cases[2]["src"]) and np.array_equal(cases[8]["u8"], cases[8]["src"])
    assert cases[3]["u8"].shape[:2] == cases[3]["target"] and cases[5]["u8"].shape[:2] == cases[5]["target"] == (21, 16)
    for i in (3, 5):
        assert np.array_equal(cases[i]["plain"], cases[i]["u8"].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    # a missing view is the normalised zero
    _, z = R.view(None, 8, (2, 3), MEAN, STD)
    assert np.array_equal(z[:, 0, 0], (np.float32(0) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)) and R.view(None, 8, (2, 3))[1].max() == 0


def test_geometry_equals_raw_image_geometry_and_the_library(L, cases):
    from geoguessr_ai_amd.training.preprocess import DevicePanoramaTransform, raw_image_geometry
    sizes = [(c["src"].shape[0], c["src"].shape[1], c["rs"]) for c in cases] + [(640, 640, 336), (480, 640, 336), (640, 480, 336), (333, 500, 336), (500, 333, 224),
                                                                               (7, 1000, 3), (1000, 7, 5), (1, 1, 336), (2, 3, 1)]
    hr, wr = C.c_int(), C.c_int()
    for h, w, rs in sizes:
        assert L.lib().gg_pano_resized_size(h, w, rs, C.byref(hr), C.byref(wr)) == 0
        assert (hr.value, wr.value) == R.resized_size(h, w, rs) == DevicePanoramaTransform((8, 8), required_size=rs, device="cpu").resized_size(h, w), (h, w, rs)
        if rs:
            assert (hr.value, wr.value) == raw_image_geometry(h, w, "torchvision", rs)[1]
        else:
            assert (hr.value, wr.value) == (h, w)
    assert L.lib().gg_pano_resized_size(0, 3, 8, C.byref(hr), C.byref(wr)) < 0 and L.lib().gg_pano_resized_size(3, 3, -1, C.byref(hr), C.byref(wr)) < 0


def test_pano_header_compiles_as_c_and_layout_matches_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_pano.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.PANO_SYMBOLS) == {"gg_pano_resized_size", "gg_pano_workspace_bytes", "gg_pano_batch"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.PANO_SIGNATURES[n][1]), n
    fields = [f[0] for f in L.PanoArgs._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "gg_pano.h"\nint main(void){printf("%zu", sizeof(GgPanoArgs));'
           + "".join(f'printf(" %zu", offsetof(GgPanoArgs, {f}));' for f in fields)
           + 'printf("\\n%d %d %d\\n", GG_PANO_MAX_SLOTS, GG_PANO_MAX_IMAGES, GG_PANO_MAX_TARGET);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        lines = subprocess.check_output([os.path.join(d, "t")]).decode().strip().split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(L.PanoArgs)] + [getattr(L.PanoArgs, f).offset for f in fields]
    assert [int(v) for v in lines[1].split()] == [L.PANO_MAX_SLOTS, L.PANO_MAX_IMAGES, L.PANO_MAX_TARGET]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    assert set(re.findall(r"\b(gg_pano_[a-z0-9_]+)\b", nm)) == set(L.PANO_SYMBOLS)
    assert "gg_pano.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "pano_transform.hip" in mk.split("SRCS")[1].split("\n")[0]
    assert re.search(r"pano_transform\.hip\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", mk) and re.search(r"pano_transform\.hip\.o:[^\n]*gg_pano\.h[^\n]*eval_passes\.h", mk)
    assert re.search(r"eval_transform\.hip\.o:[^\n]*eval_passes\.h", mk)


def _refusals(L, cases):
    """(tables, message) for every argument set the header says is refused (device pointers play no part)."""
    srcs = [cases[0]["src"], cases[1]["src"], cases[8]["src"]]
    T = lambda slots=(0, 1, 2, -1), rs=8, target=(12, 12), **kw: PanoTables(L, srcs, slots, rs, target, **kw)
    out = [(T(num_slots=0), b"num_slots=0"), (T(num_slots=4097), b"num_slots=4097"), (T(num_images=-1), b"num_images=-1"), (T(num_images=4097), b"num_images=4097"),
           (T(num_images=0), b"slot 0 holds image 0, outside [-1, 0)"), (T(slots=(0, 3, 1, 2)), b"slot 1 holds image 3, outside [-1, 3)"),
           (T(slots=(0, 1, -2, 2)), b"slot 2 holds image -2"), (T(Ht=0), b"Ht=0"), (T(Ht=2049), b"Ht=2049"), (T(Wt=0), b"Wt=0"), (T(Wt=2049), b"Wt=2049"),
           (T(resize=-1), b"resize=-1"), (T(std=(C.c_float * 3)(1, 0, 1)), b"zero std"), (T(slot_image=None), b"null slot_image"),
           (T(offsets=None), b"null offsets"), (T(heights=None), b"null offsets"), (T(widths=None), b"null offsets"), (T(src_bytes=1000), b"image 0"),
           (T(rs=(1 << 20) + 1), b"image 0: resized size"), (T(rs=40000), b"image 0: resized size")]
    neg = T()
    neg.offsets[2] = -1
    out.append((neg, b"image 2"))
    late = T()
    late.offsets[1] += 1000000
    out.append((late, b"image 1"))
    empty = T()
    empty.heights[1] = 0
    out.append((empty, b"image 1 has size"))
    # the reduction-factor limit (ksize beyond 2^20) cannot be reached through this call: the size rule keeps the aspect ratio, so a factor above 2^19 on the short edge
    # needs an image of more than 2^38 pixels, which "image %d has size" refuses first; the check stays in the library for the day the limits move
    wide = T()
    wide.heights[0], wide.widths[0], wide.args.src_bytes = 16, 400000000, 3 * 16 * 400000000
    out.append((wide, b"image 0 has size 16 x 400000000"))
    return out


def test_workspace_query_refusals_by_name(L, cases):
    lib = L.lib()
    q = lambda t: lib.gg_pano_workspace_bytes(C.byref(t.args))
    srcs = [cases[0]["src"], cases[1]["src"], cases[8]["src"]]
    good = PanoTables(L, srcs, (0, 1, 2, -1), 8, (12, 12))
    exact = q(good)
    assert exact > 0 and exact % 256 == 0
    # monotone in the images; slots cost four bytes each; an image nothing resamples costs only its table entry
    assert q(PanoTables(L, srcs[:1], (0,), 8, (12, 12))) < q(PanoTables(L, srcs[:2], (0, 1), 8, (12, 12))) <= exact
    assert q(PanoTables(L, srcs, (0, 1, 2, -1), 0, (12, 12))) == 512 + 256 and q(PanoTables(L, srcs[:1], (0,), 0, (12, 12))) == 256 + 256          # the two tables
    assert q(PanoTables(L, srcs[2:], (0,), 8, (12, 12))) > 512
    assert lib.gg_pano_workspace_bytes(None) == -1 and b"null args" in lib.gg_last_error()
    for t, msg in _refusals(L, cases):
        assert q(t) == -1 and msg in lib.gg_last_error(), (msg, lib.gg_last_error())
    # num_images = 0 is allowed when every slot is -1, and needs no source tables; a zero std is not read without `normalize`
    assert q(PanoTables(L, [], (-1, -1), 8, (12, 12), offsets=None, heights=None, widths=None)) > 0
    assert q(PanoTables(L, srcs, (0, 1, 2, -1), 8, (12, 12), normalize=False, std=(C.c_float * 3)(1, 0, 1))) == exact


def test_bad_batches_are_refused_on_the_host_before_anything_touches_a_device(L, cases):
    """gg_pano_batch validates against host tables: it answers (by name) on a machine without a GPU, and a buffer standing in for the device pointers is untouched."""
    lib = L.lib()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    srcs = [cases[0]["src"], cases[1]["src"], cases[8]["src"]]
    need = lib.gg_pano_workspace_bytes(C.byref(PanoTables(L, srcs, (0, 1, 2, -1), 8, (12, 12)).args))
    assert lib.gg_pano_batch(None, None) != 0 and b"null args" in lib.gg_last_error()
    ok = dict(src=p, dst=p, workspace=p, workspace_bytes=need)
    for t, msg in _refusals(L, cases):
        for k, v in ok.items():
            setattr(t.args, k, v)
        assert lib.gg_pano_batch(C.byref(t.args), None) < 0 and msg in lib.gg_last_error(), (msg, lib.gg_last_error())
    u8_off = np.array([0, 1000, 2000], np.int64)
    for kw, msg in ((dict(), b"null src / dst / workspace"), (dict(src=p, dst=p), b"null src / dst / workspace"), (dict(src=p, workspace=p), b"null src / dst / workspace"),
                    (dict(dst=p, workspace=p), b"null src / dst / workspace"), (dict(ok, workspace_bytes=need - 1), b"the workspace has"),
                    (dict(ok, workspace=p + 4), b"8-byte aligned"), (dict(ok, dst_u8=p), b"dst_u8 without u8_offsets"),
                    (dict(ok, dst_u8=p, u8_offsets=u8_off.ctypes.data, dst_u8_bytes=2000 + 3 * 10 * 8 - 1), b"resized image 2 (10 x 8 at byte 2000) lies outside dst_u8")):
        t = PanoTables(L, srcs, (0, 1, 2, -1), 8, (12, 12), **kw)
        assert lib.gg_pano_batch(C.byref(t.args), None) < 0 and msg in lib.gg_last_error(), (msg, lib.gg_last_error())
    assert bytes(buf) == b"\0" * 64


def test_slot_table_from_nested_lists():
    from geoguessr_ai_amd._lib import GgError
    from geoguessr_ai_amd.training.preprocess import panorama_slot_table
    a, b, c, d, e = b"a", b"b", b"c", b"d", b"e"
    items, t = panorama_slot_table([[None, a, b, c], [None, None, None, None], [d, None, e, None]])
    assert items == [a, b, c, d, e] and t.dtype == np.int32 and t.tolist() == [[-1, 0, 1, 2], [-1, -1, -1, -1], [3, -1, 4, -1]]
    items, t = panorama_slot_table([a, None, b])
    assert items == [a, b] and t.shape == (3,) and t.tolist() == [0, -1, 1]
    items, t = panorama_slot_table([(a,), (None,)])
    assert items == [a] and t.tolist() == [[0], [-1]]
    items, t = panorama_slot_table([[None, None]])
    assert items == [] and t.tolist() == [[-1, -1]]
    arr = np.zeros((4, 5, 3), np.uint8)                       # an (H, W, 3) array is a view, not a panorama
    items, t = panorama_slot_table([arr, arr])
    assert len(items) == 2 and t.tolist() == [0, 1]
    for bad in ([], [[a, b], [c]], [[a], b], [[]], None):
        with pytest.raises(GgError):
            panorama_slot_table(bad)


def test_defaults_leave_the_old_paths_untouched():
    """train_model / evaluate_model take `transform=None` and then never look at an `images` column; the transform's own keywords and refusals that need no device."""
    import torch
    from geoguessr_ai_amd._lib import GgError
    from geoguessr_ai_amd.training import train_eval_loop as T
    from geoguessr_ai_amd.training.coordinator import panorama_batches
    from geoguessr_ai_amd.training.jpeg import PackedImages
    from geoguessr_ai_amd.training.preprocess import DevicePanoramaTransform
    assert inspect.signature(T.train_model).parameters["transform"].default is None
    assert inspect.signature(T.evaluate_model).parameters["transform"].default is None
    ds = {"pixel_values": torch.arange(24.).view(4, 6), "labels": torch.arange(8.).view(4, 2)}
    got = T._take(ds, torch.tensor([2, 0]))
    assert set(got) == {"pixel_values", "labels"} and torch.equal(got["pixel_values"], ds["pixel_values"][[2, 0]])
    assert [b["labels"].tolist() for b in T._batches(ds, 3, False, 0, 0, 1)] == [ds["labels"][:3].tolist(), ds["labels"][3:].tolist()]
    seen = []
    data = T._take({"images": [["a0", None], ["b0", "b1"], ["c0", "c1"]], "labels": torch.arange(6.).view(3, 2)}, torch.tensor([2, 0]), lambda v: seen.append(v) or "pv")
    assert seen == [[["c0", "c1"], ["a0", None]]] and data["pixel_values"] == "pv" and "images" not in data and data["labels"].tolist() == [[4, 5], [0, 1]]
    rows = [{"images": ["a0"], "labels": torch.zeros(2)}, {"images": ["b0"], "labels": torch.ones(2)}]
    data = T._take(rows, torch.tensor([1, 0]), lambda v: v)
    assert data["pixel_values"] == [["b0"], ["a0"]] and data["labels"].tolist() == [[1, 1], [0, 0]]
    p = inspect.signature(DevicePanoramaTransform.__init__).parameters
    assert (p["required_size"].default, p["device"].default, p["jpeg_split_bytes"].default) == (336, "cuda", 0)
    t = DevicePanoramaTransform((224, 224), MEAN, None, device="cpu")                  # prepare_batch's rule: normalise only when both are given
    assert t.mean is None and t.std is None and t.target == (224, 224) and t.required_size == 336
    assert DevicePanoramaTransform((5, 9), MEAN, STD, 8, device="cpu").mean == MEAN
    with pytest.raises(ValueError):
        DevicePanoramaTransform((5, 9), required_size=-1, device="cpu")
    with pytest.raises(GgError, match="either all JPEG files"):
        t._pack([[b"\xff\xd8", np.zeros((2, 2, 3), np.uint8)]])
    with pytest.raises(GgError, match="slot table"):
        t._pack(PackedImages(torch.zeros(12, dtype=torch.uint8), np.zeros(1, np.int64), [(2, 2)], torch.zeros(1, dtype=torch.int32)))
    assert PackedImages._fields[:5] == ("packed", "offsets", "sizes", "status", "slow") and PackedImages._field_defaults["slots"] is None
    b = panorama_batches([{"images": [None], "lat": 1.0, "lon": 2.0}] * 5, 2, t)
    assert len(b) == 3 and b.order(0).tolist() == [0, 1, 2, 3, 4]
    s = panorama_batches([{}] * 5, 2, t, shuffle=True, seed=3)
    assert sorted(s.order(0).tolist()) == [0, 1, 2, 3, 4] and s.order(0).tolist() != s.order(1).tolist()
