"""CPU-only checks of the batched eval transform (include/gg_eval.h, geoguessr_ai_amd.training.preprocess.DeviceEvalTransform): the fixture made by Pillow
(tests/golden/eval_batch_pil.npz, tests/golden/make_golden_eval_batch.py) against the numpy restatement of oracle/preprocess_ref.py, the header as C, the struct
layouts against the ctypes binding, the exported symbols, what gg_eval_workspace_bytes answers on the host, and the per-image entry point (gg_preprocess_pil, the
B = 1 call of the same passes): its workspace bound and its host refusals.  Nothing here needs a GPU; everything here fails without the header, the symbols and the
classes."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import preprocess_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_batch_pil.npz"))
    return {k: g[k] for k in g.files}


def _cases(g):
    return [(i, g[f"src{i}"], str(g["pipeline"][i]), int(g["size"][i]), float(g["crop_pct"][i]), str(g["crop_mode"][i])) for i in range(len(g["size"]))]


def test_fixture_crops_equal_the_numpy_restatement(fixture):
    """Pillow's own Image.resize + crop (the fixture) against oracle/preprocess_ref.py on all fourteen geometries: the oracle the GPU tests lean on for arbitrary
    geometry stays pinned on these shapes, and the package's raw_image_geometry decides the same geometry as the fixture script."""
    from geoguessr_ai_amd.training.preprocess import raw_image_geometry
    g = fixture
    want_shapes = [(37, 53), (61, 29), (32, 32), (32, 48), (17, 23), (301, 97), (45, 70), (33, 64), (64, 35), (32, 32), (40, 32), (97, 301), (35, 50), (50, 35)]
    assert [g[f"src{i}"].shape[:2] for i in range(14)] == want_shapes and len(g["size"]) == 14
    passes = set()
    for i, src, pipe, size, pct, mode in _cases(g):
        u8, _ = P.raw_image_pixel_values(src, pipe, size, MEAN, STD, pct, mode)
        assert np.array_equal(u8, g[f"crop{i}"]), (i, int((u8 != g[f"crop{i}"]).sum()))
        flt, (hr, wr), (top, left) = raw_image_geometry(src.shape[0], src.shape[1], pipe, size, pct, mode)
        assert (hr, wr, top, left) == tuple(int(v) for v in g["geom"][i]) and flt == int(g["filter"][i]), i
        passes.add((wr != src.shape[1], hr != src.shape[0]))
    assert passes == {(True, True), (False, False), (True, False), (False, True)}          # both passes, neither, only the horizontal, only the vertical
    assert any((g[f"crop{i}"] == 0).any() and (g[f"crop{i}"] == 255).any() for i in range(14))      # bicubic overshoot clips at both ends


def test_eval_header_compiles_as_c_and_layouts_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_eval.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.EVAL_SYMBOLS) == {"gg_eval_workspace_bytes", "gg_eval_batch"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.EVAL_SIGNATURES[n][1]), n
    prints = [(c, ct, [f[0] for f in ct._fields_]) for c, ct in (("GgEvalGeom", L.EvalGeom), ("GgEvalArgs", L.EvalArgs))]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gg_eval.h"\nint main(void){' + "".join(
        f'printf("%zu", sizeof({c}));' + "".join(f'printf(" %zu", offsetof({c}, {f}));' for f in fields) + 'printf("\\n");' for c, _, fields in prints) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        lines = subprocess.check_output([os.path.join(d, "t")]).decode().strip().split("\n")
    for (cname, ct, fields), line in zip(prints, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields], cname
    from geoguessr_ai_amd.training.preprocess import GEOM_DTYPE
    assert GEOM_DTYPE.itemsize == C.sizeof(L.EvalGeom) == 16
    assert {n: GEOM_DTYPE.fields[n][1] for n in GEOM_DTYPE.names} == {f[0]: getattr(L.EvalGeom, f[0]).offset for f in L.EvalGeom._fields_}
    assert "gg_eval.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "eval_transform.hip" in mk.split("SRCS")[1].split("\n")[0]
    assert re.search(r"eval_transform\.hip\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", mk) and re.search(r"eval_transform\.hip\.o:[^\n]*gg_eval\.h", mk)


class _Batch:
    """Host tables of a batch of fixture images (kept alive next to the args that point into them)."""

    def __init__(self, L, g, idx, size, geom=True, **kw):
        srcs = [g[f"src{i}"] for i in idx]
        nbytes = [s.size for s in srcs]
        self.offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        self.heights, self.widths = np.array([s.shape[0] for s in srcs], np.int32), np.array([s.shape[1] for s in srcs], np.int32)
        self.geom = np.ascontiguousarray(np.stack([g["geom"][i] for i in idx]).astype(np.int32))
        a = L.EvalArgs()
        a.src_bytes = int(sum(nbytes))
        a.offsets, a.heights, a.widths = self.offsets.ctypes.data, self.heights.ctypes.data, self.widths.ctypes.data
        a.geom = self.geom.ctypes.data if geom else None
        a.B, a.Hc, a.Wc, a.filter, a.mul_rescale, a.normalize = len(idx), size, size, 3, 0, 1
        a.mean, a.std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        for k, v in kw.items():
            setattr(a, k, v)
        self.args = a


SIZE32 = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13]          # the fixture's images with a 32 x 32 crop; 5 and 11 crop to 16 x 16


def test_workspace_query_refusals_monotone_and_bound(L, fixture):
    lib, g = L.lib(), fixture
    q = lambda b: lib.gg_eval_workspace_bytes(C.byref(b.args))
    exact = q(_Batch(L, g, SIZE32, 32))
    assert exact > 0 and exact % 256 == 0
    # monotone in B
    sizes = [q(_Batch(L, g, SIZE32[:n], 32)) for n in range(1, len(SIZE32) + 1)]
    assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1] == exact
    # geom == NULL: at least the value of every fixture geometry, alone and together
    for i in range(14):
        s = int(g["size"][i])
        one, bound = q(_Batch(L, g, [i], s)), q(_Batch(L, g, [i], s, geom=False))
        assert 0 < one <= bound, (i, one, bound)
    assert exact <= q(_Batch(L, g, SIZE32, 32, geom=False))
    assert q(_Batch(L, g, [5, 11], 16)) <= q(_Batch(L, g, [5, 11], 16, geom=False))
    # every refused argument set answers -1, by name
    assert lib.gg_eval_workspace_bytes(None) == -1 and b"null args" in lib.gg_last_error()

    def geom_edit(col, val, row=1):
        b = _Batch(L, g, SIZE32[:3], 32)
        b.geom[row, col] = val
        return b
    huge = _Batch(L, g, [5], 16)
    huge.heights[0], huge.widths[0], huge.args.src_bytes = 1, 30000000, 3 * 30000000          # 30 000 000 columns -> 16: ksize beyond 2^20
    huge.geom[0] = (16, 16, 0, 0)
    for b, msg in ((_Batch(L, g, SIZE32[:3], 32, B=0), b"B=0"), (_Batch(L, g, SIZE32[:3], 32, B=4097), b"B=4097"), (_Batch(L, g, SIZE32[:3], 32, Hc=0), b"Hc=0"),
                   (_Batch(L, g, SIZE32[:3], 32, Wc=2049), b"Wc=2049"), (_Batch(L, g, SIZE32[:3], 32, filter=1), b"filter must be 2"),
                   (_Batch(L, g, SIZE32[:3], 32, filter=4), b"filter must be 2"), (_Batch(L, g, SIZE32[:3], 32, std=(C.c_float * 3)(1, 0, 1)), b"zero std"),
                   (_Batch(L, g, SIZE32[:3], 32, offsets=None), b"null offsets"), (_Batch(L, g, SIZE32[:3], 32, heights=None), b"null offsets"),
                   (_Batch(L, g, SIZE32[:3], 32, src_bytes=1000), b"image 0"), (geom_edit(2, 36), b"image 1: the crop window"), (geom_edit(3, -1), b"image 1: the crop window"),
                   (geom_edit(0, 31), b"image 1: the crop window"), (geom_edit(1, 0), b"image 1: resized size"), (huge, b"reduction factor too large")):
        assert q(b) == -1 and msg in lib.gg_last_error(), (msg, lib.gg_last_error())
    neg = _Batch(L, g, SIZE32[:3], 32)
    neg.offsets[2] = -1
    assert q(neg) == -1 and b"image 2" in lib.gg_last_error()
    # a zero std is not read without `normalize`
    assert q(_Batch(L, g, SIZE32[:3], 32, std=(C.c_float * 3)(1, 0, 1), normalize=0)) > 0


def test_bad_batches_are_refused_on_the_host_before_anything_touches_a_device(L, fixture):
    """gg_eval_batch validates against host tables: it answers (by name) on a machine without a GPU, and a buffer standing in for the device pointers is untouched."""
    lib, g = L.lib(), fixture
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    good = _Batch(L, g, SIZE32[:3], 32)
    need = lib.gg_eval_workspace_bytes(C.byref(good.args))
    assert lib.gg_eval_batch(None, None) != 0 and b"null args" in lib.gg_last_error()
    for kw, msg in ((dict(), b"null src / dst / workspace"), (dict(src=p, dst=p), b"null src / dst / workspace"), (dict(src=p, workspace=p), b"null src / dst / workspace"),
                    (dict(src=p, dst=p, workspace=p, workspace_bytes=need - 1), b"the workspace has"), (dict(src=p, dst=p, workspace=p, workspace_bytes=need, filter=5), b"filter must be 2"),
                    (dict(src=p, dst=p, workspace=p, workspace_bytes=need, geom=None), b"null geom")):
        b = _Batch(L, g, SIZE32[:3], 32, **kw)
        assert lib.gg_eval_batch(C.byref(b.args), None) < 0 and msg in lib.gg_last_error(), (msg, lib.gg_last_error())
    assert bytes(buf) == b"\0" * 64


def test_per_image_workspace_query_bounds_every_crop_window(L, fixture):
    """gg_preprocess_pil_workspace_bytes(Hs, Ws, flt, Hr, Wr, Wc) has no Hc and no top: on the 14 fixture geometries and both filters it is at least
    gg_eval_workspace_bytes of that image alone for every crop window Hc in {1, Hr // 2, Hr}, top in {0, Hr - Hc}, left = 0.  It answers -1 for what the shared plan
    refuses and goes on answering for an Hr above the crop limit of 2048."""
    lib, g = L.lib(), fixture
    checked = 0
    for i in range(14):
        Hs, Ws = g[f"src{i}"].shape[:2]
        Hr, Wr = (int(v) for v in g["geom"][i][:2])
        Wc = int(g["size"][i])
        for flt in (2, 3):
            bound = lib.gg_preprocess_pil_workspace_bytes(Hs, Ws, flt, Hr, Wr, Wc)
            assert bound > 0, (i, flt, lib.gg_last_error())
            for Hc in sorted({1, max(Hr // 2, 1), Hr}):
                for top in sorted({0, Hr - Hc}):
                    b = _Batch(L, g, [i], Wc, Hc=Hc, filter=flt)
                    b.geom[0] = (Hr, Wr, top, 0)
                    one = lib.gg_eval_workspace_bytes(C.byref(b.args))
                    assert 0 < one <= bound, (i, flt, Hc, top, one, bound, lib.gg_last_error())
                    checked += 1
    assert checked >= 14 * 2 * 4
    q = lib.gg_preprocess_pil_workspace_bytes
    assert q(50, 60, 1, 28, 34, 24) == -1 and q(50, 60, 4, 28, 34, 24) == -1
    for bad in ((0, 60, 3, 28, 34, 24), (50, -1, 3, 28, 34, 24), (50, 60, 3, 0, 34, 24), (50, 60, 3, 28, 0, 24), (50, 60, 3, 28, 34, 0)):
        assert q(*bad) == -1, bad
    assert q(1, 30000000, 3, 1, 16, 16) == -1                     # 30 000 000 columns -> 16: the shared ksize rule
    assert q(8, 8, 3, 3000, 8, 8) > 0                             # Hr above GG_EVAL_MAX_CROP: the call accepts it with Hc <= 2048, so the query answers


def test_per_image_call_refuses_on_the_host_before_anything_touches_a_device(L):
    """gg_preprocess_pil names what only it can (null pointers, mean without std) and leaves the rest to the shared plan, whose messages come back; all of it on the
    host: a buffer standing in for the device pointers is untouched."""
    lib = L.lib()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    m3 = (C.c_float * 3)(*MEAN)
    s3 = (C.c_float * 3)(*STD)

    def call(src=p, filter=3, resized=(28, 34), crop=(2, 5, 24, 24), mean=m3, std=s3, dst=p, ws=p):
        return lib.gg_preprocess_pil(src, 50, 60, filter, resized[0], resized[1], crop[0], crop[1], crop[2], crop[3], 0, mean, std, dst, None, ws, None)
    for kw, msg in ((dict(src=None), b"null src / dst / workspace"), (dict(dst=None), b"null src / dst / workspace"), (dict(ws=None), b"null src / dst / workspace"),
                    (dict(std=None), b"mean and std come together"), (dict(filter=4), b"filter must be 2"),
                    (dict(resized=(24, 30), crop=(2, 0, 24, 24)), b"must lie inside the resized image")):
        assert call(**kw) < 0 and msg in lib.gg_last_error(), (msg, lib.gg_last_error())
    assert bytes(buf) == b"\0" * 64


def test_device_eval_transform_refuses_before_the_device(L):
    """What needs no device: an unknown pipeline, and the consumers' keywords exist with their defaults off."""
    import inspect
    from geoguessr_ai_amd.training.preprocess import DeviceEvalTransform, images_to_pixel_values
    from geoguessr_ai_amd.pretrain.tinyvit_embedder import TinyViTEmbedding
    from geoguessr_ai_amd.pretrain.clip_embedder import CLIPEmbedding
    from geoguessr_ai_amd import finetune_tinyvit as FT
    with pytest.raises(ValueError, match="unknown pipeline"):
        DeviceEvalTransform(32, MEAN, STD, pipeline="pillow")
    assert inspect.signature(images_to_pixel_values).parameters["batched"].default is False
    assert inspect.signature(TinyViTEmbedding.__init__).parameters["batch_transform"].default is False
    assert inspect.signature(CLIPEmbedding.__init__).parameters["batch_transform"].default is False
    t = DeviceEvalTransform(32, MEAN, STD, "timm", 0.875, device="cpu")
    seen = list(FT.eval_transformed([], t))
    assert seen == [] and (t.size, t.pipeline, t.crop_pct, t.crop_mode) == (32, "timm", 0.875, "center")
