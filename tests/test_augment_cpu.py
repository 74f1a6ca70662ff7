"""CPU-only checks of the device-side training transform (include/gg_aug.h, geoguessr_ai_amd.finetune_tinyvit.augment): the numpy restatement against Pillow's own
outputs (tests/golden/augment_pil.npz), timm's level -> argument table, the config parser, the record sampler, and the boundary of the new entry points.  Nothing
here needs a GPU; everything here fails without the module and the header."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = (0.485, 0.456, 0.406)


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.fixture(scope="module")
def A():
    from geoguessr_ai_amd.finetune_tinyvit import augment
    return augment


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "augment_pil.npz"))
    return {k: g[k] for k in g.files}


# ------------------------------------------------------------------------------------------------- the restatement against Pillow
def test_restatement_equals_pillow_byte_for_byte(golden, A):
    g = golden
    S, srcs = int(g["S"]), [g["src0"], g["src1"], g["src2"]]
    assert [s.shape[:2] for s in srcs] == [(50, 50), (61, 83), (96, 64)] and S == 32 and len(g["case_op"]) == 102
    ops_seen, bad = set(), []
    for i in range(len(g["case_op"])):
        rec = np.zeros((), A.RECORD_DTYPE)
        rec["top"], rec["left"], rec["h"], rec["w"] = (int(v) for v in g["case_box"][i])
        rec["flip"], rec["num_layers"] = int(g["case_flip"][i]), int(g["case_layers"][i])
        for l in range(int(g["case_layers"][i])):
            o = rec["ops"][l]
            o["op"], o["applied"], o["iarg"], o["factor"] = int(g["case_op"][i]), 1, int(g["case_iarg"][i]), g["case_factor"][i]
            o["m"], o["resample"], o["fill"] = g["case_m"][i], int(g["case_resample"][i]), g["fill"]
        ops_seen.add((int(g["case_op"][i]), int(g["case_resample"][i]) if int(g["case_op"][i]) in R.AFFINE_OPS else 0))
        out = R.apply_record(srcs[int(g["case_src"][i])], rec, S, int(g["case_filter"][i]))
        d = int((out != g["out"][i]).sum())
        if d:
            bad.append((i, int(g["case_op"][i]), d))
    assert not bad, f"(case, op, differing bytes): {bad}"
    assert {o for o, _ in ops_seen} == set(range(15)) | {-1} and all((o, rs) in ops_seen for o in R.AFFINE_OPS for rs in (2, 3))
    # the cases the golden exists for: an upsampled axis, an axis equal to S, factors on both sides of 1, Posterize of 8 bits, the identity branches
    boxes = {tuple(b) for b in g["case_box"]}
    assert any(w < S for _, _, _, w in boxes) and any(h == S for _, _, h, _ in boxes)
    f = g["case_factor"][np.isin(g["case_op"], (R.COLOR, R.CONTRAST, R.BRIGHTNESS, R.SHARPNESS))]
    assert (f > 1).any() and (f < 1).any() and 8 in g["case_iarg"][g["case_op"] == R.POSTERIZE]
    flat = R.crop_resize_flip(srcs[2], 20, 16, 32, 32, S, 3, False)
    h = [np.bincount(flat[..., c].ravel(), minlength=256) for c in range(3)]
    ident = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.lut_autocontrast(h[0]), ident) and np.array_equal(R.lut_equalize(h[0]), ident)          # constant channel: hi <= lo; one occupied bin
    assert np.array_equal(R.lut_equalize(h[1]), ident) and not np.array_equal(R.lut_autocontrast(h[1]), ident)      # two levels, the rare one < 255 pixels: step == 0
    assert not np.array_equal(R.lut_equalize(h[2]), ident)


def test_op_ids_and_rotate_matrix_are_the_restatements(A):
    assert [A.OP_IDS[n] for n in A.RAND_INCREASING_OPS] == list(range(15)) == [R.AUTO_CONTRAST, R.EQUALIZE, R.INVERT, R.ROTATE, R.POSTERIZE, R.SOLARIZE, R.SOLARIZE_ADD,
                                                                                 R.COLOR, R.CONTRAST, R.BRIGHTNESS, R.SHARPNESS, R.SHEAR_X, R.SHEAR_Y, R.TRANSLATE_X,
                                                                                 R.TRANSLATE_Y]
    hdr = open(os.path.join(ROOT, "include", "gg_aug.h")).read()
    enum = dict(re.findall(r"GG_AUG_([A-Z_]+) = (\d+)", hdr))
    assert {k: int(v) for k, v in enum.items() if k != "NUM_OPS"} == {n.upper(): i for i, n in enumerate(
        ["Auto_Contrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "Solarize_Add", "Color", "Contrast", "Brightness", "Sharpness", "Shear_X", "Shear_Y",
         "Translate_X", "Translate_Y"])} and int(enum["NUM_OPS"]) == 15
    for ang in (0.0, 27.0, -13.5, 390.0):
        assert A.rotate_matrix(ang, 32, 32) == R.rotate_matrix(ang, 32, 32)
    assert A.rotate_matrix(0.0, 224, 224) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------- timm's tables
def test_level_to_argument_table_at_levels_0_9_and_10(A):
    """timm 1.0.21 LEVEL_TO_ARG for the increasing set, computed by hand from its formulas."""
    lv = A.level_to_arg
    for name in ("AutoContrast", "Equalize", "Invert"):
        assert lv(name, 9.0) == {}
    assert [lv("PosterizeIncreasing", l)["iarg"] for l in (0, 9, 10)] == [4, 1, 0]                  # 4 - int(level / 10 * 4)
    assert [lv("SolarizeIncreasing", l)["iarg"] for l in (0, 9, 10)] == [256, 26, 0]                # 256 - int(level / 10 * 256)
    assert [lv("SolarizeAdd", l)["iarg"] for l in (0, 9, 10)] == [0, 99, 110]                       # min(128, int(level / 10 * 110))
    for name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
        assert [lv(name, l, +1.0)["factor"] for l in (0, 9, 10)] == [1.0, 1.0 + 0.9 * 0.9, 1.9]
        assert [lv(name, l, -1.0)["factor"] for l in (0, 9, 10)] == [1.0, 1.0 - 0.9 * 0.9, 0.1]     # max(0.1, .): 1 - 0.9 = 0.0999.. clamps to 0.1
    for l, v in ((0, 0.0), (9, 0.9 * 0.3), (10, 0.3)):
        assert lv("ShearX", l, 1.0)["m"] == [1.0, v, 0.0, 0.0, 1.0, 0.0] and lv("ShearY", l, -1.0)["m"] == [1.0, 0.0, 0.0, -v, 1.0, 0.0]
    for l, v in ((0, 0.0), (9, 0.9 * 0.45 * 224), (10, 0.45 * 224)):
        assert lv("TranslateXRel", l, -1.0)["m"] == [1.0, 0.0, -v, 0.0, 1.0, 0.0] and lv("TranslateYRel", l, 1.0)["m"] == [1.0, 0.0, 0.0, 0.0, 1.0, v]
    for l, deg in ((0, 0.0), (9, 27.0), (10, 30.0)):
        assert lv("Rotate", l, -1.0, 224)["m"] == R.rotate_matrix(-deg, 224, 224)
    assert A.fill_colour(MEAN) == (124, 116, 104) and A.fill_colour((1.0, 0.0, 0.5)) == (255, 0, 128)


def test_config_parser(A):
    c = A.parse_config("rand-m9-mstd0.5-inc1")
    assert c == dict(magnitude=9.0, magnitude_std=0.5, magnitude_max=10.0, increasing=True, num_layers=2, prob=0.5)
    c = A.parse_config("rand-m7-mstd101-inc1-n3-p0.25-mmax8")
    assert c == dict(magnitude=7.0, magnitude_std=float("inf"), magnitude_max=8.0, increasing=True, num_layers=3, prob=0.25)
    assert A.parse_config("rand-inc1-n0")["num_layers"] == 0 and A.parse_config("rand-inc1")["magnitude"] == 10.0
    for bad in ("augmix-m3", "rand-m9", "rand-m9-inc0", "rand-m9-inc1-n5", "rand-m9-inc1-w0", "original-mstd0.5"):
        with pytest.raises(ValueError):
            A.parse_config(bad)


# ------------------------------------------------------------------------------------------------- the sampler
def test_sample_params_boxes_ops_and_frequencies(A):
    sizes = [(50, 50), (61, 83), (96, 64), (480, 640), (33, 700)] * 4000          # 20 000 records of two slots each
    rec = A.sample_params(sizes, 224, "rand-m9-mstd0.5-inc1", np.random.default_rng(123), MEAN, "random")
    assert rec.dtype == A.RECORD_DTYPE and rec.shape == (20000,)
    H, W = np.array([s[0] for s in sizes]), np.array([s[1] for s in sizes])
    assert (rec["top"] >= 0).all() and (rec["left"] >= 0).all() and (rec["h"] > 0).all() and (rec["w"] > 0).all()
    assert (rec["top"] + rec["h"] <= H).all() and (rec["left"] + rec["w"] <= W).all()
    # accepted boxes: area fraction in [0.08, 1] and aspect in [3/4, 4/3] up to the rounding of w and h to integers (half a pixel each)
    centred = (rec["top"] == (H - rec["h"]) // 2) & (rec["left"] == (W - rec["w"]) // 2)
    frac = rec["h"] * rec["w"] / (H * W)
    lo_a, hi_a = (rec["w"] - 0.5) / (rec["h"] + 0.5), (rec["w"] + 0.5) / (rec["h"] - 0.5)
    in_spec = (hi_a >= 3 / 4) & (lo_a <= 4 / 3) & ((rec["h"] + 0.5) * (rec["w"] + 0.5) >= 0.08 * H * W) & (frac <= 1.0)
    thin = (H == 33)                                                               # 33 x 700: an aspect no accepted box reaches often -> the fallback
    assert in_spec[~thin].all()
    assert (in_spec | centred)[thin].all() and (~in_spec[thin]).any()
    fb = thin & ~in_spec
    assert (rec["h"][fb] == 33).all() and (rec["w"][fb] == int(round(33 * 4 / 3))).all() and centred[fb].all()      # clamped to the ratio limit, centred
    assert (rec["num_layers"] == 2).all()
    ops = rec["ops"][:, :2]
    assert set(np.unique(ops["op"])) == set(range(15)) and (rec["ops"][:, 2:]["applied"] == 0).all()
    n = 20000
    sd = math.sqrt(n * 0.25)                                                       # binomial(20 000, 0.5)
    for slot in (0, 1):
        assert abs(int(ops["applied"][:, slot].sum()) - n / 2) <= 4 * sd, slot     # per-op probability 0.5
    assert abs(int(rec["flip"].sum()) - n / 2) <= 4 * sd                           # flip probability 0.5
    assert set(np.unique(ops["resample"])) == {2, 3} and (ops["fill"] == np.array([124, 116, 104], np.uint8)).all()
    counts = np.bincount(ops["op"][:, 0], minlength=15)
    assert (np.abs(counts - n / 15) <= 4 * math.sqrt(n * (1 / 15) * (14 / 15))).all()                               # uniform over the 15 ops
    f = ops["factor"][np.isin(ops["op"], (7, 8, 9, 10))]
    assert (f >= 0.1 - 1e-7).all() and (f <= 1.9 + 1e-6).all() and (f > 1).any() and (f < 1).any()
    # the same seed gives the same table, another seed another one; a fixed interpolation fixes the resample code
    again = A.sample_params(sizes, 224, "rand-m9-mstd0.5-inc1", np.random.default_rng(123), MEAN, "random")
    assert again.tobytes() == rec.tobytes()
    assert A.sample_params(sizes[:50], 224, generator=np.random.default_rng(124)).tobytes() != A.sample_params(sizes[:50], 224, generator=np.random.default_rng(123)).tobytes()
    assert (A.sample_params(sizes[:50], 224, generator=np.random.default_rng(1), interpolation="bicubic")["ops"]["resample"] == 3).all()
    assert (A.sample_params(sizes[:5], 224, "rand-m9-inc1-n0", np.random.default_rng(1))["num_layers"] == 0).all()


def test_fallback_box_is_centred_and_clamped(A):
    class Never:                                                                   # every attempt proposes the largest area at the widest aspect: never fits a tall image
        def uniform(self, a, b): return b
        def integers(self, a, b): return a
    assert A.crop_box(700, 33, Never()) == ((700 - 44) // 2, 0, 44, 33, False)     # in_ratio < 3/4: w = W, h = round(W / (3/4))
    assert A.crop_box(33, 700, Never())[4] is False and A.crop_box(33, 700, Never())[:4] == (0, (700 - 44) // 2, 33, 44)
    top, left, h, w, ok = A.crop_box(100, 100, np.random.default_rng(0))
    assert ok and 0 <= top <= 100 - h and 0 <= left <= 100 - w


# ------------------------------------------------------------------------------------------------- the C boundary
def test_aug_header_symbols_and_struct_layouts_match_the_binding(L, A):
    hdr = open(os.path.join(ROOT, "include", "gg_aug.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.AUG_SYMBOLS) == {"gg_aug_workspace_bytes", "gg_aug_batch"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.AUG_SIGNATURES[n][1]), n
    prints = []
    for cname, ct in (("GgAugOp", L.AugOp), ("GgAugRecord", L.AugRecord), ("GgAugArgs", L.AugArgs)):
        fields = [f[0] for f in ct._fields_]
        prints.append((cname, ct, fields))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gg_aug.h"\nint main(){' + "".join(
        f'printf("%zu", sizeof({c}));' + "".join(f'printf(" %zu", offsetof({c}, {f}));' for f in fields) + 'printf("\\n");' for c, _, fields in prints) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        lines = subprocess.check_output([os.path.join(d, "t")]).decode().strip().split("\n")
    for (cname, ct, fields), line in zip(prints, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields], cname
    # the numpy mirrors of the record: same size, same offsets
    assert A.OP_DTYPE.itemsize == C.sizeof(L.AugOp) == 72 and A.RECORD_DTYPE.itemsize == C.sizeof(L.AugRecord) == 312
    for dt, ct in ((A.OP_DTYPE, L.AugOp), (A.RECORD_DTYPE, L.AugRecord)):
        assert {n: dt.fields[n][1] for n in dt.names} == {f[0]: getattr(ct, f[0]).offset for f in ct._fields_}
    assert "gg_aug.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    assert "augment.hip" in open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()


def test_bad_batches_are_refused_on_the_host_before_anything_touches_a_device(L, A):
    """Validation runs on the host against host tables: it answers (by name) on a machine without a GPU, and the capacity function answers -1 for the same tables."""
    lib = L.lib()
    sizes = [(50, 50), (61, 83), (96, 64)]
    rec = A.sample_params(sizes, 32, "rand-m9-mstd0.5-inc1", np.random.default_rng(0), MEAN, "bicubic")
    rec[1]["ops"][0]["op"] = R.ROTATE
    offs = np.array([0, 7500, 7500 + 15189], np.int64)
    hs, ws = np.array([50, 61, 96], np.int32), np.array([50, 83, 64], np.int32)

    def args(r, **kw):
        a = L.AugArgs()
        a.src_bytes = 7500 + 15189 + 96 * 64 * 3
        a.offsets, a.heights, a.widths = offs.ctypes.data, hs.ctypes.data, ws.ctypes.data
        a.B, a.S, a.filter = 3, 32, 3
        a.mean, a.std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(0.229, 0.224, 0.225)
        a.records = r.ctypes.data if r is not None else None
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    bound, exact = lib.gg_aug_workspace_bytes(C.byref(args(None))), lib.gg_aug_workspace_bytes(C.byref(args(rec)))
    assert 0 < exact <= bound and exact % 256 == 0
    full = rec.copy()
    full["top"], full["left"], full["h"], full["w"] = 0, 0, hs, ws
    assert lib.gg_aug_workspace_bytes(C.byref(args(full))) == bound                # the bound is the whole image as the box
    assert lib.gg_aug_workspace_bytes(None) == -1 and lib.gg_aug_batch(None, None) != 0 and b"null args" in lib.gg_last_error()

    def edited(fn):
        r = rec.copy()
        fn(r)
        return r

    def box(r): r[2]["left"] = 64 - int(r[2]["w"]) + 1
    def empty(r): r[0]["h"] = 0
    def op(r): r[0]["ops"][1]["op"] = 99
    def resample(r): r[1]["ops"][0]["resample"] = 0
    def layers(r): r[1]["num_layers"] = -1
    for fn, msg in ((box, b"record 2: the box"), (empty, b"record 0: the box"), (op, b"record 0 slot 1: unknown op id 99"),
                    (resample, b"record 1 slot 0: resample must be 2 or 3, got 0"), (layers, b"record 1: num_layers=-1")):
        r = edited(fn)
        assert lib.gg_aug_workspace_bytes(C.byref(args(r))) == -1 and msg in lib.gg_last_error(), msg
        assert lib.gg_aug_batch(C.byref(args(r)), None) != 0 and msg in lib.gg_last_error(), msg
    for kw, msg in ((dict(filter=1), b"filter must be 2"), (dict(B=0), b"B=0"), (dict(S=0), b"S=0"), (dict(src_bytes=1000), b"image 0"),
                    (dict(std=(C.c_float * 3)(1, 0, 1)), b"zero std"), (dict(offsets=None), b"null offsets")):
        assert lib.gg_aug_workspace_bytes(C.byref(args(rec, **kw))) == -1 and msg in lib.gg_last_error(), msg
    # a resample code on a slot that is not affine is not read; a short workspace and NULL device pointers are refused before any launch
    r = edited(lambda r: r[0]["ops"].__setitem__("op", R.INVERT) or r[0]["ops"].__setitem__("resample", 0))
    assert lib.gg_aug_workspace_bytes(C.byref(args(r))) > 0
    assert lib.gg_aug_batch(C.byref(args(rec)), None) != 0 and b"null src / dst / workspace" in lib.gg_last_error()
    buf = (C.c_char * 64)()
    a = args(rec, src=C.addressof(buf), dst=C.addressof(buf), workspace=C.addressof(buf), workspace_bytes=exact - 1)
    assert lib.gg_aug_batch(C.byref(a), None) != 0 and b"the workspace has" in lib.gg_last_error()
    assert bytes(buf) == b"\0" * 64
