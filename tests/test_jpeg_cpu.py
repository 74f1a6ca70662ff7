"""CPU-only checks of the JPEG path (include/gg_jpeg.h, csrc/jpeg_entropy.h, geoguessr_ai_amd.training.jpeg): the numpy restatement (tests/jpeg_ref.py) against
Pillow's own results (tests/golden/jpeg_pil.npz and freshly encoded files), the host-side plan (sizes, sampling, segments, offsets, every refusal by its name), the
header as C against the ctypes binding, and the entropy decoder's very statements in a stand-alone program under AddressSanitizer and UBSan (a child process with
its own main; nothing is loaded into Python).  Nothing here needs a GPU; everything here fails without the header, the symbols and the modules."""
import ctypes as C
import io
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def load_fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    n = len(g["desc"])
    return {"files": [g[f"file_{i}"].tobytes() for i in range(n)], "rgb": [g[f"rgb_{i}"] for i in range(n)], "desc": [str(d) for d in g["desc"]],
            "refuse": [g[f"refuse_{i}"].tobytes() for i in range(len(g["refuse_name"]))], "refuse_name": [str(s) for s in g["refuse_name"]],
            "refuse_desc": [str(s) for s in g["refuse_desc"]]}


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def test_fixture_covers_what_it_should(fx):
    d = fx["desc"]
    assert len(d) >= 75 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")) < 1 << 20
    for size in ("1x1", "8x8", "16x16", "17x23", "40x48", "33x50", "3x70", "47x9", "64x48"):
        for mode in ("4:4:4", "4:2:2", "4:2:0", "grey"):
            assert any(x.startswith(f"{size} {mode} ") for x in d), (size, mode)
    for q in ("q30", "q75", "q95", "q100"):
        assert any(q in x.split() for x in d)
    for opt in ("optimize", "restart_marker_blocks", "restart_marker_rows", "comment exif", "checker"):
        assert any(opt in x for x in d), opt
    assert any(b"\xff\xfe" in f and b"\xff\xe1" in f for f in fx["files"])                  # a COM and an APP1 segment
    assert any((r == 0).any() and (r == 255).any() for r in fx["rgb"])


def test_restatement_equals_pillow_on_every_golden(fx):
    for i, (f, want) in enumerate(zip(fx["files"], fx["rgb"])):
        got = J.decode(f)
        assert got.shape == want.shape and np.array_equal(got, want), (i, fx["desc"][i], int((got != want).sum()))


def test_restatement_equals_pillow_on_200_fresh_random_images():
    from PIL import Image
    rng = np.random.default_rng(1234)
    for t in range(200):
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if t % 2:
            a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        else:
            a = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + rng.integers(0, 40, (h, w, 3))).clip(0, 255).astype(np.uint8)
        mode, q, kw = ["4:4:4", "4:2:2", "4:2:0", "grey"][t % 4], int(rng.integers(5, 101)), {}
        if t % 5 == 0:
            kw["optimize"] = True
        if t % 7 == 0:
            kw["restart_marker_blocks"] = int(rng.integers(1, 5))
        buf, im = io.BytesIO(), Image.fromarray(a)
        if mode == "grey":
            im.convert("L").save(buf, "JPEG", quality=q, **kw)
        else:
            im.save(buf, "JPEG", quality=q, subsampling=mode, **kw)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        got = J.decode(buf.getvalue())
        assert np.array_equal(got, want), (t, w, h, mode, q, kw, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------- the host-side plan
def test_plan_answers_sizes_sampling_segments_and_offsets(L, fx):
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    plan = JpegPlan(fx["files"])
    assert plan.first_refused == -1 and plan.B == len(fx["files"])
    out_at, stream_at = 0, plan.table_bytes
    assert plan.table_bytes % 256 == 0 and plan.table_bytes > 0
    for b, (f, rgb) in enumerate(zip(fx["files"], fx["rgb"])):
        i, p = plan.info[b], J.parse(f)
        assert (i.refusal, i.height, i.width, i.components, i.hs, i.vs) == (0, rgb.shape[0], rgb.shape[1], p["ncomp"], p["hs"], p["vs"]), (b, fx["desc"][b])
        assert i.segments == len(p["segments"]), (b, fx["desc"][b])
        assert i.out_offset == out_at and i.out_offset % 256 == 0                            # DeviceEvalTransform._pack's rule
        out_at += (3 * i.height * i.width + 255) // 256 * 256
        assert i.stream_offset >= stream_at and i.stream_offset % 16 == 0
        stream_at = i.stream_offset + len(f)
    assert plan.output_bytes == out_at and plan.stream_bytes >= stream_at and plan.workspace_bytes > 0
    segs = [plan.info[b].segments for b in range(plan.B)]
    assert max(segs) > 4 and min(segs) == 1                                                  # restart files and plain ones
    modes = {(plan.info[b].components, plan.info[b].hs, plan.info[b].vs) for b in range(plan.B)}
    assert modes == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    # the stream buffer: every byte is written (two fills agree), and the files lie at their offsets
    bufs = []
    for fill in (0xFF, 0x00):
        a = np.full(plan.stream_bytes, fill, np.uint8)
        plan.fill(a.ctypes.data)
        bufs.append(a)
    assert np.array_equal(bufs[0], bufs[1])
    for b, f in enumerate(fx["files"]):
        o = plan.info[b].stream_offset
        assert bufs[0][o:o + len(f)].tobytes() == f
    plan.close()
    # the same file's answers do not depend on the batch
    solo = JpegPlan([fx["files"][5]])
    assert (solo.info[0].height, solo.info[0].width, solo.info[0].segments, solo.info[0].out_offset) == (fx["rgb"][5].shape[0], fx["rgb"][5].shape[1], segs[5], 0)


def test_plan_refuses_each_case_by_its_name_and_per_image(L, fx):
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    lib = L.lib()
    names = [lib.gg_jpeg_refusal_name(c).decode() for c in range(14)]
    assert names[0] == "ok" and len(set(names)) == 14 and set(fx["refuse_name"]) == set(names[1:])      # every refusal of the header has a fixture
    good = fx["files"][4]
    files = []
    for r in fx["refuse"]:
        files += [good, r]
    plan = JpegPlan(files)
    assert plan.first_refused == 1
    for n, (want, desc) in enumerate(zip(fx["refuse_name"], fx["refuse_desc"])):
        assert plan.info[2 * n].refusal == 0, desc                                          # the neighbours are accepted
        assert plan.refusal_name(2 * n + 1) == want, (desc, plan.refusal_name(2 * n + 1), want)
    with pytest.raises(L.GgError, match="image 1 is refused: not a JPEG"):
        plan.require_accepted()
    # decode refuses such a plan before anything is launched (no device pointer is looked at: the call fails on the host)
    rc = lib.gg_jpeg_decode(plan.handle, 256, 1 << 30, 256, 1 << 30, 256, 256, 1 << 30, None)
    assert rc < 0 and b"image 1 is refused: not a JPEG" in lib.gg_last_error()
    # a file cut inside its entropy data is accepted by the plan (the decode reports it by status); cut inside its header it is refused
    b, e = J.parse(good)["segments"][0]
    cut = JpegPlan([good[:(b + e) // 2], good[:100], b"", good + b"trailing bytes"])
    assert [cut.info[b].refusal for b in range(4)] == [0, 12, 1, 0]
    assert lib.gg_jpeg_plan_create(None, None, 1, None) < 0 and b"null" in lib.gg_last_error()
    with pytest.raises(L.GgError):
        JpegPlan([])
    with pytest.raises(L.GgError):
        JpegPlan([good, "not bytes"])


def test_jpeg_header_compiles_as_c_and_layouts_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_jpeg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_jpeg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.JPEG_SYMBOLS) and len(declared) == 11
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.JPEG_SIGNATURES[n][1]), n
    fields = [f[0] for f in L.JpegInfo._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gg_jpeg.h"\nint main(void){printf("%zu", sizeof(GgJpegInfo));' + "".join(
        f'printf(" %zu", offsetof(GgJpegInfo, {f}));' for f in fields) + 'printf(" %d %d %d\\n", GG_JPEG_MAX_B, GG_JPEG_MAX_DIM, GG_JPEG_NUM_REFUSALS);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [C.sizeof(L.JpegInfo)] + [getattr(L.JpegInfo, f).offset for f in fields] + [L.JPEG_MAX_B, 16384, 14] and C.sizeof(L.JpegInfo) == 48
    # the exported gg_jpeg_ symbols of the built library are exactly the declared ones
    nm = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    assert set(re.findall(r"\b(gg_jpeg_[a-z0-9_]+)\b", nm)) == set(L.JPEG_SYMBOLS)
    assert "gg_jpeg.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "jpeg.hip" in mk.split("SRCS")[1].split("\n")[0] and "jpeg_entropy.h" in mk


# ---------------------------------------------------------------------------------------------------------------- the entropy decoder under sanitizers
def _table(t):
    counts, vals = t
    return bytes(counts) + bytes(vals) + bytes(256 - len(vals))


def _job(p, data, mcus):
    """One segment as a job of tests/jpeg_entropy_main.cpp"""
    nc = p["ncomp"]
    blocks = [p["hs"] * p["vs"], 1, 1] if nc == 3 else [1, 0, 0]
    tabs = b"".join(_table(p["dc"][min(c, nc - 1)]) + _table(p["ac"][min(c, nc - 1)]) for c in range(3))
    return struct.pack("<6i", nc, blocks[0], blocks[1], blocks[2], mcus, len(data)) + tabs + data


def _segments(f):
    """[(segment bytes, MCUs, first block)] of an intact file"""
    p = J.parse(f)
    total, ri, out = p["mcux"] * p["mcuy"], p["ri"], []
    for i, (b, e) in enumerate(p["segments"]):
        mcu0 = i * ri if ri else 0
        out.append((f[b:e], min(ri, total - mcu0) if ri else total, mcu0 * p["bpm"]))
    return p, out


@pytest.fixture(scope="module")
def entropy_exe():
    d = tempfile.mkdtemp(prefix="jpeg_entropy_")
    exe = os.path.join(d, "jpeg_entropy_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",         # the runtimes inside the program: it runs in whatever environment the suite runs in
                           os.path.join(ROOT, "tests", "jpeg_entropy_main.cpp"), "-o", exe])
    return exe


def _run(exe, jobs):
    """-> [(status, steps, int16 coefficients)]; asserts a clean exit and no sanitizer report"""
    with tempfile.TemporaryDirectory() as d:
        jp, rp = os.path.join(d, "jobs"), os.path.join(d, "results")
        with open(jp, "wb") as fh:
            fh.write(struct.pack("<i", len(jobs)) + b"".join(jobs))
        r = subprocess.run([exe, jp, rp], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
        raw, out, at = open(rp, "rb").read(), [], 0
        for _ in jobs:
            status, steps, n = struct.unpack_from("<iqi", raw, at)
            at += 16
            out.append((status, steps, np.frombuffer(raw, np.int16, n, at).reshape(-1, 64)))
            at += 2 * n
        assert at == len(raw)
        return out


def test_entropy_decoder_on_every_golden_scan_under_sanitizers(fx, entropy_exe):
    jobs, want = [], []
    for f in fx["files"]:
        p, segs = _segments(f)
        coef, status = J.coefficients(f, p)
        assert status == 0
        for data, mcus, blk0 in segs:
            jobs.append(_job(p, data, mcus))
            want.append((coef[blk0:blk0 + mcus * p["bpm"]], len(data)))
    assert len(jobs) > len(fx["files"])
    for n, ((status, steps, got), (ref, nbytes)) in enumerate(zip(_run(entropy_exe, jobs), want)):
        assert status == 0 and steps <= 8 * nbytes + 1, (n, status, steps, nbytes)
        assert np.array_equal(got, ref), (n, int((got != ref).sum()))                        # every coefficient written (the canary is gone), and the right one


def truncation_files(fx):
    """The two small restart-free files whose truncations the host program decodes here and the GPU decodes in tests/test_gpu_jpeg.py"""
    picks = [i for i, d in enumerate(fx["desc"]) if d.startswith(("16x16 4:2:0 ", "17x23 grey "))][:2]
    assert len(picks) == 2
    return [fx["files"][i] for i in picks]


def truncated(f):
    """f cut in the middle of its entropy-coded data"""
    b, e = J.parse(f)["segments"][0]
    return f[:(b + e) // 2]


def test_entropy_decoder_on_every_truncation_of_two_files_under_sanitizers(fx, entropy_exe):
    for f in truncation_files(fx):
        p, segs = _segments(f)
        assert len(segs) == 1
        data, mcus, _ = segs[0]
        full, _ = J.coefficients(f, p)
        res = _run(entropy_exe, [_job(p, data[:cut], mcus) for cut in range(len(data))])
        for cut, (status, steps, got) in enumerate(res):
            assert steps <= 8 * cut + 1, (cut, steps)
            assert status in (1, 2, 3) or np.array_equal(got, full), cut                     # a cut that only loses padding bits may still decode, and then correctly
        half = len(data) // 2
        assert truncated(f).endswith(data[:half]) and not truncated(f).endswith(data[:half + 1])          # the cut that tests/test_gpu_jpeg.py decodes ...
        assert res[half][0] != 0                                                             # ... has a non-zero status here
        assert res[0][0] == 1 and sum(r[0] != 0 for r in res) >= len(data) - 2


def with_fill_bytes(f, run=1):
    """f with `run` extra FF bytes in front of every FF of its entropy-coded data and of the EOI behind it: FF .. FF 00 stays the data byte FF, FF .. FF Dn stays
    the marker (fill bytes may precede a marker); libjpeg's reader, and so Pillow, decodes the same picture."""
    b = J.parse(f)["segments"][0][0]
    return f[:b] + f[b:].replace(b"\xff", b"\xff" * (run + 1))


def fill_byte_files(fx):
    """Hand-made from goldens that have stuffed FF bytes and restart markers: one extra FF each, and runs of 9 (longer than the reader's eight-byte window)"""
    picks = [f for f, d in zip(fx["files"], fx["desc"]) if "restart" in d and "noise" in d][:2] + [f for f, d in zip(fx["files"], fx["desc"]) if d.startswith("40x48 4:2:0 noise")][:1]
    assert len(picks) == 3 and all(f[J.parse(f)["segments"][0][0]:].count(b"\xff\x00") > 0 for f in picks)
    return [with_fill_bytes(f, run) for f in picks for run in (1, 9)], [f for f in picks for _ in (1, 9)]


def test_fill_bytes_decode_as_pillow_decodes_them(L, fx, entropy_exe):
    from PIL import Image
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    filled, plain = fill_byte_files(fx)
    plan = JpegPlan(filled)
    jobs, want = [], []
    for b, (f, g) in enumerate(zip(filled, plain)):
        pil = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        assert np.array_equal(pil, np.asarray(Image.open(io.BytesIO(g)).convert("RGB"))) and np.array_equal(J.decode(f), pil)      # Pillow's own answer
        p, segs = _segments(f)
        assert plan.info[b].refusal == 0 and plan.info[b].segments == len(segs) == len(_segments(g)[1])
        coef, status = J.coefficients(g)
        assert status == 0
        for data, mcus, blk0 in segs:
            jobs.append(_job(p, data, mcus)); want.append(coef[blk0:blk0 + mcus * p["bpm"]])
    for (status, steps, got), ref in zip(_run(entropy_exe, jobs), want):
        assert status == 0 and np.array_equal(got, ref)


def test_entropy_decoder_on_2000_corruptions_under_sanitizers(fx, entropy_exe):
    rng = np.random.default_rng(2026)
    pool = [(p, data, mcus) for f in fx["files"] for p, segs in [_segments(f)] for data, mcus, _ in segs if len(data) > 0]
    jobs, lens = [], []
    for _ in range(2000):
        p, data, mcus = pool[int(rng.integers(len(pool)))]
        a = bytearray(data)
        a[int(rng.integers(len(a)))] = int(rng.integers(256))
        jobs.append(_job(p, bytes(a), mcus)); lens.append(len(a))
    res = _run(entropy_exe, jobs)                                                            # a clean exit: no report, and the program's own step bound held
    assert all(steps <= 8 * n + 1 for (_, steps, _), n in zip(res, lens))
    assert {r[0] for r in res} >= {0, 1} and all(r[0] in (0, 1, 2, 3) for r in res)
