"""CPU-only checks of the progressive JPEG decode (include/gg_jprog.h, csrc/jpeg_progressive.h): the fixture and the numpy restatement (tests/jprog_ref.py) against
Pillow and against the baseline twins' coefficients; the host-side plan (sizes, scans, rounds, segments, the scan table, every refusal by name and per image, mixed
batches, what the older entry points say to such plans); the header as C against the binding; the lane functions, scan by scan with the kernel's very statements, in
a stand-alone program under AddressSanitizer and UBSan (tests/jprog_entropy_main.cpp: a child process with its own main, nothing is loaded into Python).  Nothing
here needs a GPU; everything here fails without the header, the symbols and the functions."""
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
from tests import jprog_ref as R
from tests.test_jpeg_cpu import _table, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG_FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_prog_pil.npz")
SCAN_DTYPE = np.dtype([(n, "<i4") for n in ("img", "base", "cmask", "Ss", "Se", "Ah", "Al", "dc0", "dc1", "dc2", "ac", "bw", "bh", "round", "seg0", "nseg")])
NEW_NAMES = {32: "bad progressive scan script", 33: "incomplete progression", 34: "more than 64 scans", 35: "DNL marker or a frame height of 0"}


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def load_prog_fixture():
    g = np.load(PROG_FIXTURE)
    n, r = len(g["desc"]), len(g["refuse_name"])
    return {"files": [g[f"file_{i}"].tobytes() for i in range(n)], "rgb": [g[f"rgb_{i}"] for i in range(n)], "desc": [str(d) for d in g["desc"]],
            "refuse": [g[f"refuse_{i}"].tobytes() for i in range(r)], "refuse_name": [str(x) for x in g["refuse_name"]], "refuse_desc": [str(x) for x in g["refuse_desc"]]}


@pytest.fixture(scope="module")
def px():
    return load_prog_fixture()


@pytest.fixture(scope="module")
def parsed(px):
    return [R.parse(f) for f in px["files"]]


@pytest.fixture(scope="module")
def coefs(px, parsed):
    """Every golden's coefficients by the restatement, decoded once"""
    out = []
    for f, p in zip(px["files"], parsed):
        coef, status = R.coefficients(f, p)
        assert status == 0
        out.append(coef)
    return out


def pil_file(a, mode, q, **kw):
    from PIL import Image
    buf, im = io.BytesIO(), Image.fromarray(a)
    if mode == "grey":
        im.convert("L").save(buf, "JPEG", quality=q, **kw)
    else:
        im.save(buf, "JPEG", quality=q, subsampling=mode, **kw)
    return buf.getvalue()


def pil_rgb(f):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def truncated_in_last_scan(f):
    """f cut in the middle of its last scan's entropy-coded data (a file without restart markers)"""
    b, e = R.parse(f)["scans"][-1]["segments"][-1]
    return f[:(b + e) // 2]


# ---------------------------------------------------------------------------------------------------------------- the fixture and the restatement
def test_prog_fixture_covers_what_it_should(px, parsed):
    d = px["desc"]
    assert os.path.getsize(PROG_FIXTURE) < 1 << 20
    pil = [x for x in d if "pillow" in x]
    assert {x.split()[0] for x in pil} >= {"1x1", "7x9", "16x16", "17x33", "3x70", "33x50", "64x48"}
    assert {x.split()[1] for x in pil} == {"4:2:0", "4:2:2", "4:4:4", "grey"}
    assert {"q30", "q75", "q95", "q100"} <= {x.split()[3] for x in pil}
    for word in ("restart_marker_blocks", "restart_marker_rows", "gradient", "checker", "comment exif"):
        assert any(word in x for x in pil), word
    for x, p in zip(d, parsed):                                                              # a grey progressive file of Pillow's has 6 scans, a colour one 10
        if "pillow" in x:
            assert len(p["scans"]) == (6 if "grey" in x else 10) and max(s["round"] for s in p["scans"]) == 3, x
        if "restart" in x:
            assert all(s["ri"] > 0 and len(s["segments"]) > 1 for s in p["scans"]), x       # DRI is in force in every scan
    for word in ("spectral selection only", "non-interleaved DC scans", "DC with three refinements", "bands of width 1", "AC band first coded at Al 3 and refined three times",
                 "25 scans out of round order", "DHT and DRI changed between scans"):
        assert any("script: " + word in x for x in d), word
    p = parsed[next(i for i, x in enumerate(d) if "25 scans" in x)]
    rounds = [s["round"] for s in p["scans"]]
    assert len(rounds) >= 20 and rounds != sorted(rounds)                                     # rounds that differ from the file order
    p = parsed[next(i for i, x in enumerate(d) if "bands of width 1" in x)]
    assert len(p["scans"]) == 64                                                              # GG_JPROG_MAX_SCANS: Pillow opened it (its pixels are in the fixture)
    p = parsed[next(i for i, x in enumerate(d) if "DHT and DRI changed" in x and "grey" not in x)]
    assert len({s["ri"] for s in p["scans"]}) >= 4 and 0 in {s["ri"] for s in p["scans"][1:]} and len({str(s["ac"]) for s in p["scans"] if s["ac"]}) >= 3
    assert any(len(s["comps"]) == 2 for q in parsed for s in q["scans"])                      # an interleaved scan of two of three components
    assert set(px["refuse_name"]) == set(NEW_NAMES.values())                                  # every new refusal has a fixture
    assert any("last scan removed, EOI kept" in x for x in px["refuse_desc"]) and any("cut off between scans" in x for x in px["refuse_desc"])
    gradient = [p for x, p in zip(d, parsed) if "gradient" in x and "restart" in x]
    assert gradient and all(len(s["segments"]) >= 3 for p in gradient for s in p["scans"])


def test_restatement_equals_pillow_on_every_prog_golden(px, parsed, coefs):
    for i, (p, coef, want) in enumerate(zip(parsed, coefs, px["rgb"])):
        got = R.pixels(p, coef)
        assert got.shape == want.shape and np.array_equal(got, want), (i, px["desc"][i], int((got != want).sum()))
        assert np.array_equal(pil_rgb(px["files"][i]), want), i                               # and the fixture is this Pillow's decode of the very file


def test_restatement_equals_pillow_and_the_baseline_twin_on_200_fresh_files():
    """Pillow codes an image with progressive=True and with optimize=True, at the same quality and sampling, to the same quantised coefficients: the restatement's
    coefficients are held to tests/jpeg_ref.py's of the baseline twin, its pixels to Pillow's decode of the progressive file."""
    rng = np.random.default_rng(4321)
    for t in range(200):
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if t % 2:
            a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        else:
            a = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + rng.integers(0, 40, (h, w, 3))).clip(0, 255).astype(np.uint8)
        mode, q, kw = ["4:4:4", "4:2:2", "4:2:0", "grey"][t % 4], int(rng.integers(5, 101)), {}
        if t % 7 == 0:
            kw["restart_marker_blocks"] = int(rng.integers(1, 5))
        f, twin = pil_file(a, mode, q, progressive=True, **kw), pil_file(a, mode, q, optimize=True)
        p = R.parse(f)
        coef, status = R.coefficients(f, p)
        ref, ref_status = J.coefficients(twin)
        assert status == 0 and ref_status == 0 and np.array_equal(coef, ref), (t, w, h, mode, q, kw)
        want = pil_rgb(f)
        got = R.pixels(p, coef)
        assert np.array_equal(got, want), (t, w, h, mode, q, kw, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------- the host-side plan
def _scan_table(plan):
    """The scan table of a plan's table block (csrc/jpeg.hip lays the block out as images | segments | quantisers | Huffman tables | scans | segments in round
    order, each region rounded up to 256 bytes)"""
    buf = np.zeros(plan.stream_bytes, np.uint8)
    plan.fill(buf.ctypes.data)
    nscan, nseg = sum(plan.scans), sum(i.segments for i in plan.info)
    order_size = (max(nseg, 1) * 4 + 255) // 256 * 256
    scan_size = (max(nscan, 1) * SCAN_DTYPE.itemsize + 255) // 256 * 256
    end = plan.table_bytes - order_size
    scans = np.frombuffer(buf[end - scan_size:end].tobytes(), SCAN_DTYPE, nscan)
    order = np.frombuffer(buf[end:end + 4 * nseg].tobytes(), np.int32)
    return scans, order


def test_prog_plan_answers_sizes_scans_rounds_and_segments(L, px, parsed):
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    plan = JpegPlan(px["files"], progressive=True)
    assert plan.first_refused == -1 and plan.B == len(px["files"]) and plan.table_bytes % 256 == 0
    out_at = 0
    for b, (p, rgb) in enumerate(zip(parsed, px["rgb"])):
        i = plan.info[b]
        assert (i.refusal, i.height, i.width, i.components, i.hs, i.vs) == (0, rgb.shape[0], rgb.shape[1], p["ncomp"], p["hs"], p["vs"]), (b, px["desc"][b])
        assert i.segments == sum(len(s["segments"]) for s in p["scans"]) and plan.scans[b] == len(p["scans"]), (b, px["desc"][b])
        assert i.out_offset == out_at
        out_at += (3 * i.height * i.width + 255) // 256 * 256
    assert plan.output_bytes == out_at and plan.workspace_bytes == L.lib().gg_jprog_workspace_bytes(plan.handle) > 0
    assert plan.rounds == max(s["round"] for p in parsed for s in p["scans"]) >= 4
    scans, order = _scan_table(plan)
    at, seg = 0, 0
    for b, p in enumerate(parsed):
        for s in p["scans"]:
            m = scans[at]
            assert (m["img"], m["base"], m["cmask"]) == (b, 0, sum(1 << c for c in s["comps"])), (b, at)
            assert (m["Ss"], m["Se"], m["Ah"], m["Al"], m["round"]) == (s["Ss"], s["Se"], s["Ah"], s["Al"], s["round"]), (b, at, px["desc"][b])
            assert (m["bw"], m["bh"], m["seg0"], m["nseg"]) == (s["bw"], s["bh"], seg, len(s["segments"])), (b, at, px["desc"][b])
            at += 1; seg += len(s["segments"])
    assert at == len(scans) and sorted(order.tolist()) == list(range(seg))                   # every segment has its lane in exactly one round
    seg_round = np.concatenate([np.full(m["nseg"], m["round"]) for m in scans])
    assert (np.diff(seg_round[order]) >= 0).all()                                             # and the rounds follow one another
    # every byte of the stream buffer is written, and a file's answers do not depend on the batch
    bufs = []
    for fill in (0xFF, 0x00):
        a = np.full(plan.stream_bytes, fill, np.uint8)
        plan.fill(a.ctypes.data)
        bufs.append(a)
    assert np.array_equal(bufs[0], bufs[1])
    plan.close()
    n = next(i for i, x in enumerate(px["desc"]) if "25 scans" in x)
    solo = JpegPlan([px["files"][n]], progressive=True)
    assert (solo.scans, solo.rounds, solo.info[0].out_offset) == ([25], max(s["round"] for s in parsed[n]["scans"]), 0)
    pil = JpegPlan([px["files"][0], px["files"][3]], progressive=True)                        # libjpeg's standard scripts: 3 rounds
    assert pil.scans == [10, 6] and pil.rounds == 3


def test_prog_plan_refuses_each_case_by_its_name_and_per_image(L, px):
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    lib = L.lib()
    assert {c: lib.gg_jprog_refusal_name(c).decode() for c in NEW_NAMES} == NEW_NAMES
    for c in range(14):                                                                      # codes 0 .. 13 keep their names, but for 9
        if c != 9:
            assert lib.gg_jprog_refusal_name(c) == lib.gg_jpeg_refusal_name(c)
    assert lib.gg_jprog_refusal_name(9) == b"a baseline file with more than one scan or a non-interleaved scan"
    assert lib.gg_jprog_refusal_name(36) == b"unknown" and lib.gg_jprog_refusal_name(20) == b"unknown" and lib.gg_jpeg_refusal_name(32) == b"unknown"
    good = px["files"][5]
    files = []
    for r in px["refuse"]:
        files += [good, r]
    plan = JpegPlan(files, progressive=True)
    assert plan.first_refused == 1
    codes = {v: k for k, v in NEW_NAMES.items()}
    for n, (want, desc) in enumerate(zip(px["refuse_name"], px["refuse_desc"])):
        assert plan.info[2 * n].refusal == 0 and plan.scans[2 * n] == 10, desc               # the neighbours are accepted
        assert plan.info[2 * n + 1].refusal == codes[want] and plan.refusal_name(2 * n + 1) == want and plan.scans[2 * n + 1] == 0, (desc, plan.refusal_name(2 * n + 1))
    with pytest.raises(L.GgError, match="image 1 is refused: bad progressive scan script"):
        plan.require_accepted()
    rc = lib.gg_jprog_decode(plan.handle, 256, 1 << 30, 256, 1 << 30, 256, 256, 1 << 30, None)
    assert rc < 0 and b"gg_jprog_decode: image 1 is refused: bad progressive scan script" in lib.gg_last_error()
    assert lib.gg_jprog_plan_scans(plan.handle, -1) == -1 and lib.gg_jprog_plan_scans(plan.handle, len(files)) == -1
    # the refusals of include/gg_jpeg.h keep their codes in such a plan; a baseline file with two scans is code 9
    fx = load_fixture()
    old = JpegPlan(fx["refuse"], progressive=True)
    for b, want in enumerate(fx["refuse_name"]):
        if want == "progressive (SOF2)":
            assert old.info[b].refusal == 12, b                                              # the fixture's SOF2 case is a header alone: no scan before the end
        elif want == "more than one scan or a non-interleaved scan":
            assert old.info[b].refusal == 9 and old.refusal_name(b).startswith("a baseline file with more than one scan")
        else:
            assert old.refusal_name(b) == want, (b, want, old.refusal_name(b))
    # a file cut inside its last scan's data: accepted without DRI (the decode reports it), refused with DRI (too few restart markers)
    plain = next(f for f, x in zip(px["files"], px["desc"]) if x.startswith("33x50 4:2:0 gradient"))
    rst = next(f for f, x in zip(px["files"], px["desc"]) if "restart_marker_rows" in x)
    b, e = R.parse(rst)["scans"][-1]["segments"][0]
    cut = JpegPlan([truncated_in_last_scan(plain), rst[:(b + e) // 2], plain[:60], b"", plain + b"trailing bytes"], progressive=True)
    assert [cut.info[b].refusal for b in range(5)] == [0, 11, 12, 1, 0]
    assert lib.gg_jprog_plan_create(None, None, 1, None) < 0 and b"gg_jprog_plan_create: null" in lib.gg_last_error()


def test_mixed_batches_and_what_the_older_entry_points_say(L, px):
    from geoguessr_ai_amd.training.jpeg import DeviceJpegDecoder, JpegPlan
    lib = L.lib()
    fx = load_fixture()
    base = fx["files"][:12] + [f for f, x in zip(fx["files"], fx["desc"]) if "restart" in x][:4]
    prog = px["files"][:6]
    files = [f for pair in zip(base, prog + prog + prog) for f in pair]
    mixed, plain = JpegPlan(files, progressive=True), JpegPlan(base)
    assert mixed.first_refused == -1 and mixed.rounds == 3
    for n in range(len(base)):                                                               # a baseline file: one scan, and the answers of gg_jpeg_plan_create
        i, j = mixed.info[2 * n], plain.info[n]
        assert (i.height, i.width, i.components, i.hs, i.vs, i.segments, i.refusal) == (j.height, j.width, j.components, j.hs, j.vs, j.segments, 0)
        assert mixed.scans[2 * n] == 1 and mixed.scans[2 * n + 1] in (6, 10)
    scans, order = _scan_table(mixed)
    assert [int(m["base"]) for m in scans if m["img"] % 2 == 0] == [1] * len(base) and all(m["round"] == 1 for m in scans if m["base"])
    # the same files through gg_jpeg_plan_create: refused as today, per image
    today = JpegPlan(files)
    assert today.first_refused == 1 and [today.info[b].refusal for b in range(len(files))] == [0, 2] * len(base)
    assert today.refusal_name(1) == "progressive (SOF2)" and today.scans is None and today.rounds is None
    with pytest.raises(L.GgError, match=r"image 1 is refused: progressive \(SOF2\)"):
        today.require_accepted()
    for fn in (lib.gg_jprog_plan_scans, ):
        assert fn(today.handle, 0) == -1
    assert lib.gg_jprog_plan_rounds(today.handle) == -1 and lib.gg_jprog_workspace_bytes(today.handle) == -1 and lib.gg_jprog_plan_rounds(None) == -1
    # refused on the host before any launch: no device pointer is looked at
    rc = lib.gg_jprog_decode(plain.handle, 256, 1 << 30, 256, 1 << 30, 256, 256, 1 << 30, None)
    assert rc < 0 and b"gg_jprog_decode: the plan was not made by gg_jprog_plan_create" in lib.gg_last_error()
    rc = lib.gg_jpeg_decode(mixed.handle, 256, 1 << 30, 256, 1 << 30, 256, 256, 1 << 30, None)
    assert rc < 0 and b"gg_jpeg_decode: image 1 is progressive (SOF2)" in lib.gg_last_error()
    rc = lib.gg_jscan_decode(mixed.handle, 256, 1 << 30, 256, 1 << 30, 256, None, 256, 1 << 30, None)
    assert rc < 0 and b"gg_jscan_decode: image 1 is progressive (SOF2)" in lib.gg_last_error()
    rc = lib.gg_jprog_decode(mixed.handle, 256, 1 << 30, 256, 1 << 30, 256, 256, mixed.workspace_bytes - 1, None)
    assert rc < 0 and b"gg_jprog_workspace_bytes" in lib.gg_last_error()
    rc = lib.gg_jprog_decode(mixed.handle, 256, 1 << 30, 264, 1 << 30, 256, 256, 1 << 30, None)
    assert rc < 0 and b"16-byte aligned" in lib.gg_last_error()
    assert lib.gg_jprog_decode(mixed.handle, None, 1 << 30, 256, 1 << 30, 256, 256, 1 << 30, None) < 0 and b"null" in lib.gg_last_error()
    assert lib.gg_jprog_decode(mixed.handle, 256, mixed.stream_bytes - 1, 256, 1 << 30, 256, 256, 1 << 30, None) < 0 and b"gg_jpeg_plan_stream_bytes" in lib.gg_last_error()
    # progressive does not combine with split_bytes
    for make in (lambda: JpegPlan(files, split_bytes=64, progressive=True), lambda: DeviceJpegDecoder("cpu", split_bytes=64, progressive=True)):
        with pytest.raises(L.GgError, match="progressive=True does not combine with split_bytes"):
            make()


def test_jprog_header_compiles_as_c_and_the_exports_are_the_declared_and_bound_ones(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_jprog.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_jprog_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.JPROG_SYMBOLS) and len(declared) == 6
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.JPROG_SIGNATURES[n][1]), n
    src = ('#include <stdio.h>\n#include "gg_jprog.h"\nint main(void){printf("%d %d %d %d %d %d %d %d\\n", GG_JPROG_MAX_SCANS, GG_JPROG_BAD_SCRIPT, GG_JPROG_INCOMPLETE, '
           'GG_JPROG_TOO_MANY_SCANS, GG_JPROG_DNL, GG_JPROG_END_REFUSALS, GG_JPEG_NUM_REFUSALS, (int)sizeof(GgJpegInfo)); return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [L.JPROG_MAX_SCANS, 32, 33, 34, 35, 36, 14, 48] and L.JPROG_MAX_SCANS == 64
    nm = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    assert set(re.findall(r"\b(gg_jprog_[a-z0-9_]+)\b", nm)) == set(L.JPROG_SYMBOLS)
    assert len(set(re.findall(r"\b(gg_jpeg_[a-z0-9_]+)\b", nm))) == 11                       # the gg_jpeg_* exports stay the eleven
    assert "gg_jprog" not in open(os.path.join(ROOT, "include", "gg.h")).read()
    assert "gg_jprog.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    line = mk.split("jpeg.hip.o:")[1].split("\n")[0]
    assert "gg_jprog.h" in line and "jpeg_progressive.h" in line
    assert C.sizeof(C.c_int32) * 16 == SCAN_DTYPE.itemsize


# ---------------------------------------------------------------------------------------------------------------- the lane functions under sanitizers
def _file_job(p, data):
    """One file as a job of tests/jprog_entropy_main.cpp: the scans and segments ``p`` names, with the bytes ``data`` has there (``data`` may be a cut or damaged
    copy of the file ``p`` was parsed from: the plan's table is made from the headers, which such a copy shares)"""
    out = struct.pack("<6i", p["ncomp"], p["hs"], p["vs"], p["mcux"], p["mcuy"], len(p["scans"]))
    none = ([0] * 16, [])
    for s in p["scans"]:
        out += struct.pack("<9i", sum(1 << c for c in s["comps"]), s["Ss"], s["Se"], s["Ah"], s["Al"], s["bw"], s["bh"], s["ri"], len(s["segments"]))
        out += b"".join(_table(s["dc"].get(c, none)) for c in range(3)) + _table(s["ac"] or none)
        for b, e in s["segments"]:
            seg = data[b:e]
            out += struct.pack("<i", len(seg)) + seg
    return out


@pytest.fixture(scope="module")
def jprog_exe():
    d = tempfile.mkdtemp(prefix="jprog_entropy_")
    exe = os.path.join(d, "jprog_entropy_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",         # the runtimes inside the program: it runs in whatever environment the suite runs in
                           os.path.join(ROOT, "tests", "jprog_entropy_main.cpp"), "-o", exe])
    return exe


def _run(exe, jobs):
    """-> [(status, int16 coefficients)]; asserts a clean exit (the program's own checks of the step bound and of every segment's own elements among them) and no
    sanitizer report"""
    with tempfile.TemporaryDirectory() as d:
        jp, rp = os.path.join(d, "jobs"), os.path.join(d, "results")
        with open(jp, "wb") as fh:
            fh.write(struct.pack("<i", len(jobs)) + b"".join(jobs))
        r = subprocess.run([exe, jp, rp], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
        raw, out, at = open(rp, "rb").read(), [], 0
        for _ in jobs:
            status, n = struct.unpack_from("<2i", raw, at)
            at += 8
            out.append((status, np.frombuffer(raw, np.int16, n, at).reshape(-1, 64)))
            at += 2 * n
        assert at == len(raw)
        return out


def host_status(exe, files):
    """Per file, by the host program: the status gg_jprog_decode must report for it (tests/test_gpu_jprog.py).  A file cut short is taken with the scans of its
    headers, as the plan takes it."""
    return [st for st, _ in _run(exe, [_file_job(R.parse(f), f) for f in files])]


def test_lane_functions_on_every_golden_under_sanitizers(px, parsed, coefs, jprog_exe):
    res = _run(jprog_exe, [_file_job(p, f) for p, f in zip(parsed, px["files"])])
    for n, ((status, got), ref) in enumerate(zip(res, coefs)):
        assert status == 0 and np.array_equal(got, ref), (n, px["desc"][n], status, int((got != ref).sum()))


def truncation_files(px):
    """Two small restart-free files: Pillow's 16x16 4:2:0 (10 scans, refinements among them) and the grey file whose DC is refined three times"""
    picks = [next(i for i, d in enumerate(px["desc"]) if d.startswith("16x16 4:2:0 ")), next(i for i, d in enumerate(px["desc"]) if "grey script: DC with three" in d)]
    return [px["files"][i] for i in picks]


def test_lane_functions_on_every_truncation_of_two_files_under_sanitizers(px, jprog_exe):
    rng = np.random.default_rng(11)
    for f in truncation_files(px):
        p = R.parse(f)
        first = p["scans"][0]["segments"][0][0]
        cuts = list(range(first, len(f)))
        res = _run(jprog_exe, [_file_job(p, f[:cut]) for cut in cuts])
        assert all(st in (0, 1, 2, 3) for st, _ in res)
        last = p["scans"][-1]["segments"][-1]
        assert all(st != 0 for (st, _), cut in zip(res, cuts) if cut < last[1] - 2), [cut for (st, _), cut in zip(res, cuts) if st == 0]      # a cut file is reported
        for n in list(rng.integers(0, len(cuts), 40)):                                       # and the restatement says the same of it
            want, st = R.coefficients(f[:cuts[n]], p)
            assert (st != 0) == (res[n][0] != 0) and (st != 0 or np.array_equal(want, res[n][1])), (cuts[n], st, res[n][0])


def test_lane_functions_on_2000_corruptions_under_sanitizers(px, parsed, jprog_exe):
    rng = np.random.default_rng(2026)
    cases = []
    for t in range(2000):
        n = int(rng.integers(len(parsed)))
        p, f = parsed[n], px["files"][n]
        s = p["scans"][int(rng.integers(len(p["scans"])))]
        b, e = s["segments"][int(rng.integers(len(s["segments"])))]
        if e <= b:
            continue
        a = bytearray(f)
        a[int(rng.integers(b, e))] = int(rng.integers(256))
        cases.append((p, bytes(a)))                                                          # a marker made this way ends the segment's data where it stands
    res = _run(jprog_exe, [_file_job(p, f) for p, f in cases])                               # a clean exit: no report, the step bound and every segment's own elements held
    assert len(cases) > 1900 and all(st in (0, 1, 2, 3) for st, _ in res) and {st for st, _ in res} >= {0, 1, 2}
    for n in list(rng.integers(0, len(cases), 60)):
        want, st = R.coefficients(cases[n][1], cases[n][0])
        assert (st != 0) == (res[n][0] != 0) and (st != 0 or np.array_equal(want, res[n][1])), (n, st, res[n][0])
