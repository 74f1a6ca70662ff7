"""CPU-only checks of the JPEG decode with many lanes inside one scan (include/gg_jscan.h, csrc/jpeg_entropy.h's jscan_* functions): the new fixture against
Pillow and the numpy restatement; the four passes, lane by lane with the kernels' very statements, in a stand-alone program under AddressSanitizer and UBSan
(tests/jscan_main.cpp: a child process with its own main, nothing is loaded into Python) against the sequential decoder, tests/jpeg_ref.py's coefficients and the
scheme's restatement (tests/jscan_ref.py); the host-side plan's sub-segment table; the header as C against the binding.  Nothing here needs a GPU; everything here
fails without the header, the symbols and the functions."""
import ctypes as C
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import jpeg_ref as J
from tests import jscan_ref as S
from tests.test_jpeg_cpu import _segments, _table, fill_byte_files, load_fixture, truncation_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_split_pil.npz")
SUB_DTYPE = np.dtype([("begin", "<i8"), ("end", "<i8"), ("dbeg", "<i8"), ("dend", "<i8"), ("seg", "<i4"), ("idx", "<i4"), ("nsub", "<i4"), ("pad", "<i4")])


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def load_split_fixture():
    g = np.load(SPLIT_FIXTURE)
    n = len(g["desc"])
    return {"files": [g[f"file_{i}"].tobytes() for i in range(n)], "rgb": [g[f"rgb_{i}"] for i in range(n)], "desc": [str(d) for d in g["desc"]]}


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def sx():
    return load_split_fixture()


@pytest.fixture(scope="module")
def scans(fx, sx):
    """Every scan of both fixtures, decoded once by tests/jpeg_ref.py: [(parse, segment bytes, MCUs, the segment's coefficients)]"""
    out = []
    for f in fx["files"] + sx["files"]:
        p, segs = _segments(f)
        coef, status = J.coefficients(f, p)
        assert status == 0
        for data, mcus, blk0 in segs:
            out.append((p, data, mcus, coef[blk0:blk0 + mcus * p["bpm"]]))
    return out


def test_split_fixture_covers_what_it_should(sx):
    d = sx["desc"]
    assert 8 <= len(d) <= 12 and os.path.getsize(SPLIT_FIXTURE) < 1 << 20
    assert {x.split()[0] for x in d} == {"160x160", "200x136"}
    assert {x.split()[1] for x in d} == {"4:2:0", "4:2:2", "4:4:4", "grey"}
    assert {"q50", "q90", "q95"} <= {x.split()[3] for x in d}
    for word in ("optimize", "checker", "gradient", "restart_marker_rows"):
        assert any(word in x for x in d), word
    plain = [f for f, x in zip(sx["files"], d) if "restart" not in x]
    assert len(plain) >= 8 and all(len(J.parse(f)["segments"]) == 1 for f in plain)
    assert sum(10_000 <= len(f) <= 40_000 for f in plain) >= 5
    checker = sx["files"][next(i for i, x in enumerate(d) if "checker" in x)]
    assert checker.count(b"\xff\x00") > 1000                                                 # rich in stuffed bytes
    rst = [f for f, x in zip(sx["files"], d) if "restart" in x]
    assert len(rst) == 2 and all(len(J.parse(f)["segments"]) in (3, 5) for f in rst)         # four MCU rows to an interval: both mechanisms combine


def test_restatement_equals_pillow_on_the_split_fixture(sx):
    for i, (f, want) in enumerate(zip(sx["files"], sx["rgb"])):
        assert np.array_equal(J.decode(f), want), (i, sx["desc"][i])


# ---------------------------------------------------------------------------------------------------------------- the four passes under sanitizers
def _job(p, data, mcus, split):
    """One segment as a job of tests/jscan_main.cpp"""
    nc = p["ncomp"]
    blocks = [p["hs"] * p["vs"], 1, 1] if nc == 3 else [1, 0, 0]
    tabs = b"".join(_table(p["dc"][min(c, nc - 1)]) + _table(p["ac"][min(c, nc - 1)]) for c in range(3))
    return struct.pack("<7i", nc, blocks[0], blocks[1], blocks[2], mcus, len(data), split) + tabs + data


def _restated(p, data, mcus, split):
    nc = p["ncomp"]
    return S.run(data, mcus, nc, [p["hs"] * p["vs"], 1, 1] if nc == 3 else [1, 0, 0], p["dc"], p["ac"], split)


def build_jscan_exe():
    d = tempfile.mkdtemp(prefix="jscan_")
    exe = os.path.join(d, "jscan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",         # the runtimes inside the program: it runs in whatever environment the suite runs in
                           os.path.join(ROOT, "tests", "jscan_main.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def jscan_exe():
    return build_jscan_exe()


def host_counts(exe, files, split):
    """Per file, by the host program: (status, slow, sub-segments) over its segments -- what gg_jscan_decode must report for it (tests/test_gpu_jscan.py).  A file
    cut short or damaged is taken with the MCU counts of its header, as the plan takes it."""
    jobs, owner = [], []
    for b, f in enumerate(files):
        p, segs = _segments(f)
        for data, mcus, _ in segs:
            jobs.append(_job(p, data, mcus, split)); owner.append(b)
    out = [[0, 0, 0] for _ in files]
    for b, (status, seq, slow, nsub, _) in zip(owner, _run(exe, jobs)):
        assert status == seq
        out[b] = [max(out[b][0], status), out[b][1] + slow, out[b][2] + nsub]
    return [tuple(o) for o in out]


def _run(exe, jobs):
    """-> [(status, sequential status, slow, sub-segments, int16 coefficients)]; asserts a clean exit (the program's own checks of its loop bounds and of its
    sub-segment table among them) and no sanitizer report"""
    with tempfile.TemporaryDirectory() as d:
        jp, rp = os.path.join(d, "jobs"), os.path.join(d, "results")
        with open(jp, "wb") as fh:
            fh.write(struct.pack("<i", len(jobs)) + b"".join(jobs))
        r = subprocess.run([exe, jp, rp], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
        raw, out, at = open(rp, "rb").read(), [], 0
        for _ in jobs:
            status, seq, slow, nsub, n = struct.unpack_from("<5i", raw, at)
            at += 20
            out.append((status, seq, slow, nsub, np.frombuffer(raw, np.int16, n, at).reshape(-1, 64)))
            at += 2 * n
        assert at == len(raw)
        return out


@pytest.mark.parametrize("split", [8, 16, 64, 512])
def test_the_four_passes_on_every_scan_of_both_fixtures_under_sanitizers(scans, jscan_exe, split):
    res = _run(jscan_exe, [_job(p, data, mcus, split) for p, data, mcus, _ in scans])
    many = 0
    for n, ((status, seq, slow, nsub, got), (p, data, mcus, ref)) in enumerate(zip(res, scans)):
        want = _restated(p, data, mcus, split)
        assert (status, seq, slow, nsub) == (0, 0, want["slow"], want["nsub"]), (n, split, status, seq, slow, nsub, want)
        assert nsub == 1 or len(data) >= 2 * split
        assert np.array_equal(got, ref), (n, split, int((got != ref).sum()))                 # every coefficient written (the canary is gone), and the right one
        many += nsub > 1
    assert many >= 10                                                                        # at 512 bytes the new fixture's scans; below that most scans


def test_most_sub_segments_of_the_split_fixture_are_reached_by_a_speculative_lane(sx):
    """At 512 bytes at most a tenth of every file's sub-segments take the slow path (what tests/golden/make_golden_jpeg_split.py asserted when it wrote the files)"""
    for f, d in zip(sx["files"], sx["desc"]):
        p, segs = _segments(f)
        runs = [_restated(p, data, mcus, 512) for data, mcus, _ in segs]
        nsub, slow = sum(r["nsub"] for r in runs), sum(r["slow"] for r in runs)
        assert nsub >= 2 and 10 * slow <= nsub, (d, nsub, slow)


def test_every_truncation_of_two_files_and_sampled_cuts_of_two_large_ones_under_sanitizers(fx, sx, jscan_exe):
    rng = np.random.default_rng(7)
    cases = []
    for f in truncation_files(fx):
        p, segs = _segments(f)
        data, mcus, _ = segs[0]
        cases += [(p, data[:cut], mcus) for cut in range(len(data))]
    for f in sx["files"][:2]:                                                                # many sub-segments at 512 bytes too
        p, segs = _segments(f)
        data, mcus, _ = segs[0]
        cases += [(p, data[:int(cut)], mcus) for cut in rng.integers(0, len(data), 40)]
    for split in (16, 512):
        res = _run(jscan_exe, [_job(p, data, mcus, split) for p, data, mcus in cases])
        for n, ((status, seq, slow, nsub, _), (p, data, mcus)) in enumerate(zip(res, cases)):
            assert status == seq and status in (0, 1, 2, 3), (n, split, status, seq)         # jpeg_decode_segment's status on the same bytes
        assert sum(r[0] != 0 for r in res) >= len(cases) - 8 and any(r[3] > 1 and r[0] != 0 for r in res)
        for n in list(rng.integers(0, len(cases), 60)):                                      # and the restatement's, slow counts included
            want = _restated(*cases[n], split)
            assert (res[n][0], res[n][2], res[n][3]) == (want["status"], want["slow"], want["nsub"]), (n, split, res[n][:4], want)


def test_2000_corruptions_under_sanitizers(scans, jscan_exe):
    rng = np.random.default_rng(2026)
    pool = [(p, data, mcus) for p, data, mcus, _ in scans if len(data) > 0]
    large = [x for x in pool if len(x[1]) >= 4096]
    cases = []
    for t in range(2000):
        p, data, mcus = large[int(rng.integers(len(large)))] if t % 8 == 0 else pool[int(rng.integers(len(pool)))]
        a = bytearray(data)
        a[int(rng.integers(len(a)))] = int(rng.integers(256))
        cases.append((p, bytes(a), mcus))                                                    # a marker made this way ends the data where it stands, for every lane
    for split in (16, 512):
        res = _run(jscan_exe, [_job(p, data, mcus, split) for p, data, mcus in cases])      # a clean exit: no report, and the program's own bounds held
        assert all(status == seq and status in (0, 1, 2, 3) for status, seq, _, _, _ in res), [(n, r[:4]) for n, r in enumerate(res) if r[0] != r[1]][:5]
        assert {r[0] for r in res} >= {0, 1} and sum(r[3] > 1 and r[0] != 0 for r in res) >= (5 if split == 512 else 100)
        for n in list(rng.integers(0, len(cases), 30)):
            want = _restated(*cases[n], split)
            assert (res[n][0], res[n][2], res[n][3]) == (want["status"], want["slow"], want["nsub"]), (n, split, res[n][:4], want)


# ---------------------------------------------------------------------------------------------------------------- the host-side plan
def _sub_table(plan):
    """The sub-segment table of a plan's table block: its last region (csrc/jpeg.hip lays the block out as images | segments | quantisers | Huffman tables |
    first sub-segment of every segment | sub-segments, each region rounded up to 256 bytes)"""
    buf = np.zeros(plan.stream_bytes, np.uint8)
    plan.fill(buf.ctypes.data)
    n = plan.total_subsegments
    size = (max(n, 1) * SUB_DTYPE.itemsize + 255) // 256 * 256
    return np.frombuffer(buf[plan.table_bytes - size:plan.table_bytes].tobytes(), SUB_DTYPE, n)


def test_plan_cuts_every_segment_where_the_restatement_cuts_it_and_never_behind_an_ff(L, fx, sx):
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    filled, _ = fill_byte_files(fx)
    files = fx["files"] + sx["files"] + filled
    for split in (8, 16, 64, 512):
        plan, plain = JpegPlan(files, split_bytes=split), JpegPlan(files)
        assert plan.first_refused == -1 and plan.split_bytes == split
        for b in range(plan.B):                                                              # every gg_jpeg_plan_* answer is the plain plan's, but for the longer table block
            i, j = plan.info[b], plain.info[b]
            assert (i.height, i.width, i.components, i.hs, i.vs, i.segments, i.refusal, i.out_offset) == (j.height, j.width, j.components, j.hs, j.vs, j.segments, j.refusal, j.out_offset)
        assert plan.output_bytes == plain.output_bytes and plan.base_workspace_bytes == plain.workspace_bytes < plan.workspace_bytes
        assert plan.table_bytes > plain.table_bytes and plan.table_bytes % 256 == 0
        subs, at, seg, moved = _sub_table(plan), 0, 0, 0
        assert plan.total_subsegments == sum(plan.subsegments) == len(subs)
        for b, f in enumerate(files):
            p, n_img = J.parse(f), 0
            for sb, se in p["segments"]:
                data = f[sb:se]
                cuts, dtotal = S.cut(data, split)
                mine = subs[at:at + len(cuts)]
                assert [(int(m["begin"]), int(m["dbeg"])) for m in mine] == cuts, (split, b)
                assert mine["begin"][0] == 0 and mine["end"][-1] == len(data) and (mine["end"][:-1] == mine["begin"][1:]).all()       # the sub-segments tile the segment
                assert mine["dend"][-1] == dtotal and (mine["dend"][:-1] == mine["dbeg"][1:]).all()
                assert (mine["seg"] == seg).all() and mine["idx"].tolist() == list(range(len(cuts))) and (mine["nsub"] == len(cuts)).all()
                assert all(data[int(c) - 1] != 0xFF for c in mine["begin"][1:])              # no boundary behind an FF: none inside FF 00 or a run of fill bytes
                assert len(cuts) == 1 or len(data) >= 2 * split
                assert all(int(m["end"] - m["begin"]) >= split for m in mine) or len(cuts) == 1
                moved += int((np.diff(mine["begin"]) > split).sum())
                at += len(cuts); seg += 1; n_img += len(cuts)
            assert plan.subsegments[b] == n_img
        assert at == len(subs)
        if split <= 16:
            assert moved > 20                                                                # cuts that had to move behind FF 00 or a run of fill bytes
        plan.close(); plain.close()


def test_split_bytes_outside_the_range_and_a_plain_plan_are_refused_by_name(L, fx):
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    lib = L.lib()
    for bad in (-1, 1, 7, (1 << 20) + 1):
        with pytest.raises(L.GgError, match=r"split_bytes=-?\d+ outside \[8, 1048576\]"):
            JpegPlan(fx["files"][:2], split_bytes=bad)
    for ok in (8, 1 << 20):
        plan = JpegPlan(fx["files"][:2], split_bytes=ok)
        assert plan.total_subsegments >= 2
        plan.close()
    plain = JpegPlan(fx["files"][:2])
    assert plain.subsegments is None and lib.gg_jscan_plan_subsegments(plain.handle, 0) == -1 and lib.gg_jscan_plan_total_subsegments(plain.handle) == -1
    assert lib.gg_jscan_workspace_bytes(plain.handle) == -1
    # refused on the host before any launch: no device pointer is looked at
    rc = lib.gg_jscan_decode(plain.handle, 256, 1 << 30, 256, 1 << 30, 256, None, 256, 1 << 30, None)
    assert rc < 0 and b"gg_jscan_decode: the plan has no sub-segment table" in lib.gg_last_error()
    plan = JpegPlan([fx["files"][0], fx["refuse"][fx["refuse_name"].index("progressive (SOF2)")]], split_bytes=64)
    assert plan.subsegments[1] == 0 and lib.gg_jscan_plan_subsegments(plan.handle, 2) == -1
    rc = lib.gg_jscan_decode(plan.handle, 256, 1 << 30, 256, 1 << 30, 256, None, 256, 1 << 30, None)
    assert rc < 0 and b"image 1 is refused: progressive" in lib.gg_last_error()
    good = JpegPlan(fx["files"][:2], split_bytes=64)
    rc = lib.gg_jscan_decode(good.handle, 256, 1 << 30, 256, 1 << 30, 256, None, 256, good.workspace_bytes - 1, None)
    assert rc < 0 and b"gg_jscan_workspace_bytes" in lib.gg_last_error()
    rc = lib.gg_jscan_decode(good.handle, 256, 1 << 30, 264, 1 << 30, 256, None, 256, 1 << 30, None)
    assert rc < 0 and b"16-byte aligned" in lib.gg_last_error()
    assert lib.gg_jscan_decode(good.handle, None, 1 << 30, 256, 1 << 30, 256, None, 256, 1 << 30, None) < 0 and b"null" in lib.gg_last_error()


def test_jscan_header_compiles_as_c_and_the_exports_are_the_declared_and_bound_ones(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_jscan.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_jscan_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.JSCAN_SYMBOLS) and len(declared) == 5
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.JSCAN_SIGNATURES[n][1]), n
    src = ('#include <stdio.h>\n#include "gg_jscan.h"\nint main(void){GgJpegPlan* p = 0; printf("%d %d %d\\n", GG_JSCAN_MIN_SPLIT, GG_JSCAN_MAX_SPLIT, '
           '(int)gg_jscan_plan_total_subsegments(p)); return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
    assert (L.JSCAN_MIN_SPLIT, L.JSCAN_MAX_SPLIT) == (8, 1 << 20)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    assert set(re.findall(r"\b(gg_jscan_[a-z0-9_]+)\b", nm)) == set(L.JSCAN_SYMBOLS)
    assert "gg_jscan.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "gg_jscan.h" in mk.split("jpeg.hip.o:")[1].split("\n")[0]
    assert C.sizeof(C.c_int32) * 12 == SUB_DTYPE.itemsize
