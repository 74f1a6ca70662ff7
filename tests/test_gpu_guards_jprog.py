"""Memory discipline of include/gg_jprog.h, in the way tests/test_gpu_guards_jpeg.py holds include/gg_jpeg.h: every device buffer of a gg_jprog_decode call lives in
a guarded buffer (tests/guards.py) -- the stream buffer, the packed output, the status array and the workspace at EXACTLY gg_jprog_workspace_bytes -- each case
runs under the NaN fill and the large-finite fill (which is also what the workspace holds before the call: the progressive scans write only what they code, so a
coefficient the zero fill missed would show), and asserts that the stream buffer is unchanged, that only -- and all of -- the logical outputs were written (the
output's row padding, the neighbours of status, the workspace's tail), that the two runs agree bit for bit, and that the bytes are Pillow's
(tests/golden/jpeg_prog_pil.npz).

CASES is the registry; test_every_jprog_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_guards import run_guarded
from tests.test_jpeg_cpu import load_fixture
from tests.test_jprog_cpu import load_prog_fixture, truncated_in_last_scan

gpu = pytest.mark.gpu
CASES = {}
HOST_ONLY = "host memory only: no device pointer is taken"
EXEMPT = {n: HOST_ONLY for n in ("gg_jprog_refusal_name", "gg_jprog_plan_create", "gg_jprog_plan_scans", "gg_jprog_plan_rounds")}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def test_every_jprog_entry_point_is_guarded_or_exempt():
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_jprog.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_jprog_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    assert guarded == {"gg_jprog_workspace_bytes", "gg_jprog_decode"} and len(declared) == 6


@case("gg_jprog_workspace_bytes", "gg_jprog_decode")
@gpu
@pytest.mark.parametrize("size", ["33x50", "64x48", "17x33"])
def test_jprog_decode(size):
    """Every progressive file of one size (Pillow's scripts in all samplings and grey, restart intervals, the hand-made scan scripts: non-interleaved DC scans,
    refinements of every kind, 64 and 25 scans, tables and intervals that change between scans) in one call, with two baseline files of that size and one
    progressive file cut short among them: its image is all zeros.  33x50: 4950 bytes an image, so rows of the output are padded; 64x48: no padding at all."""
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    px, fx = load_prog_fixture(), load_fixture()
    idx = [i for i, d in enumerate(px["desc"]) if d.startswith(size + " ")]
    files, want = [px["files"][i] for i in idx], [px["rgb"][i] for i in idx]
    cut = next(n for n, i in enumerate(idx) if "restart" not in px["desc"][i])
    files.insert(1, truncated_in_last_scan(files[cut])); want.insert(1, np.zeros_like(want[cut]))
    w, h = (int(v) for v in size.split("x"))
    twins = [i for i, r in enumerate(fx["rgb"]) if r.shape[:2] == (h, w)][:2]
    for i in twins:
        files.insert(3, fx["files"][i]); want.insert(3, fx["rgb"][i])
    B, nbytes = len(files), want[0].size
    ld = (nbytes + 255) // 256 * 256
    assert B >= 8 and all(x.size == nbytes for x in want) and (ld > nbytes) == (size != "64x48") and (len(twins) == 2 or size == "17x33")

    def call(G, L):
        plan = JpegPlan(files, progressive=True)
        plan.require_accepted()
        assert plan.output_bytes == B * ld and [i.out_offset for i in plan.info] == [b * ld for b in range(B)] and plan.rounds >= 3 and max(plan.scans) >= 10
        host = torch.empty(plan.stream_bytes, dtype=torch.uint8)
        plan.fill(host.data_ptr())
        stream_buf = G.inp("stream", host)
        out = G.out("out", B, nbytes, torch.uint8, ld=ld)
        status = G.out("status", 1, B, torch.int32)
        need = L.lib().gg_jprog_workspace_bytes(plan.handle)
        assert need == plan.workspace_bytes > 0
        ws = G.scratch("workspace", need, row_bytes=8 * 128)
        L.check(L.lib().gg_jprog_decode(plan.handle, stream_buf.ptr, plan.stream_bytes, out.ptr, B * ld, status.ptr, ws.ptr, need, L.stream()), "gg_jprog_decode")
        host.zero_()                                      # the host copy is not read after the call returns
        plan.close()

        def check(val):
            st = val["status"].numpy().reshape(-1)
            assert all(0 <= int(s) <= 3 for s in st) and [int(s) != 0 for s in st] == [b == 1 for b in range(B)], st      # every status written (they start as -1)
            got = val["out"].numpy()
            for b, x in enumerate(want):
                assert np.array_equal(got[b].reshape(x.shape), x), (size, b)
        return {"out": out, "status": status}, check
    run_guarded(call)
