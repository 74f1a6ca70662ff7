"""Memory discipline of include/gg_jpeg.h, in the way tests/test_gpu_guards_aug.py holds its header: every device buffer of a gg_jpeg_decode call lives in a guarded
buffer (tests/guards.py) -- the stream buffer, the packed output, the status array and the workspace at EXACTLY gg_jpeg_workspace_bytes -- each case runs under the
NaN fill and the large-finite fill (which is also what the workspace holds before the call), and asserts that the stream buffer is unchanged, that only -- and all
of -- the logical outputs were written (the alignment gaps between the images are row padding here: every case takes files of one size), that the two runs agree
bit for bit, and that the bytes are Pillow's (tests/golden/jpeg_pil.npz).

CASES is the registry; test_every_jpeg_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_guards import run_guarded
from tests.test_jpeg_cpu import load_fixture

gpu = pytest.mark.gpu
CASES = {}
HOST_ONLY = "host memory only: no device pointer is taken"
EXEMPT = {n: HOST_ONLY for n in ("gg_jpeg_refusal_name", "gg_jpeg_plan_create", "gg_jpeg_plan_destroy", "gg_jpeg_plan_info", "gg_jpeg_plan_first_refused",
                                 "gg_jpeg_plan_stream_bytes", "gg_jpeg_plan_table_bytes", "gg_jpeg_plan_output_bytes", "gg_jpeg_plan_fill")}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def test_every_jpeg_entry_point_is_guarded_or_exempt():
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_jpeg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_jpeg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    assert guarded == {"gg_jpeg_workspace_bytes", "gg_jpeg_decode"} and len(declared) == 11


@case("gg_jpeg_workspace_bytes", "gg_jpeg_decode")
@gpu
@pytest.mark.parametrize("size", ["17x23", "33x50", "64x48", "3x70"])
def test_jpeg_decode(size):
    """Every golden of one size (all samplings and grey; 33x50 adds restart segments and the COM / APP1 file, 64x48 one restart interval per MCU row, 3x70 the
    replicated narrow chroma) in one call, with one file cut short among them: its image is all zeros."""
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    from tests.test_jpeg_cpu import truncated
    fx = load_fixture()
    idx = [i for i, d in enumerate(fx["desc"]) if d.startswith(size + " ")]
    files, want = [fx["files"][i] for i in idx], [fx["rgb"][i] for i in idx]
    cut = next(n for n, i in enumerate(idx) if "restart" not in fx["desc"][i])
    files.insert(1, truncated(files[cut])); want.insert(1, np.zeros_like(want[cut]))
    B, nbytes = len(files), want[0].size
    ld = (nbytes + 255) // 256 * 256
    assert B >= 5 and all(w.size == nbytes for w in want) and (ld > nbytes or size == "64x48")

    def call(G, L):
        plan = JpegPlan(files)
        plan.require_accepted()
        assert plan.output_bytes == B * ld and [i.out_offset for i in plan.info] == [b * ld for b in range(B)]
        host = torch.empty(plan.stream_bytes, dtype=torch.uint8)
        plan.fill(host.data_ptr())
        stream_buf = G.inp("stream", host)
        out = G.out("out", B, nbytes, torch.uint8, ld=ld)
        status = G.out("status", 1, B, torch.int32)
        need = L.lib().gg_jpeg_workspace_bytes(plan.handle)
        assert need == plan.workspace_bytes > 0
        ws = G.scratch("workspace", need, row_bytes=8 * 128)
        L.check(L.lib().gg_jpeg_decode(plan.handle, stream_buf.ptr, plan.stream_bytes, out.ptr, B * ld, status.ptr, ws.ptr, need, L.stream()), "gg_jpeg_decode")
        host.zero_()                                      # the host copy is not read after the call returns
        plan.close()

        def check(val):
            st = val["status"].numpy().reshape(-1)
            assert all(0 <= int(s) <= 3 for s in st) and [int(s) != 0 for s in st] == [b == 1 for b in range(B)], st      # every status written (they start as -1)
            got = val["out"].numpy()
            for b, w in enumerate(want):
                assert np.array_equal(got[b].reshape(w.shape), w), (size, b)
        return {"out": out, "status": status}, check
    run_guarded(call)
