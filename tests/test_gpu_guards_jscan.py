"""Memory discipline of include/gg_jscan.h, in the way tests/test_gpu_guards_jpeg.py holds include/gg_jpeg.h: every device buffer of a gg_jscan_decode call lives in
a guarded buffer (tests/guards.py) -- the stream buffer, the packed output, the status and slow arrays and the workspace at EXACTLY gg_jscan_workspace_bytes --
each case runs under the NaN fill and the large-finite fill (which is also what the workspace holds before the call), and asserts that the stream buffer is
unchanged, that only -- and all of -- the logical outputs were written (the output's row padding, the neighbours of status and slow, the workspace's tail), that
the two runs agree bit for bit, and that the bytes are Pillow's (tests/golden/jpeg_split_pil.npz).

CASES is the registry; test_every_jscan_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_guards import run_guarded
from tests.test_jpeg_cpu import truncated
from tests.test_jscan_cpu import load_split_fixture

gpu = pytest.mark.gpu
CASES = {}
HOST_ONLY = "host memory only: no device pointer is taken"
EXEMPT = {n: HOST_ONLY for n in ("gg_jscan_plan_create", "gg_jscan_plan_subsegments", "gg_jscan_plan_total_subsegments")}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def test_every_jscan_entry_point_is_guarded_or_exempt():
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_jscan.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_jscan_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    assert guarded == {"gg_jscan_workspace_bytes", "gg_jscan_decode"} and len(declared) == 5


@case("gg_jscan_workspace_bytes", "gg_jscan_decode")
@gpu
@pytest.mark.parametrize("size,split", [("160x160", 16), ("160x160", 512), ("200x136", 64), ("200x136", 512)])
def test_jscan_decode(size, split):
    """Every file of one size (all samplings and grey, the optimised tables, the checkerboard's stuffed bytes, restart intervals of four MCU rows) in one call, with
    one file cut short among them: its image is all zeros.  200x136: 81600 bytes an image, so rows of the output are padded; 160x160: no padding at all."""
    from geoguessr_ai_amd.training.jpeg import JpegPlan
    sx = load_split_fixture()
    idx = [i for i, d in enumerate(sx["desc"]) if d.startswith(size + " ")]
    files, want = [sx["files"][i] for i in idx], [sx["rgb"][i] for i in idx]
    cut = next(n for n, i in enumerate(idx) if "restart" not in sx["desc"][i])
    files.insert(1, truncated(files[cut])); want.insert(1, np.zeros_like(want[cut]))
    B, nbytes = len(files), want[0].size
    ld = (nbytes + 255) // 256 * 256
    assert B >= 5 and all(w.size == nbytes for w in want) and (ld > nbytes) == (size == "200x136")

    def call(G, L):
        plan = JpegPlan(files, split_bytes=split)
        plan.require_accepted()
        assert plan.output_bytes == B * ld and [i.out_offset for i in plan.info] == [b * ld for b in range(B)] and plan.total_subsegments > 4 * B
        host = torch.empty(plan.stream_bytes, dtype=torch.uint8)
        plan.fill(host.data_ptr())
        stream_buf = G.inp("stream", host)
        out = G.out("out", B, nbytes, torch.uint8, ld=ld)
        status = G.out("status", 1, B, torch.int32)
        slow = G.out("slow", 1, B, torch.int32)
        need = L.lib().gg_jscan_workspace_bytes(plan.handle)
        assert need == plan.workspace_bytes > plan.base_workspace_bytes
        ws = G.scratch("workspace", need, row_bytes=8 * 128)
        L.check(L.lib().gg_jscan_decode(plan.handle, stream_buf.ptr, plan.stream_bytes, out.ptr, B * ld, status.ptr, slow.ptr, ws.ptr, need, L.stream()), "gg_jscan_decode")
        host.zero_()                                      # the host copy is not read after the call returns
        subs = list(plan.subsegments)
        plan.close()

        def check(val):
            st = val["status"].numpy().reshape(-1)
            assert all(0 <= int(s) <= 3 for s in st) and [int(s) != 0 for s in st] == [b == 1 for b in range(B)], st      # every status written (they start as -1)
            sl = val["slow"].numpy().reshape(-1)
            assert all(0 <= int(s) <= n for s, n in zip(sl, subs)), (sl, subs)               # every slow count written
            got = val["out"].numpy()
            for b, w in enumerate(want):
                assert np.array_equal(got[b].reshape(w.shape), w), (size, split, b)
        return {"out": out, "status": status, "slow": slow}, check
    run_guarded(call)
