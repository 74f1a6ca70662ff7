"""Memory discipline of include/gg_pano.h, in the way tests/test_gpu_guards_eval.py holds its header: every device tensor of a gg_pano_batch call lives in a guarded
buffer (tests/guards.py) -- the packed sources, dst, the resized uint8 output and the workspace at EXACTLY gg_pano_workspace_bytes -- the source and both outputs 16
bytes off their alignment; each case runs under the NaN fill and the large-finite fill (which is also what the workspace holds before the call) and asserts that the
sources are unchanged, that only -- and all of -- the logical outputs were written (the gaps between the packed images and between the resized images included), that
the two runs agree bit for bit, and that the values are Pillow's and torch's (tests/golden/pano_pil.npz).

CASES is the registry; test_every_pano_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import pano_ref as R
from tests.pano_cases import MEAN, ROOT, STD, PanoTables, load_cases
from tests.test_gpu_guards import run_guarded

gpu = pytest.mark.gpu
F32, U8 = torch.float32, torch.uint8
GOLDEN = load_cases()
CASES = {}
EXEMPT = {"gg_pano_resized_size": "host arithmetic on four integers: it takes no device pointer"}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def test_every_pano_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_pano.h is called by a guard case of this file or is in EXEMPT with its reason -- exactly one of the two; and a case really calls
    what it registers."""
    from tests.test_guards_cpu import _coverage_gaps
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_pano.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    src = open(__file__).read()
    for e in guarded:
        assert re.search(r"\b" + e + r"\b", src[src.index("def _guarded_call("):])
    for victim in ("gg_pano_workspace_bytes", "gg_pano_batch"):
        assert _coverage_gaps(declared, guarded - {victim}, EXEMPT)[0] == [victim]
    assert len(guarded) == 2 and len(declared) == 3 and list(EXEMPT) == ["gg_pano_resized_size"]


def _guarded_call(srcs, slots, rs, target, normalize):
    """gg_pano_batch under guard bands: src exactly the packed bytes (1-byte gaps: unaligned images), dst exactly [S * 3 * Ht, Wt] f32, dst_u8 exactly the resized
    images with 2-byte gaps, the workspace exactly gg_pano_workspace_bytes(args); the host tables are wiped right after the call returns."""
    Ht, Wt = target
    flat = np.asarray(slots, np.int32).reshape(-1)
    S = flat.size
    sizes = [R.resized_size(s.shape[0], s.shape[1], rs) for s in srcs]
    u8_starts, at = [], 0
    for hr, wr in sizes:
        u8_starts.append(at)
        at += 3 * hr * wr + 2
    u8_total = at - 2
    want = [R.view(s, rs, target, MEAN if normalize else None, STD if normalize else None) for s in srcs]
    missing = R.view(None, rs, target, MEAN if normalize else None, STD if normalize else None)[1]

    def call(G, L):
        t = PanoTables(L, srcs, flat, rs, target, normalize, gap=1)
        a = t.args
        src = G.inp("src", torch.from_numpy(t.host[:t.host.size - 1]), misalign=16)
        a.src_bytes = t.host.size - 1
        dst = G.out("dst", S * 3 * Ht, Wt, F32, misalign=16)
        dst_u8 = G.out("dst_u8", 1, u8_total, U8, misalign=16)
        u8_offsets = np.array(u8_starts, np.int64)
        need = L.lib().gg_pano_workspace_bytes(C.byref(a))
        assert need > 0, L.lib().gg_last_error()
        ws = G.scratch("workspace", need, row_bytes=3 * 70 + 4)
        a.src, a.dst, a.dst_u8, a.u8_offsets, a.dst_u8_bytes, a.workspace, a.workspace_bytes = src.ptr, dst.ptr, dst_u8.ptr, u8_offsets.ctypes.data, u8_total, ws.ptr, need
        L.check(L.lib().gg_pano_batch(C.byref(a), L.stream()), "gg_pano_batch")
        t.offsets[...] = -1
        t.heights[...] = 0
        t.widths[...] = 0
        t.slots[...] = 99
        u8_offsets[...] = -1

        def check(val):
            flat8 = val["dst_u8"].numpy().reshape(-1)
            gaps = np.ones(u8_total, bool)
            for o, (hr, wr), (w8, _) in zip(u8_starts, sizes, want):
                assert np.array_equal(flat8[o:o + 3 * hr * wr].reshape(hr, wr, 3), w8)
                gaps[o:o + 3 * hr * wr] = False
            assert (flat8[gaps] == 0xFF).all()                        # the bytes between the resized images are as the guard left them
            d = val["dst"].numpy().reshape(S, 3, Ht, Wt)
            for s, img in enumerate(flat):
                assert np.abs(d[s] - (missing if img < 0 else want[img][1])).max() <= 1e-5, s
        return {"dst": dst, "dst_u8": dst_u8}, check
    run_guarded(call)


@case("gg_pano_workspace_bytes", "gg_pano_batch")
@gpu
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("i", range(len(GOLDEN)))
def test_pano_golden_case(i, normalize):
    c = GOLDEN[i]
    _guarded_call([c["src"]], [0], c["rs"], c["target"], normalize)


@case("gg_pano_workspace_bytes", "gg_pano_batch")
@gpu
@pytest.mark.parametrize("slots", [[[-1, 0, 1, 2], [-1, -1, -1, -1], [3, 4, 5, -1]], [6, 5, 4, 3, 2, 1, 0], [[2, 2], [0, 2]]])
def test_pano_slots(slots):
    _guarded_call([GOLDEN[i]["src"] for i in (0, 1, 2, 4, 6, 7, 8)], slots, 8, (12, 20), True)
