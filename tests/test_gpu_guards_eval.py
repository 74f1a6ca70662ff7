"""Memory discipline of include/gg_eval.h, in the way tests/test_gpu_guards_aug.py holds its header: every device tensor of a call lives in a guarded buffer
(tests/guards.py) -- the packed sources, dst, dst_u8 and the workspace at EXACTLY gg_eval_workspace_bytes -- each case runs under the NaN fill and the large-finite
fill (which is also what the workspace holds before the call), and asserts that the sources are unchanged, that only -- and all of -- the logical outputs were
written, that the two runs agree bit for bit, and that the bytes are Pillow's (tests/golden/eval_batch_pil.npz).

CASES is the registry; test_every_eval_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_guards import run_guarded

gpu = pytest.mark.gpu
F32, U8 = torch.float32, torch.uint8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = {}
EXEMPT = {}                  # gg_eval_workspace_bytes touches no device memory, but every case calls it for the workspace's size: nothing is exempt


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def _declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_eval.h")).read(), flags=re.S)
    return set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))


def test_every_eval_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_eval.h is called by a guard case of this file or is in EXEMPT with its reason -- exactly one of the two; and a case really calls
    what it registers."""
    from tests.test_guards_cpu import _coverage_gaps
    declared = _declared()
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing, f"entry points of include/gg_eval.h with neither a guard test nor an exemption: {missing}"
    assert not unknown, f"registry / exemption names the header does not declare: {unknown}"
    assert not both, f"both guarded and exempt: {both}"
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    for victim in ("gg_eval_workspace_bytes", "gg_eval_batch"):
        assert _coverage_gaps(declared, guarded - {victim}, EXEMPT)[0] == [victim]
    assert len(guarded) == len(declared) == 2 and not EXEMPT


# B = 5 mixed fixture images with a 32 x 32 crop: both passes (a reduction and the up-scale), neither pass with a column offset, only the horizontal pass, only the vertical pass
MIXED = (0, 3, 4, 12, 13)


@case("gg_eval_workspace_bytes", "gg_eval_batch")
@gpu
@pytest.mark.parametrize("want_u8", [True, False])
def test_eval_batch(want_u8):
    """gg_eval_batch: src exactly the packed bytes (1-byte gaps: unaligned images), dst exactly [B * 3 * S, S] f32, dst_u8 exactly [B * S, 3 S] bytes, the workspace
    exactly gg_eval_workspace_bytes(args) and holding the fill (NaN bytes / 0x47) before the call; offsets, sizes and geometry are host memory and are wiped right
    after the call returns."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_batch_pil.npz"))
    S, B = 32, len(MIXED)
    srcs, want = [g[f"src{i}"] for i in MIXED], np.stack([g[f"crop{i}"] for i in MIXED])
    starts, at = [], 0
    for s in srcs:
        starts.append(at)
        at += s.size + 1
    host = np.zeros(at - 1, np.uint8)
    for s, o in zip(srcs, starts):
        host[o:o + s.size] = s.reshape(-1)
    packed = torch.from_numpy(host)

    def call(G, L):
        offsets = np.array(starts, np.int64)
        heights, widths = np.array([s.shape[0] for s in srcs], np.int32), np.array([s.shape[1] for s in srcs], np.int32)
        geom = np.ascontiguousarray(np.stack([g["geom"][i] for i in MIXED]).astype(np.int32))
        src = G.inp("src", packed)
        dst = G.out("dst", B * 3 * S, S, F32)
        a = L.EvalArgs()
        a.src, a.src_bytes = src.ptr, packed.numel()
        a.offsets, a.heights, a.widths, a.geom = offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data, geom.ctypes.data
        a.B, a.Hc, a.Wc, a.filter, a.mul_rescale, a.normalize = B, S, S, 3, 0, 1
        a.mean, a.std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        need = L.lib().gg_eval_workspace_bytes(C.byref(a))
        assert need > 0
        ws = G.scratch("workspace", need, row_bytes=3 * S * 83)
        outs = {"dst": dst}
        if want_u8:
            outs["dst_u8"] = G.out("dst_u8", B * S, 3 * S, U8)
            a.dst_u8 = outs["dst_u8"].ptr
        a.dst, a.workspace, a.workspace_bytes = dst.ptr, ws.ptr, need
        L.check(L.lib().gg_eval_batch(C.byref(a), L.stream()), "gg_eval_batch")
        offsets[...] = -1
        heights[...] = 0
        widths[...] = 0
        geom[...] = 0

        def check(val):
            if want_u8:
                assert np.array_equal(val["dst_u8"].numpy().reshape(B, S, S, 3), want)
            x = want.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)
            x = (x - np.asarray(MEAN, np.float32).reshape(1, 3, 1, 1)) / np.asarray(STD, np.float32).reshape(1, 3, 1, 1)
            assert np.abs(val["dst"].numpy().reshape(B, 3, S, S) - x).max() <= 1e-6
        return outs, check
    run_guarded(call)
