"""Memory discipline of include/gg_aug.h, in the way tests/test_gpu_guards_pad.py holds its header: every device tensor of a call lives in a guarded buffer
(tests/guards.py) -- the packed sources, dst, dst_u8 and the workspace at EXACTLY gg_aug_workspace_bytes -- each case runs under the NaN fill and the large-finite
fill (which is also what the workspace holds before the call), and asserts that the sources are unchanged, that only -- and all of -- the logical outputs were
written, that the two runs agree bit for bit, and that the bytes are those of the numpy restatement (tests/augment_ref.py).

CASES is the registry; test_every_aug_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.test_gpu_guards import run_guarded

gpu = pytest.mark.gpu
F32, U8 = torch.float32, torch.uint8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = {}
EXEMPT = {}                  # gg_aug_workspace_bytes touches no device memory, but every case calls it for the workspace's size: nothing is exempt


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def _declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_aug.h")).read(), flags=re.S)
    return set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))


def test_every_aug_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_aug.h is called by a guard case of this file or is in EXEMPT with its reason -- exactly one of the two; and a case really calls
    what it registers."""
    from tests.test_guards_cpu import _coverage_gaps
    declared = _declared()
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing, f"entry points of include/gg_aug.h with neither a guard test nor an exemption: {missing}"
    assert not unknown, f"registry / exemption names the header does not declare: {unknown}"
    assert not both, f"both guarded and exempt: {both}"
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    for victim in ("gg_aug_workspace_bytes", "gg_aug_batch"):
        assert _coverage_gaps(declared, guarded - {victim}, EXEMPT)[0] == [victim]
    assert len(guarded) == len(declared) == 2 and not EXEMPT


def _batch(layers, seed):
    from geoguessr_ai_amd.finetune_tinyvit.augment import sample_params
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_pil.npz"))
    srcs = [g["src0"], g["src1"], g["src2"], np.ascontiguousarray(g["src1"][::-1])]
    recs = sample_params([s.shape[:2] for s in srcs], 32, f"rand-m9-mstd0.5-inc1-n{layers}", np.random.default_rng(seed), MEAN, "random")
    recs["ops"]["applied"] = 1
    return srcs, recs


# layers / seed / filter / forced ops of image 0: the resize alone; two sampled layers; four layers with both statistics passes (bins, then the grey sum)
@case("gg_aug_workspace_bytes", "gg_aug_batch")
@gpu
@pytest.mark.parametrize("want_u8", [True, False])
@pytest.mark.parametrize("layers,seed,flt,forced", [(0, 1, 3, ()), (2, 2, 2, (R.SHARPNESS, R.ROTATE)), (4, 3, 3, (R.EQUALIZE, R.CONTRAST, R.AUTO_CONTRAST, R.SHEAR_Y))])
def test_aug_batch(layers, seed, flt, forced, want_u8):
    """gg_aug_batch: src exactly the packed bytes, dst exactly [B * 3 * S, S] f32, dst_u8 exactly [B * S, 3 S] bytes, the workspace exactly gg_aug_workspace_bytes(args)
    and holding the fill (NaN bytes / 0x47) before the call; the record table, offsets and sizes are host memory and are wiped right after the call returns."""
    from geoguessr_ai_amd.finetune_tinyvit.augment import RECORD_DTYPE
    S = 32
    srcs, recs0 = _batch(layers, seed)
    for l, op in enumerate(forced):
        recs0[0]["ops"][l]["op"] = op
    want = np.stack([R.apply_record(s, r, S, flt) for s, r in zip(srcs, recs0)])
    B = len(srcs)
    sizes = [3 * s.shape[0] * s.shape[1] for s in srcs]
    packed = torch.from_numpy(np.concatenate([s.reshape(-1) for s in srcs]))

    def call(G, L):
        recs = np.array(recs0, RECORD_DTYPE)
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        heights, widths = np.array([s.shape[0] for s in srcs], np.int32), np.array([s.shape[1] for s in srcs], np.int32)
        src = G.inp("src", packed)
        dst = G.out("dst", B * 3 * S, S, F32)
        a = L.AugArgs()
        a.src, a.src_bytes = src.ptr, packed.numel()
        a.offsets, a.heights, a.widths = offsets.ctypes.data, heights.ctypes.data, widths.ctypes.data
        a.B, a.S, a.filter = B, S, flt
        a.mean, a.std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        a.records = recs.ctypes.data
        need = L.lib().gg_aug_workspace_bytes(C.byref(a))
        assert need > 0
        ws = G.scratch("workspace", need, row_bytes=3 * S * 83)
        outs = {"dst": dst}
        if want_u8:
            outs["dst_u8"] = G.out("dst_u8", B * S, 3 * S, U8)
            a.dst_u8 = outs["dst_u8"].ptr
        a.dst, a.workspace, a.workspace_bytes = dst.ptr, ws.ptr, need
        L.check(L.lib().gg_aug_batch(C.byref(a), L.stream()), "gg_aug_batch")
        recs[...] = np.zeros((), RECORD_DTYPE)
        offsets[...] = -1
        heights[...] = 0
        widths[...] = 0

        def check(val):
            if want_u8:
                assert np.array_equal(val["dst_u8"].numpy().reshape(B, S, S, 3), want)
            assert np.array_equal(val["dst"].numpy().reshape(B, 3, S, S), R.normalise(want, MEAN, STD))
        return outs, check
    run_guarded(call)
