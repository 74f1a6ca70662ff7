"""Writes tests/golden/flash_bwd_parent.npz: dqkv of the NON-causal gg_attention_flash_bwd (dtype 0, 1 and 3; the cases of tests/clip_text_train_helpers.PARENT_CASES)
on the inputs tests/test_gpu_clip_text_train.py::test_noncausal_flash_backward_bits_unchanged regenerates from the same seeds.  Run it with GG_LIB pointing at a
libgg.so built from the commit BEFORE the causal template parameter was added to the backward kernels; the test then holds every later build to those bits.
    GG_LIB=/path/to/parent/libgg.so python tools/make_flash_bwd_parent_golden.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geoguessr_ai_amd import _lib as L          # noqa: E402
from tests.clip_text_train_helpers import PARENT_CASES, pack_parent, parent_case          # noqa: E402

L.TEXT_TRAIN_SIGNATURES.clear()          # (the parent build does not export the third header)
store = {}
for H, T, B in PARENT_CASES:
    b = {dtype: parent_case(L, H, T, B, dtype) for dtype in (0, 1, 3)}
    for k, v in pack_parent(b[0], b[1], b[3]).items():
        store[f"h{H}_t{T}_b{B}_{k}"] = v
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "flash_bwd_parent.npz")
os.makedirs(os.path.dirname(path), exist_ok=True)
np.savez_compressed(path, **store)
print("wrote", path, os.path.getsize(path), "bytes", {k: (v.shape, str(v.dtype)) for k, v in store.items()})
assert os.path.getsize(path) < (1 << 20)
