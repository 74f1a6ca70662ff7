"""Writes tests/golden/attention16_parent.npz: the bits of out (int16 view) and lse of gg_attention_flash16_fwd and gg_attention_flash16_win_fwd on the seeded calls
of tests/attention16_cases.py::parent_bits, which test_bits_unchanged_from_the_parent_build of tests/test_gpu_attention16.py and tests/test_gpu_attention16_win.py
regenerate.  Run it with GG_LIB pointing at a libgg.so built from the commit BEFORE csrc/attention_flash16.hip and csrc/attention_flash16_win.hip became one
kernel; the tests then hold every later build to those bits.
    GG_LIB=/path/to/parent/libgg.so python tools/make_attention16_parent_golden.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geoguessr_ai_amd import ops          # noqa: E402
from tests import attention16_cases as A          # noqa: E402

store = {**A.parent_bits(ops, window=False), **A.parent_bits(ops, window=True)}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attention16_parent.npz")
os.makedirs(os.path.dirname(path), exist_ok=True)
np.savez_compressed(path, **store)
print("wrote", path, {k: v.shape for k, v in store.items()})
