"""Writes tests/golden/flash_fwd_parent.npz: out / lse of the NON-causal gg_attention_flash_fwd (dtype 3 and dtype 0; 2 sequences x 2 heads of 50 and of 65 tokens) on the
inputs tests/test_gpu_clip_text.py::test_noncausal_flash_forward_bits_unchanged regenerates from the same seeds.  Run it with GG_LIB pointing at a libgg.so built
from the commit BEFORE the causal template parameter was added to the forward kernels; the test then holds every later build to those bits.
    GG_LIB=/path/to/parent/libgg.so python tools/make_flash_parent_golden.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geoguessr_ai_amd import _lib as L          # noqa: E402
from tests.clip_text_helpers import causal, make_qkv          # noqa: E402

L.TEXT_SIGNATURES.clear()          # (the parent build does not export the second header)
store = {}
for T in (50, 65):
    for dtype in (3, 0):
        buf, _, _, _ = make_qkv(2, T, 2, dtype, 500 + T)
        rc, out, lse = causal(L, buf, 2, T, 2, dtype, buf.shape[1], fn="gg_attention_flash_fwd")
        assert rc == 0, L.lib().gg_last_error()
        store[f"out_{T}_{dtype}"] = out.float().cpu().numpy()
        store[f"lse_{T}_{dtype}"] = lse.cpu().numpy()
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "flash_fwd_parent.npz")
os.makedirs(os.path.dirname(path), exist_ok=True)
np.savez_compressed(path, **store)
print("wrote", path, {k: v.shape for k, v in store.items()})
