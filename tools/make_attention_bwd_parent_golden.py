"""Writes tests/golden/attention_bwd_parent.json: SHA-256 digests of dq, dk, dv (and of the inputs) of gg_attention_flash_bwd on the seeded streaming-route calls of
tests/attention_cases.py::parent_bwd_bits, which test_streaming_backward_bits_unchanged_from_the_parent_build of tests/test_gpu_attention_conditioning.py
regenerates.  Run it with GG_LIB pointing at a libgg.so built from the commit BEFORE the two-pass backward kernels of csrc/attention_flash.hip lost their resident
template forms; the test then holds every later build to those bits.
    GG_LIB=/path/to/parent/libgg.so python tools/make_attention_bwd_parent_golden.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geoguessr_ai_amd import ops          # noqa: E402
from tests import attention_cases as A          # noqa: E402

store = A.parent_bwd_bits(ops)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attention_bwd_parent.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as f:
    json.dump(store, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", path, sorted(store))
