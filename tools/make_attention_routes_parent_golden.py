"""Writes tests/golden/attention_routes_parent.json: SHA-256 digests of out and lse (forwards) and dqkv (backwards; dbias is requested and not hashed -- LDS float atomics
in no fixed order) of every case of tests/attention_route_cases.py::DIGEST_CASES (tests/attention_cases.py::ROUTES at the table's own shapes, class `plain`, fixed seed;
7 x 7 windows with 65 windows; the window_map form with 3 of 8 windows live), with the inputs' digests next to them.  test_route_bits_unchanged_from_the_parent_build
of tests/test_gpu_attention_routes.py regenerates them.  Run it with GG_LIB pointing at a libgg.so built from the commit BEFORE the attention launchers were put
behind one route decision; the test then holds every later build to those bits.
    GG_LIB=/path/to/parent/libgg.so python tools/make_attention_routes_parent_golden.py [out.json]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geoguessr_ai_amd import _lib as L          # noqa: E402
from tests import attention_route_cases as R          # noqa: E402

if not hasattr(C.CDLL(L.LIB_PATH), "gg_attention_route"):
    L.ATTN_ROUTE_SIGNATURES.clear()          # (the build in front of the route struct has no report to bind; nothing here asks it)
L.require_gpu()
store = {r["name"]: R.route_bits(L, r) for r in R.DIGEST_CASES}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attention_routes_parent.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as f:
    json.dump(store, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", path, len(store))
