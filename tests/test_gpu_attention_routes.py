"""Every attention route computes, bit for bit, what it computed before the launchers were put behind one route decision (csrc/attention_route.h): SHA-256 digests
of out and lse and of dqkv (dbias is computed along, through a dbias_scratch, and not hashed: its first stage is LDS float atomics in no fixed order, so not
even two runs of one build agree on its last bits -- tests/attention_route_cases.py::route_bits has the figures; its order-fixed second stage is held bit for bit
there, as the fp64 sum of the scratch rows the route reports) of every case of
tests/attention_route_cases.py::DIGEST_CASES against tests/golden/attention_routes_parent.json, which tools/make_attention_routes_parent_golden.py wrote with the
build of the commit in front of that change.  Before each launch gg_attention_route must report the case's recorded kernels on the very arguments that are
launched.  (The two flash16 families have parent goldens of their own -- tests/golden/attention16_parent.npz, attention16_bwd_parent.npz -- and the flash16 window
backward's dbias, which is not order-fixed, stays under its tolerance test.)"""
import json
import os

import pytest

from tests import attention_route_cases as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "attention_routes_parent.json")) as f:
        return json.load(f)


def test_golden_file_holds_every_case(gold):
    assert sorted(gold) == sorted(r["name"] for r in R.DIGEST_CASES)


@pytest.mark.parametrize("name", [r["name"] for r in R.DIGEST_CASES])
def test_route_bits_unchanged_from_the_parent_build(L, gold, name):
    r = next(x for x in R.DIGEST_CASES if x["name"] == name)

    def check_route(r, bwd, a, entry, dtype):
        got, rt = R.reported(L, a, entry, dtype)
        assert got == r["kernels"][int(bwd)], (name, entry, got, r["kernels"][int(bwd)])
        return rt

    got = R.route_bits(L, r, check_route)
    want = gold[name]
    assert got["inputs"] == want["inputs"], f"{name}: the inputs differ from the golden file's (a changed generator, not a finding about a kernel)"
    assert sorted(got) == sorted(want) == sorted(("inputs", "out", "lse") + (("dqkv",) if r["bwd"] else ()))
    bad = [t for t in sorted(got) if t != "inputs" and got[t] != want[t]]
    assert not bad, (name, bad)
