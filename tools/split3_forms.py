"""The cases of tests/split3_cases.py that need a development switch (GG_* switches are honoured only under GG_DEV_SWITCHES, a gate the library reads once per
process), run by tests/test_gpu_split3_forms.py and tests/test_split3_cases_cpu.py in a fresh child process per group:

  run <VARIABLE> <value>   under GG_DEV_SWITCHES=1 <VARIABLE>=<value> (GG_SPLIT3A_TILE=256 / 128, GG_SPLIT3A_BN=96 / 128, GG_SPLIT3_NO_EC=1): the cases of that
                           group on the GPU, every family and epilogue of the case, held to the exact references of the unswitched run
  routes                   no GPU: prints, as one JSON line, what gg_gemm_nt_split3_route reports for every (case, epilogue) of the table under the switches of
                           this process

One `<case> -> ok` line per case (or `-> FAIL` with the assertion); exit code 0 when all passed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import split3_cases as S
from tests import split3_run as R


def fake_args(case, epi, *, bias_off=0, ldc_pad=S.PAD):
    """GgSplit3Args of a (case, epilogue) with made-up, 16-byte aligned addresses: enough for the route report, which dereferences nothing."""
    from geoguessr_ai_amd import _lib as L
    P0 = 0x10000
    P = {k: (P0, case.N + S.PAD) for k in ("residual", "second", "preact", "c_planes")}
    P["C"] = (P0, case.N + ldc_pad)
    P["B"], P["bias"], P["rowscale"] = (P0, case.K + S.PAD), (P0 + bias_off, 0), (P0, 0)
    a = R.fill_args(L.Split3Args(), case, epi, P)
    a.a_planes, a.lda = P0, case.K + S.PAD
    return a


def report(case, epi):
    return R.route_of(fake_args(case, epi), 0 if case.entry == "planes" else 1, 1 if case.entry == "pro" else 0, 1 if epi == "stats" else 0)


def routes():
    print(json.dumps({f"{c.name}/{e}": list(report(c, e)) for c in S.CASES for e in c.epis}))
    return 0


def run(group):
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    assert os.environ.get("GG_DEV_SWITCHES") and os.environ.get(group[0]) == group[1], f"run {group[0]} {group[1]} needs GG_DEV_SWITCHES=1 {group[0]}={group[1]}"
    ok = True
    for c in S.in_group(group):
        try:
            R.check_case(c, under_switch=True)
            print(f"{c.name} [{group[0]}={group[1]}] -> ok", flush=True)
        except AssertionError as e:                                  # a wrong number; anything else (a device error) ends the run
            ok = False
            print(f"{c.name} [{group[0]}={group[1]}] -> FAIL: {e}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "routes":
        sys.exit(routes())
    if mode == "run" and len(sys.argv) == 4 and (sys.argv[2], sys.argv[3]) in S.GROUPS:
        sys.exit(run((sys.argv[2], sys.argv[3])))
    sys.exit(__doc__)
