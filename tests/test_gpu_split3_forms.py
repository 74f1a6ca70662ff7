"""The split-bf16 GEMMs (csrc/gemm_split3.hip) on every tile form, k-loop form and plane product of their four kernels, bit for bit.

The cases, the exact operand families and the references are tests/split3_cases.py; the launch and the comparison are tests/split3_run.py.  Every NT test first asserts,
through gg_gemm_nt_split3_route on the arguments of the launch itself, that the shape reaches the kernel, tile width, epilogue class, tile grid and LDS size the case
records, then runs it through _lib: the exact epilogues (none, bias, "linear" = bias, row scale, residual, result planes, column statistics) must equal the exact
reference under torch.equal, with no NaN left inside an output and only NaN in its pad columns; the activation epilogues return the saved pre-activation bit for bit
and the activation inside the f32-site gate of tests/act_cases.py.  An af32 result must also equal, bit for bit, the plane-fed kernel's on the restatement's planes.
No tolerance is defined here.

What the operand families add to an integer family: their significands are 19 (or 10 and 9) bits wide, so the second and third bf16 planes are non-zero and each of
the six plane products a1 b1 ... a3 b1 carries part of every result; one lost product on one fragment is a wrong element, not 1e-7 of a norm.

The cases that need a development switch run in a child process per group (tools/split3_forms.py): each af32 kernel at the contraction lengths the dispatch gives
the other one (GG_SPLIT3A_TILE), at the other tile width (GG_SPLIT3A_BN), and with the generic epilogue in place of the compile-time classes (GG_SPLIT3_NO_EC).
"""
import os
import subprocess
import sys

import pytest

from tests import split3_cases as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def R():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    from tests import split3_run
    return split3_run


@pytest.mark.parametrize("case", S.UNSWITCHED, ids=lambda c: c.name)
def test_split3_form(R, case):
    """Every case that runs under the dispatch's own rules: each family and each epilogue of the case."""
    R.check_case(case)


@pytest.mark.parametrize("group", S.GROUPS, ids=lambda g: "=".join(g))
def test_switched_group(group):
    """One fresh child process per switch group, GG_DEV_SWITCHES=1 plus the switch: one `-> ok` line per case."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("GG_") or k == "GG_LIB"}
    env.update({"GG_DEV_SWITCHES": "1", group[0]: group[1]})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "split3_forms.py"), "run", group[0], group[1]], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, (r.stdout[-4000:], r.stderr[-3000:])
    assert r.stdout.count("-> ok") == len(S.in_group(group)), (r.stdout[-4000:], r.stderr[-3000:])


@pytest.mark.parametrize("name", [c.name for c in S.TN_CASES])
def test_tn_split3_exact(R, name):
    """gg_gemm_tn_split3 with the split count of the case: every slab and the gg_splitk_reduce result bit for bit; rows behind M - 1 and row scales behind the last
    sample hold NaN, the scratch behind the last slab keeps its NaN."""
    R.check_tn(name)


def test_split3_bf16_edges(R):
    """gg_split3_bf16 against the restated split on the three families, +-0, denormals, the clamp range up to FLT_MAX, +-inf and NaN (ldx > cols), plane by plane."""
    R.check_split_edges()
