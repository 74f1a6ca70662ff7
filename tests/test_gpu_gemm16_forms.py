"""gg_gemm_nt and gg_gemm_nt_f16 (csrc/gemm.hip in both builds) on every tile walk and k-loop form of the register-staged and the LDS-DMA kernels, bit for bit.

The cases, the exact operand family and the references are tests/gemm16_cases.py; the launch and the comparison are tests/gemm16_run.py.  Every test first asserts, through
gg_gemm_nt_route on the arguments of the launch itself, that the shape reaches the kernel, tile grid and tile walk the case records, then runs it: the plain and the linear
epilogue (bias, row scale, residual) must equal the exact reference under torch.equal, the pad columns of C must keep their NaN, and a second call must give the same bits;
the activation epilogues return the pre-activation copy bit for bit and the activation inside the per-element gate of tests/act_cases.py.  No tolerance is defined here.

What only a K tail can show: a 16-byte chunk beyond K is zero-filled by pushing its buffer offset out of range.  Rows beyond M or N use the same mechanism, but their results
are dropped by the store's range check; a chunk beyond K enters a product that is kept, and the columns behind K hold NaN here.

The cases that need a development switch run in a child process per group (tools/gemm16_forms.py): the 256 x 256 geometry forced by GG_GEMM_DMA_TILE=256, and the M = 1030
cases on the register-staged kernel under GG_GEMM_DMA=0, which must give the LDS-DMA kernel's bits.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import gemm16_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def R():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    from tests import gemm16_run
    return gemm16_run


@pytest.mark.parametrize("dtype", [G.BF16, G.F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_gemm16_form(R, case, dtype):
    """Every case of the table under the dispatch's own rules (the forced cases take the 192 x 128 form here and the 256 x 256 form in test_forced_256_geometry)."""
    d = R.DeviceCase(case, dtype)
    for epi in case.epis:
        d.check(epi, G.natural_route(case, epi))


def _child(mode, cases, **switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GG_") or k == "GG_LIB"}
    env.update(GG_DEV_SWITCHES="1", **switches)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gemm16_forms.py"), mode], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, (r.stdout[-4000:], r.stderr[-3000:])
    assert r.stdout.count("-> ok") == 2 * len(cases), (r.stdout[-4000:], r.stderr[-3000:])


def test_forced_256_geometry():
    """GG_GEMM_DMA_TILE=256: (1030, 512, K) for K = 192 ... 4096 (5 x 2 tiles, the last M tile 6 rows) and (1290, 1280, 256) (groups of 4 M-tiles, a last group of 2) on
    gemm_nt_dma_kernel<., ., 8, 4>, both types; at K = 200 with GELU / QuickGELU + pre-activation copy, QuickGELU and x GELU' / x QuickGELU' of a second tensor."""
    _child("tile256", G.FORCED_256, GG_GEMM_DMA_TILE="256")


def test_register_staged_kernel_gives_the_same_bits():
    """GG_GEMM_DMA=0: the M = 1030 cases on gemm_nt_kernel<128, 128>, held to the same exact references; their activation epilogues bit-compared with the LDS-DMA form."""
    _child("dma0", G.M1030, GG_GEMM_DMA="0")


@pytest.mark.parametrize("M,N,K", G.TN_SHAPES)
def test_gemm_tn_exact(R, M, N, K):
    """ops.gemm_tn (gg_gemm_tn + gg_splitk_reduce) on the exact family: f32 output, so bit for bit whatever the row split."""
    from geoguessr_ai_amd import ops, _lib
    splits = _lib.lib().gg_gemm_tn_splits(M, N, K)
    assert splits > 1 and M % (-(-(-(-M // splits)) // 64) * 64) != 0          # several splits of whole 64-row steps, the last one ragged
    dY, X, want = G.tn_case(M, N, K)
    got = ops.gemm_tn(dY.to(G.BF16).cuda(), X.to(G.BF16).cuda())
    torch.cuda.synchronize()
    bad = ~(got.cpu() == want)
    assert not bool(bad.any()), f"gemm_tn {M}x{N}x{K}: {int(bad.sum())} of {bad.numel()} elements differ, first at {tuple(int(i) for i in bad.nonzero()[0])}"
