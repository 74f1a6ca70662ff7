"""The cases of tests/gemm16_cases.py that need a development switch (GG_* switches are honoured only under GG_DEV_SWITCHES, a gate the library reads once per
process), run by tests/test_gpu_gemm16_forms.py and tests/test_gemm16_cases_cpu.py in a fresh child process per group:

  tile256   under GG_DEV_SWITCHES=1 GG_GEMM_DMA_TILE=256: the forced cases on the LDS-DMA 256 x 256 kernel, gg_gemm_nt and gg_gemm_nt_f16, every epilogue of the case
  dma0      under GG_DEV_SWITCHES=1 GG_GEMM_DMA=0: the M = 1030 cases on the register-staged kernel.  The exact epilogues are held to the same exact reference (so
            to the LDS-DMA kernel's bits); the activation epilogues are also run with the switch taken away for one launch (GG_GEMM_DMA is read per launch) and
            must give the LDS-DMA form's bits
  routes    no GPU: prints, as one JSON line, what gg_gemm_nt_route reports for every (case, epilogue) of the table under the switches of this process

One `<case> <type> -> ok` line per case and type (or `-> FAIL` with the assertion); exit code 0 when all passed."""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tests import gemm16_cases as G
from tests import gemm16_run as R


def fake_args(case, epi, *, ldc_pad=G.PAD, res_off=0, ldr_pad=G.PAD, out_f32=0):
    """GgGemmArgs of a (case, epilogue) with made-up, 16-byte aligned addresses: enough for the route report, which dereferences nothing."""
    from geoguessr_ai_amd import _lib as L
    a = L.GemmArgs()
    P = 0x10000
    a.A, a.lda, a.B, a.ldb, a.C, a.ldc = P, case.K + G.PAD, P, case.K + G.PAD, P, case.N + ldc_pad
    a.M, a.N, a.K, a.split_k, a.out_f32 = case.M, case.N, case.K, 1, out_f32
    if epi == "linear":
        a.bias, a.rowscale, a.rows_per_scale, a.residual, a.ldr = P, P, G.ROWS_PER_SCALE, P + res_off, case.N + ldr_pad
    elif epi in ("gelu_pre", "quick_pre", "quick"):
        a.bias, a.act = P, G.ACT_CODE["gelu" if epi == "gelu_pre" else "quick"]
        a.preact = P if epi != "quick" else None
    elif epi in ("dgelu", "dquick"):
        a.dact_preact, a.dact = P, G.ACT_CODE["gelu" if epi == "dgelu" else "quick"]
    return a


def routes():
    print(json.dumps({f"{c.name}/{e}": R.route_of(fake_args(c, e)) for c in G.CASES for e in c.epis}))
    return 0


@contextlib.contextmanager
def without_env(name):
    old = os.environ.pop(name)
    try:
        yield
    finally:
        os.environ[name] = old


def run(mode):
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    cases = G.FORCED_256 if mode == "tile256" else G.M1030
    ok = True
    for c in cases:
        for dtype in (G.BF16, G.F16):
            tag = f"{c.name} {str(dtype)[6:]}"
            d = None
            try:
                d = R.DeviceCase(c, dtype)
                for epi in c.epis:
                    if mode == "tile256":
                        d.check(epi, c.route256)
                        continue
                    out, pre = d.check(epi, G.reg_route(c))
                    if epi not in G.EXACT_EPIS:
                        with without_env("GG_GEMM_DMA"):
                            o2, p2, route = d.launch(epi)
                        assert route[0] in (G.DMA192, G.DMA256), (tag, epi, route)
                        assert torch.equal(out.view(torch.int16), o2.view(torch.int16)), f"{tag} {epi}: the register-staged and the LDS-DMA kernel differ"
                        assert pre is None or torch.equal(pre.view(torch.int16), p2.view(torch.int16)), f"{tag} {epi}: the pre-activation copies differ"
                print(f"{tag} [{mode}] -> ok", flush=True)
            except AssertionError as e:                              # a wrong number; anything else (a device error) ends the run
                ok = False
                print(f"{tag} [{mode}] -> FAIL: {e}", flush=True)
            del d
    return 0 if ok else 1


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("tile256", "dma0", "routes"):
        sys.exit(__doc__)
    sys.exit(routes() if mode == "routes" else run(mode))
