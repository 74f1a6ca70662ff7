"""CPU checks of tests/gemm16_cases.py and of gg_gemm_nt_route (host arithmetic: no GPU): the operand family is exact on the whole table, the route report answers the
recorded route of every case with and without the development switches, the edges of the routing rules sit where gemm.hip's comments put them, and the table holds
every class of k-loop form and tile walk of both LDS-DMA geometries."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import gemm16_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "gemm16_forms.py")


@pytest.fixture(scope="module")
def T():
    """tools/gemm16_forms.py as a module (fake_args), with the library built."""
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    spec = importlib.util.spec_from_file_location("gemm16_forms_tool", TOOL)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def route(a):
    from tests import gemm16_run as R
    return R.route_of(a)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_family_is_exact(case):
    """f32 product == f64 product, every expected value an integer <= 256 exact in bf16 and fp16, both roundings of the linear epilogue included (asserted inside
    expected()); the operand family is what the module states; NaN pads."""
    o, e = G.operands(case.name), G.expected(case.name)
    assert set(o["A"].unique().tolist()) == {-1.0, 0.0, 1.0} and 0.45 < float((o["A"] != 0).float().mean()) < 0.55
    assert set(o["B"].unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert float(o["bias"].abs().max()) <= 8 and float(o["residual"].abs().max()) <= 8 and set(o["rowscale"].unique().tolist()) <= {0.0, 1.0, 2.0}
    assert o["rowscale"].numel() == -(-case.M // G.ROWS_PER_SCALE) and all(t % G.ROWS_PER_SCALE for t in (16, 96, 128, 192, 256))
    print(f"\n[{case.name}] max |A B^T| {float(e['z'].abs().max()):.0f}, max |linear| {float(e['linear'].abs().max()):.0f}, k-form {case.kform}")
    assert float(e["z"].abs().max()) <= G.MAX_EXACT and float(e["linear"].abs().max()) <= G.MAX_EXACT
    if o["second"] is not None:
        assert torch.equal(o["second"].to(G.BF16).float(), o["second"]) and torch.equal(o["second"].to(G.F16).float(), o["second"])
    buf = G.padded(o["B"], G.BF16)
    assert buf.stride(0) == case.K + G.PAD and bool(torch.isnan(buf[:, case.K:]).all()) and torch.equal(buf[:, :case.K].float(), o["B"])
    assert bool(torch.isnan(G.nan_out(4, case.N, G.F16)).all())


def test_comparison_names_the_tile():
    want = torch.zeros(300, 200)
    got = want.clone().to(G.BF16)
    G.assert_bits(got, want, G.DMA192, "clean")
    got[197, 130] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 60000 elements differ \(1 NaN\); first at element \(197, 130\): tile \(tm 1, tn 1\), wave row 0, wave column 0, .*\(NaN\)"):
        G.assert_bits(got, want, G.DMA192, "x")
    got = want.clone().to(G.BF16)
    got[299, 199] = 1.0
    with pytest.raises(AssertionError, match=r"tile \(tm 1, tn 0\), wave row 0, wave column 3, tile-local \(43, 199\): got 1.0, exact 0.0"):
        G.assert_bits(got, want, G.DMA256, "x")


def test_kform_classes():
    assert G.kform(192) == (3, 0, 3, 0) and G.kform(200) == (4, 1, 2, 1) and G.kform(224) == (4, 1, 2, 4) and G.kform(232) == (4, 1, 2, 5)
    assert G.kform(248) == (4, 1, 2, 7) and G.kform(320) == (5, 1, 3, 0) and G.kform(384) == (6, 2, 2, 0) and G.kform(448) == (7, 2, 3, 0)
    assert G.kform(456) == (8, 3, 2, 1) and G.kform(4096) == (64, 31, 2, 0) and G.kform(264) == (5, 1, 3, 1)


def test_route_report_matches_the_table(T):
    for c in G.CASES:
        for e in c.epis:
            assert route(T.fake_args(c, e)) == G.natural_route(c, e), (c.name, e)


def _child_routes(**switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GG_") or k == "GG_LIB"}
    env.update(switches)
    r = subprocess.run([sys.executable, TOOL, "routes"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return {k: tuple(v) for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}


def test_route_report_under_the_switches(T):
    """The gate GG_DEV_SWITCHES is read once per process, so each group of switches gets a child.  GG_GEMM_DMA_TILE=256: the forced cases answer their recorded route,
    every other case that takes the LDS-DMA form answers the 256 x 256 grid of its shape, the register-staged cases do not move.  GG_GEMM_DMA=0: everything is
    register-staged.  Without the gate the switches change nothing."""
    got = _child_routes(GG_DEV_SWITCHES="1", GG_GEMM_DMA_TILE="256")
    for c in G.CASES:
        for e in c.epis:
            nat = G.natural_route(c, e)
            want = c.route256 if c.route256 else (nat if nat[0] in (G.R128, G.R64) else (G.DMA256,) + G.grid_of(G.DMA256, c.M, c.N))
            assert got[f"{c.name}/{e}"] == want, (c.name, e)
    got = _child_routes(GG_DEV_SWITCHES="1", GG_GEMM_DMA="0")
    for c in G.CASES:
        for e in c.epis:
            assert got[f"{c.name}/{e}"] == G.reg_route(c), (c.name, e)
    got = _child_routes(GG_GEMM_DMA_TILE="256", GG_GEMM_DMA="0")
    for c in G.CASES:
        for e in c.epis:
            assert got[f"{c.name}/{e}"] == G.natural_route(c, e), (c.name, e)


def test_routing_rule_edges(T):
    """Each rule of the dispatch on either side of its edge, without running a kernel."""
    def mk(M, N, K):
        return G._case("edge", M, N, K, None)
    # K >= 4096 takes 256 x 256 tiles from 512 tiles on: 511 x 1 against 512 x 1 tiles of 256 rows
    assert route(T.fake_args(mk(511 * 256, 256, 4096), "plain")) == (G.DMA192, 682, 2, 0)
    assert route(T.fake_args(mk(511 * 256 + 1, 256, 4096), "plain")) == (G.DMA256, 512, 1, 0)
    assert route(T.fake_args(mk(511 * 256 + 1, 256, 4088), "plain"))[0] == G.DMA192
    assert route(T.fake_args(mk(22016, 1536, 192), "gelu_pre"))[0] == G.DMA256 and route(T.fake_args(mk(22016, 1528, 192), "gelu_pre"))[0] == G.DMA192
    # a last N tile of at most 64 columns takes the 128 x 64 register-staged tile
    assert route(T.fake_args(mk(1030, 192, 192), "plain")) == (G.R64, 9, 3, 0)
    assert route(T.fake_args(mk(1030, 200, 192), "plain")) == (G.DMA192, 6, 2, 0)
    # M >= 1024, K >= 192
    assert route(T.fake_args(mk(1023, 200, 192), "plain")) == (G.R128, 8, 2, 0) and route(T.fake_args(mk(1024, 200, 192), "plain")) == (G.DMA192, 6, 2, 0)
    assert route(T.fake_args(mk(1030, 200, 184), "linear")) == (G.R128, 9, 2, 0) and route(T.fake_args(mk(1030, 200, 192), "linear")) == (G.DMA192, 6, 2, 0)
    # the LDS-DMA epilogue has no general-shape fallbacks: a misaligned residual, a residual or output pitch that is no multiple of 8, an f32 output
    c = mk(1030, 200, 192)
    assert route(T.fake_args(c, "linear", res_off=8))[0] == G.R128 and route(T.fake_args(c, "linear", ldr_pad=4))[0] == G.R128
    assert route(T.fake_args(c, "plain", ldc_pad=4))[0] == G.R128 and route(T.fake_args(c, "plain", out_f32=1))[0] == G.R128
    # what the launch refuses, the report refuses
    from geoguessr_ai_amd import _lib as L
    a = T.fake_args(mk(1030, 200, 196), "plain")
    assert L.lib().gg_gemm_nt_route(C.byref(a), None, None, None) == -1 and b"multiples of 8" in L.lib().gg_last_error()
    a = T.fake_args(c, "plain")
    assert L.lib().gg_gemm_nt_route(C.byref(a), None, None, None) == G.DMA192                   # (out-parameters are optional)


def test_table_covers_every_form():
    """Per LDS-DMA geometry: no steady pair, one, at least two; a tail of 2 and of 3 stages; 0, 1-4 and 5-7 chunks in the K tail; the row-major walk and the
    group_m walk with a partial last group.  An edit of the table that loses a class fails here by name."""
    for kernel, under_switch in ((G.DMA192, False), (G.DMA256, True)):
        missing = G.REQUIRED_COVERAGE - G.coverage(kernel, under_switch)
        assert not missing, f"{G.ROUTE_NAME[kernel]}: the table runs no case of {sorted(missing)}"
    assert "group_m:partial" in G.coverage(G.DMA256, False)                  # the natural 256 x 256 case: 86 M-tiles in groups of 4
    assert any(G.natural_route(c, e)[0] == G.R64 for c in G.CASES for e in c.epis) and any(c.route[0] == G.R128 for c in G.CASES)
    for c in G.CASES:                                                        # the recorded grids are those of the recorded kernels
        for r in [c.route, c.route256] + list(c.route_by_epi.values()):
            assert r is None or r[1:] == G.grid_of(r[0], c.M, c.N), (c.name, r)
    assert {c.kform.tail_chunks for c in G.CASES if c.route[0] == G.DMA192} >= {0, 1, 4, 5, 7}
