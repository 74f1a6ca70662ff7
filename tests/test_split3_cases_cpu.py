"""CPU checks of tests/split3_cases.py and of gg_gemm_nt_split3_route (host arithmetic: no GPU): the operand families satisfy their exactness conditions on the whole
table, the route report answers the recorded route of every case with and without the development switches, and the table holds every class of tile form, k-loop form,
plane product and epilogue of the four split-bf16 GEMM kernels."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import split3_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "split3_forms.py")


@pytest.fixture(scope="module")
def T():
    """tools/split3_forms.py as a module (fake_args, report), with the library built."""
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    spec = importlib.util.spec_from_file_location("split3_forms_tool", TOOL)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_split_restatement():
    """The restated split on values whose planes are known: 24 significand bits fill three planes, integers one, the clamp keeps the first plane finite."""
    a, b, c = S.split3(torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -23, 3.0, -0.0, 3.4e38, float("inf")]))
    assert a[:2].tolist() == [1.0 + 2.0 ** -7, 3.0] and b[:2].tolist() == [2.0 ** -15, 0.0] and c[:2].tolist() == [2.0 ** -23, 0.0]
    assert (a[2].item(), b[2].item(), c[2].item()) == (0.0, 0.0, 0.0) and torch.signbit(a[2])
    assert a[3].item() == S.BF16_MAX and torch.isfinite(b[3]) and float(a[3].double() + b[3].double() + c[3].double()) == float(torch.tensor(3.4e38))
    assert a[4].item() == S.BF16_MAX and b[4].item() == float("inf") and torch.isnan(c[4])
    n = S.split3(torch.tensor([float("nan")]))
    assert n[0].item() == -S.BF16_MAX and torch.isnan(n[1]) and torch.isnan(n[2])          # (the clamp passes over a NaN: it sits in planes 2 and 3)
    e = S.split_edge_values()
    assert e.shape[1] % 4 == 0 and bool(torch.isnan(e).any()) and bool(torch.isinf(e).any()) and bool(((e != 0) & (e.abs() < 2.0 ** -126)).any())


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_family_is_exact(case):
    """Conditions 1-5 of the module (asserted inside expected()) on every (case, family), and the operand families are what the module states."""
    for fam in case.fams:
        o, e = S.operands(case.name, fam), S.expected(case.name, fam)
        print(f"\n[{case.name}/{fam}] sum |planes| = 2^{e['span_log2']:.2f} granules, k-form {S.kform(case.K)}")
        assert e["span_log2"] < 23
        wide = o["B"] if fam == "s1w3" else o["A"]
        if fam in ("w3s1", "s1w3"):
            m = wide.abs() * 2.0 ** 18
            assert bool((m == m.round()).all()) and float(m.min()) >= 2 ** 18 and float(m.max()) < 2 ** 19
        elif fam == "w2w2":
            m, j = o["A"].abs() * 256, o["B"].abs() * 256
            assert bool((m == m.round()).all()) and float(m.max()) < 2 ** 10 and bool((j == j.round()).all()) and float(j.max()) < 2 ** 9
        else:
            assert set(o["A"].unique().tolist()) == {-1.0, 0.0, 1.0}
        assert float(o["bias"].abs().max()) <= 8 and float(o["residual"].abs().max()) <= 8 and set(o["rowscale"].unique().tolist()) <= {0.0, 1.0, 2.0}
        assert o["rowscale"].numel() == -(-case.M // S.ROWS_PER_SCALE) and all(t % S.ROWS_PER_SCALE for t in (32, 64, 128, 256))
        buf = S.padded_planes(S.split3(o["B"]))
        assert buf.stride(1) == case.K + S.PAD and bool(torch.isnan(buf[:, :, case.K:]).all())
        assert case.M <= 1030 and case.N <= 1224 and case.K <= 1544 and case.K % 8 == 0


@pytest.mark.parametrize("name", [c.name for c in S.TN_CASES])
def test_tn_family_is_exact(name):
    c = S.TN_BY_NAME[name]
    slabs, total = S.tn_expected(name)
    assert slabs.shape == (c.splits, c.N, c.K) and torch.equal(slabs.double().sum(0), total.double())


def test_comparison_names_the_element():
    want = torch.zeros(300, 200)
    got = want.clone()
    S.assert_bits(got, want, "clean")
    got[260, 130] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 60000 elements differ \(1 NaN\); first at \(260, 130\), tile \(1, 1\) local \(4, 2\)"):
        S.assert_bits(got, want, "x", granule=1.0, tile=(256, 128))
    got = want.clone()
    got[0, 1] = 2.0 ** -18
    with pytest.raises(AssertionError, match=r"\|error\| 1 \.\. 1 granules"):
        S.assert_bits(got, want, "x", granule=2.0 ** -18)
    p = S.split3(torch.tensor([1.5, float("nan")]))
    S.assert_planes_equal(p, [q.clone() for q in p], "nan by class")
    with pytest.raises(AssertionError, match="plane 1"):
        S.assert_planes_equal(p, S.split3(torch.tensor([1.0, float("nan")])), "x")


def test_route_report_matches_the_table(T):
    """Without switches every case answers its natural route; the natural kernel and width recorded in the table are those of the restated dispatch rule."""
    for c in S.CASES:
        if c.entry == "af32":
            assert S.natural_af32(c.N, c.K) == c.natural, c.name
        elif c.entry == "planes":
            assert c.natural == ((S.PL256 if c.M > 128 else S.PL128), 128), c.name
        else:
            assert c.natural == (S.A256, S.natural_af32(c.N, c.K)[1]) and 384 <= c.K <= 1024, c.name
        for e in c.epis:
            assert T.report(c, e) == S.route_for(c, e), (c.name, e)


def _child_routes(**switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GG_") or k == "GG_LIB"}
    env.update(switches)
    r = subprocess.run([sys.executable, TOOL, "routes"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return {k: S.Route(*v) for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}


def _under(case, group):
    """(kernel, width) of a case under a switch group, by the restated rule."""
    k, w = case.natural
    if case.entry == "planes":
        return k, w
    if group[0] == "GG_SPLIT3A_TILE" and case.entry != "pro":
        k = S.A256 if group[1] == "256" else S.A128
    if group[0] == "GG_SPLIT3A_BN":
        w = int(group[1])
    return k, w


@pytest.mark.parametrize("group", S.GROUPS, ids=lambda g: "=".join(g))
def test_route_report_under_the_switches(T, group):
    """The gate GG_DEV_SWITCHES is read once per process, so each switch group gets a child: the cases of the group answer their recorded route, every other case the
    route the restated rule gives it.  Without the gate the switch changes nothing."""
    got = _child_routes(GG_DEV_SWITCHES="1", **{group[0]: group[1]})
    for c in S.CASES:
        for e in c.epis:
            want = S.run_route(c, e) if c.group == group else S.route_for(c, e, _under(c, group), no_ec=group == S.G_NOEC)
            assert got[f"{c.name}/{e}"] == want, (c.name, e)
        if c.group == group:
            assert _under(c, group) == c.switched, c.name
    got = _child_routes(**{group[0]: group[1]})
    for c in S.CASES:
        for e in c.epis:
            assert got[f"{c.name}/{e}"] == S.route_for(c, e), (c.name, e)


def test_route_report_edges(T):
    """What the launches refuse the report refuses; the vector-path conditions of the epilogue classes; the prologue's K range."""
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    r = L.Split3Route()
    c = S.BY_NAME["a128_130x200x40"]
    assert T.report(c, "bias").epilogue == 1 and T.report(c, "linear").epilogue == 4
    a = T.fake_args(c, "bias", bias_off=4)                                   # a bias that is not 16-byte aligned: the generic epilogue
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 1, 0, 0, C.byref(r)) == 0 and r.epilogue == 0
    a = T.fake_args(c, "bias", ldc_pad=6)                                    # ldc % 4 != 0
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 1, 0, 0, C.byref(r)) == 0 and r.epilogue == 0
    a = T.fake_args(c, "bias")
    a.K = 44
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 1, 0, 0, C.byref(r)) == -1 and b"K %" in lib.gg_last_error()
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 0, 0, 0, C.byref(r)) == -1 and b"multiples of 8" in lib.gg_last_error()
    a = T.fake_args(c, "bias")
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 1, 1, 0, C.byref(r)) == -1 and b"384" in lib.gg_last_error()          # the prologue needs 384 <= K <= 1024
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 0, 1, 0, C.byref(r)) == -1 and lib.gg_gemm_nt_split3_route(C.byref(a), 0, 0, 1, C.byref(r)) == -1
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 1, 0, 1, C.byref(r)) == -1 and b"colstats needs the plain epilogue" in lib.gg_last_error()
    assert lib.gg_gemm_nt_split3_route(C.byref(a), 1, 0, 0, None) == -1
    # the form edges: K = 376 / 384, M = 128 / 129 on the plane-fed entry, the fifth of the columns (N = 192 / 200)
    def mk(entry, M, N, K):
        return S._case("edge", entry, M, N, K, None)
    assert T.report(mk("af32", 300, 200, 376), "bias")[:2] == (S.A128, 128) and T.report(mk("af32", 300, 200, 384), "bias")[:2] == (S.A256, 128)
    assert T.report(mk("af32", 300, 192, 384), "bias")[:2] == (S.A256, 96) and T.report(mk("af32", 300, 576, 384), "bias")[:2] == (S.A256, 128)
    assert T.report(mk("planes", 128, 200, 64), "plain")[:2] == (S.PL128, 128) and T.report(mk("planes", 129, 200, 64), "plain")[:2] == (S.PL256, 128)
    assert T.report(mk("pro", 300, 200, 1024), "plain").lds_bytes == 2 * 3 * 384 * 64 + 2 * (1024 + 96) * 4


REQUIRED = (
    # plane-fed two-stage ring: nk 1, 2, odd >= 3, even >= 4; every tail
    [f"pl256:nk={n}" for n in (1, 2, 3, "odd", "even")] + [f"pl256:tail={t}" for t in range(4)] +
    # plane-fed three-stage ring: nk 1, 2, 3, >= 7; every tail
    [f"pl128:nk={n}" for n in (1, 2, 3)] + ["pl128:nk>=7"] + [f"pl128:tail={t}" for t in range(4)] +
    # af32 256-row: both widths, nk odd and even at K >= 384, K = 384 ... 416, 1544; under the switch nk 1, 2, 3
    ["a256:w128", "a256:w96", "a256:nk=odd", "a256:nk=even"] + [f"a256:K={k}" for k in (384, 392, 408, 416, 1544)] + [f"a256:nk={n}/switched" for n in (1, 2, 3)] +
    [f"a256:K={k}/switched" for k in (8, 40, 72)] +
    # af32 128-row: both widths, K = 8 ... 376, K = 1544 under the switch
    ["a128:w128", "a128:w96"] + [f"a128:K={k}" for k in (8, 40, 96, 200, 376)] + ["a128:K=1544/switched"] +
    # the other width, forced, on each af32 kernel
    [f"{k}:w{w}/forced" for k in ("a256", "a128") for w in (96, 128)] +
    # raggedness and tile counts
    ["pl256:last_m<64", "a256:last_m<64", "a128:last_m<64", "a128:last_m<64/single", "pl128:last_m<64/single", "last_n=72", "last_n=8", "last_n=2",
     "tiles<8", "tiles%8==0", "tiles>8,rem"] +
    # epilogues: class 1, class 4, the generic epilogue by c_planes, by N % 8 != 0 and by GG_SPLIT3_NO_EC; colstats; the prologue; the activation classes per kernel
    [f"{k}:{e}" for k in ("a256", "a128") for e in ("bias/class1", "linear/class4", "planes/class0", "bias/class0/n%8", "bias/class0/noec", "linear/class0/noec",
                                                     "stats/class0", "int", "gelu_pre/class2", "dgelu/class3", "quick_pre/class5", "dquick/class6")] +
    ["a256:pro/plain", "a256:K=1024", "pl256:planes/planes", "pl128:planes/planes"] + [f"pl256:planes/{e}" for e in S.ACT_EPIS] +
    # every family on every kernel
    [f"{k}:{f}" for k in ("pl256", "pl128", "a256", "a128") for f in S.FAMS])


def test_table_covers_every_form():
    """An edit of the table that loses a class fails here by name."""
    missing = sorted(set(REQUIRED) - S.coverage())
    assert not missing, f"the table runs no case of {missing}"
    assert {c.K for c in S.CASES if c.entry == "pro"} >= {384, 416, 1024} and {c.natural[1] for c in S.CASES if c.entry == "pro"} == {96, 128}
    assert all(S.in_group(g) for g in S.GROUPS)


def test_tn_table_covers_every_form():
    """Stages per slab 1, 2, odd >= 3, even >= 4; a last slab shorter than the others whose last stage has fewer than 32 rows; N = 260, K = 132; a grid that is no
    multiple of 8; with and without the row scale; every family."""
    geo = {c.name: S.tn_geometry(c.M, c.N, c.K, c.splits) for c in S.TN_CASES}
    st = {g.stages for g in geo.values()}
    assert {1, 2} <= st and any(s >= 3 and s % 2 for s in st) and any(s >= 4 and s % 2 == 0 for s in st)
    assert any(c.splits > 1 and g.last_rows < g.rows_per_split and g.last_rows % 32 for c, g in ((c, geo[c.name]) for c in S.TN_CASES))
    assert any(g.last_stages >= 2 and g.last_rows % 32 for g in geo.values())
    assert any(c.N == 260 and c.K == 132 for c in S.TN_CASES) and any(g.grid % 8 for g in geo.values()) and any(g.grid % 8 == 0 for g in geo.values())
    assert {c.scaled for c in S.TN_CASES} == {True, False} and {c.fam for c in S.TN_CASES} == set(S.FAMS)
    assert S.tn_geometry(4099, 384, 384, 5) == (2, 3, 832, 26, 771, 25, 30)
    with pytest.raises(AssertionError):
        S.tn_geometry(64, 8, 8, 3)
