"""Device side of tests/split3_cases.py: builds the GgSplit3Args of one (case, family, epilogue), asks gg_gemm_nt_split3_route for its route, launches
gg_gemm_nt_split3_ex / _af32 / _af32_stats / _af32_pro through _lib and compares with the exact reference; the TN weight gradient and gg_split3_bf16 likewise.  Shared by
tests/test_gpu_split3_forms.py (no switches) and tools/split3_forms.py (a child process per switch group)."""
import ctypes as C

import torch

from tests import split3_cases as S


def _L():
    from geoguessr_ai_amd import _lib
    return _lib


def route_of(args, af32, pro=0, with_colstats=0):
    """The GgSplit3Route the library reports for exactly these arguments, as a tests.split3_cases.Route."""
    L = _L()
    r = L.Split3Route()
    if L.lib().gg_gemm_nt_split3_route(C.byref(args), af32, pro, with_colstats, C.byref(r)) != 0:
        raise L.GgError(f"gg_gemm_nt_split3_route refused the arguments: {L.lib().gg_last_error().decode(errors='replace')}")
    return S.Route(r.kernel, r.tile_n, r.epilogue, r.mapped, r.tilesM, r.tilesN, r.lds_bytes)


def fill_args(a, case, epi, P):
    """The epilogue fields of a GgSplit3Args; P maps a buffer's name to (address, row pitch)."""
    a.M, a.N, a.K = case.M, case.N, case.K
    a.b_planes, a.ldb = P["B"]
    a.C, a.ldc = P["C"]
    if epi in ("bias", "linear", "gelu_pre", "quick_pre", "planes"):
        a.bias = P["bias"][0]
    if epi == "linear":
        a.rowscale, a.rows_per_scale = P["rowscale"][0], S.ROWS_PER_SCALE
        a.residual, a.ldr = P["residual"]
    elif epi in ("gelu_pre", "quick_pre"):
        a.act, a.preact = S.ACT_CODE["gelu" if epi == "gelu_pre" else "quick"], P["preact"][0]
    elif epi in ("dgelu", "dquick"):
        a.dact_preact, a.dact = P["second"][0], S.ACT_CODE["gelu" if epi == "dgelu" else "quick"]
    elif epi == "planes":
        a.c_planes, a.ldp = P["c_planes"]
    else:
        assert epi in ("plain", "bias", "stats"), epi
    return a


class DeviceCase:
    """The operands of one (case, family) on the device (NaN-padded buffers) and its exact results."""

    def __init__(self, case, fam):
        self.case, self.fam = case, fam
        o, self.want = S.operands(case.name, fam), S.expected(case.name, fam)
        fed = o["A_fed"] if case.entry == "pro" else o["A"]
        self.A = S.padded(fed, S.F32, "cuda")
        self.Ap = S.padded_planes(S.split3(o["A"]), "cuda")                  # the restatement's planes of A (of the prologue's RESULT for a prologue case)
        self.Bp = S.padded_planes(S.split3(o["B"]), "cuda")
        self.bias, self.rowscale = o["bias"].cuda(), o["rowscale"].cuda()
        self.residual, self.second = S.padded(o["residual"], S.F32, "cuda"), S.padded(o["second"], S.F32, "cuda")
        self.z2 = o["second"]
        if case.entry == "pro":
            self.stat = torch.cat((o["mean"], o["rstd"])).cuda()
            self.gamma, self.beta = o["gamma"].cuda(), o["beta"].cuda()

    def launch(self, epi, entry=None, want_route=None):
        """One launch into fresh NaN-filled outputs; returns a dict of the output buffers and the reported route."""
        c, L = self.case, _L()
        entry = entry or c.entry
        out = dict(C=S.nan_out(c.M, c.N, S.F32, "cuda"))
        if epi in ("gelu_pre", "quick_pre"):
            out["preact"] = S.nan_out(c.M, c.N, S.F32, "cuda")
        if epi == "planes":
            out["c_planes"] = torch.full((3, c.M, c.N + S.PAD), S.NAN, dtype=S.BF16, device="cuda")
        nb = -(-c.M // 128)
        if epi == "stats":
            out["colstats"] = torch.full((nb + 1, 2, c.N), S.NAN, dtype=S.F32, device="cuda")      # (one row more than the kernel owns)
        P = {k: (v.data_ptr(), v.stride(-2)) for k, v in dict(B=self.Bp, residual=self.residual, second=self.second, **out).items()}
        P["bias"], P["rowscale"] = (self.bias.data_ptr(), 0), (self.rowscale.data_ptr(), 0)
        a = fill_args(L.Split3Args(), c, epi, P)
        lib, st = L.lib(), L.stream()
        if entry == "planes":
            a.a_planes, a.lda = self.Ap.data_ptr(), self.Ap.stride(1)
            route = route_of(a, 0)
        else:
            a.a_planes, a.lda = self.A.data_ptr(), self.A.stride(0)              # (read by the route report only: the af32 calls take A and lda as arguments)
            route = route_of(a, 1, 1 if entry == "pro" else 0, 1 if epi == "stats" else 0)
        if want_route is not None:
            assert route == want_route, f"{c.name} {epi} [{entry}]: gg_gemm_nt_split3_route reports {route}, the case records {want_route}"
        if entry == "planes":
            L.check(lib.gg_gemm_nt_split3_ex(C.byref(a), st), "gg_gemm_nt_split3_ex")
        elif entry == "pro":
            L.check(lib.gg_gemm_nt_split3_af32_pro(C.byref(a), self.A.data_ptr(), self.A.stride(0), 0, self.stat.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), 0,
                                                   None, st), "gg_gemm_nt_split3_af32_pro")
        elif epi == "stats":
            L.check(lib.gg_gemm_nt_split3_af32_stats(C.byref(a), self.A.data_ptr(), self.A.stride(0), 0, out["colstats"].data_ptr(), st), "gg_gemm_nt_split3_af32_stats")
        else:
            L.check(lib.gg_gemm_nt_split3_af32(C.byref(a), self.A.data_ptr(), self.A.stride(0), 0, st), "gg_gemm_nt_split3_af32")
        torch.cuda.synchronize()
        return out, route

    def check(self, epi, want_route=None, entry=None):
        """Route, result (bit for bit, or the activation gate of tests/act_cases.py at an f32 site), untouched pads; for an af32 case the plane-fed kernel on the
        restatement's planes must give the same bits."""
        c, N, w = self.case, self.case.N, self.want
        what = f"{c.name}/{self.fam} {epi}" + (f" [{entry}]" if entry else "")
        out, route = self.launch(epi, entry, want_route)
        got = out["C"][:, :N]
        kw = dict(granule=S.GRANULE[self.fam], tile=(S.TILE_M[route.kernel], route.tile_n))
        if epi in ("plain", "stats"):
            S.assert_bits(got, w["z"], what, **kw)
        elif epi in ("bias", "planes"):
            S.assert_bits(got, w["pre"], what, **kw)
        elif epi == "linear":
            S.assert_bits(got, w["linear"], what, **kw)
        elif epi in ("gelu_pre", "quick_pre"):
            S.assert_bits(out["preact"][:, :N], w["pre"], what + " pre-activation copy", **kw)
            S.assert_act_gate(got, w["pre"], "gelu" if epi == "gelu_pre" else "quick", what)
        else:
            S.assert_act_gate(got, self.z2, "gelu_grad" if epi == "dgelu" else "quick_grad", what, upstream=w["z"])
        for k in ("C", "preact"):
            if k in out:
                S.assert_pad_nan(out[k], N, f"{what} {k}")
                assert not bool(torch.isnan(out[k][:, :N]).any()), f"{what}: NaN left inside {k}"
        if epi == "planes":
            S.assert_planes_equal([out["c_planes"][i, :, :N] for i in range(3)], w["pre_planes"], what + " c_planes")
            S.assert_pad_nan(out["c_planes"], N, what + " c_planes")
        if epi == "stats":
            nb = -(-c.M // 128)
            cs = out["colstats"]
            assert torch.equal(cs[:nb].cpu(), w["colstats"]), f"{what}: colstats differ at {(cs[:nb].cpu() != w['colstats']).nonzero()[:4].tolist()}"
            assert bool(torch.isnan(cs[nb]).all()), f"{what}: a colstats row beyond ceil(M / 128) was written"
        if (entry or c.entry) in ("af32", "pro") and epi != "stats":
            ref, _ = self.launch(epi, "planes")
            for k in ("C", "preact", "c_planes"):
                if k in out:
                    assert torch.equal(out[k].view(torch.int32 if k != "c_planes" else torch.int16), ref[k].view(torch.int32 if k != "c_planes" else torch.int16)), \
                        f"{what}: {k} differs from the plane-fed kernel on the restatement's planes"
        return out


def check_case(case, under_switch=False):
    """Every family and epilogue of a case; all of them run, and the failures are reported together (which families fail tells which plane product is wrong)."""
    bad = []
    for fam in case.fams:
        d = DeviceCase(case, fam)
        for epi in case.epis:
            try:
                d.check(epi, S.run_route(case, epi) if (under_switch or case.group is None) else S.route_for(case, epi))
            except AssertionError as e:
                bad.append(str(e))
        del d
    assert not bad, f"{len(bad)} of {len(case.fams) * len(case.epis)} (family, epilogue) runs failed:\n" + "\n".join(bad)


# ---- TN -------------------------------------------------------------------------------------------------------------------------------------------------------
def check_tn(name):
    """gg_gemm_tn_split3 with the case's split count into a NaN-filled slab scratch, each slab and the gg_splitk_reduce result against the exact references."""
    c, L = S.TN_BY_NAME[name], _L()
    dY, X, rs = S.tn_operands(name)
    slabs, total = S.tn_expected(name)
    geo = S.tn_geometry(c.M, c.N, c.K, c.splits)
    dYd, Xd = S.padded(dY, S.F32, "cuda", tail_rows=8, pad=4), S.padded(X, S.F32, "cuda", tail_rows=8)
    ld_y = dYd.stride(0)
    assert ld_y == c.N + 4 and Xd.stride(0) == c.K + S.PAD
    rsd = None
    if rs is not None:
        rsd = torch.full((rs.numel() + 8,), S.NAN, device="cuda")
        rsd[:rs.numel()] = rs.cuda()
    part = torch.full((c.splits + 1, c.N, c.K), S.NAN, device="cuda")
    lib = L.lib()
    L.check(lib.gg_gemm_tn_split3(dYd.data_ptr(), ld_y, Xd.data_ptr(), Xd.stride(0), c.M, c.N, c.K, rsd.data_ptr() if rsd is not None else None,
                                  S.ROWS_PER_SCALE if rsd is not None else 0, part.data_ptr(), c.splits, L.stream()), "gg_gemm_tn_split3")
    out = torch.full((c.N * c.K + 8,), S.NAN, device="cuda")
    L.check(lib.gg_splitk_reduce(part.data_ptr(), out.data_ptr(), c.N * c.K, c.splits, 0, 1.0, L.stream()), "gg_splitk_reduce")
    torch.cuda.synchronize()
    for i in range(c.splits):
        S.assert_bits(part[i], slabs[i], f"{name} slab {i} ({geo})", granule=S.GRANULE[c.fam], tile=(256, 128))
    assert bool(torch.isnan(part[c.splits]).all()), f"{name}: the scratch behind the last slab was written"
    S.assert_bits(out[:c.N * c.K].view(c.N, c.K), total, f"{name} reduced", granule=S.GRANULE[c.fam], tile=(256, 128))
    assert bool(torch.isnan(out[c.N * c.K:]).all()), f"{name}: gg_splitk_reduce wrote behind its result"


# ---- gg_split3_bf16 -------------------------------------------------------------------------------------------------------------------------------------------
def check_split_edges():
    L = _L()
    x = S.split_edge_values()
    rows, cols = x.shape
    xd = S.padded(x, S.F32, "cuda")                                          # ldx = cols + 8
    planes = torch.full((3 * rows * cols + 8,), S.NAN, dtype=S.BF16, device="cuda")
    L.check(L.lib().gg_split3_bf16(xd.data_ptr(), rows, cols, xd.stride(0), planes.data_ptr(), L.stream()), "gg_split3_bf16")
    torch.cuda.synchronize()
    got = planes[:3 * rows * cols].view(3, rows, cols)
    S.assert_planes_equal([got[i] for i in range(3)], S.split3(x), "gg_split3_bf16 edge set")
    total = got.cpu().double().sum(0)
    assert bool(torch.isnan(total[torch.isnan(x)]).all()), "gg_split3_bf16: the planes of a NaN do not sum to NaN"
    fin = torch.isfinite(x) & ((x.abs() >= 2.0 ** -100) | (x == 0))            # (below 2^-110 the third plane leaves bf16's subnormal range)
    assert torch.equal(total[fin], x.double()[fin]), "gg_split3_bf16: the planes of a finite value do not sum to it"
    assert bool(torch.isnan(planes[3 * rows * cols:]).all()), "gg_split3_bf16 wrote behind its planes"
