"""Device side of tests/gemm16_cases.py: builds the GgGemmArgs of one (case, epilogue), asks gg_gemm_nt_route for its route, launches gg_gemm_nt / gg_gemm_nt_f16
and compares with the exact reference.  Shared by tests/test_gpu_gemm16_forms.py (no switches) and tools/gemm16_forms.py (a child process per switch group)."""
import ctypes as C

import torch

from tests import gemm16_cases as G

ENTRY = {G.BF16: "gg_gemm_nt", G.F16: "gg_gemm_nt_f16"}


def _L():
    from geoguessr_ai_amd import _lib
    return _lib


def route_of(args):
    """(kernel, tilesM, tilesN, group_m) that gg_gemm_nt_route reports for exactly the arguments of the launch."""
    L = _L()
    g, tm, tn = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    k = L.lib().gg_gemm_nt_route(C.byref(args), C.byref(g), C.byref(tm), C.byref(tn))
    if k < 0:
        raise L.GgError(f"gg_gemm_nt_route refused the arguments: {L.lib().gg_last_error().decode(errors='replace')}")
    return (k, tm.value, tn.value, g.value)


class DeviceCase:
    """The operands of one case on the device in one 16-bit type (NaN-padded buffers), and its exact results."""

    def __init__(self, case, dtype):
        self.case, self.dtype = case, dtype
        o, e = G.operands(case.name), G.expected(case.name)
        self.A, self.B = G.padded(o["A"], dtype, "cuda"), G.padded(o["B"], dtype, "cuda")
        self.residual = G.padded(o["residual"], dtype, "cuda")
        self.second = G.padded(o["second"], dtype, "cuda") if o["second"] is not None else None
        self.bias, self.rowscale = o["bias"].cuda(), o["rowscale"].cuda()
        self.want = {k: v.cuda() for k, v in e.items()}

    def args(self, epi, out, pre):
        c, L = self.case, _L()
        a = L.GemmArgs()
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc = self.A.data_ptr(), self.A.stride(0), self.B.data_ptr(), self.B.stride(0), out.data_ptr(), out.stride(0)
        a.M, a.N, a.K, a.split_k = c.M, c.N, c.K, 1
        if epi == "linear":
            a.bias, a.rowscale, a.rows_per_scale = self.bias.data_ptr(), self.rowscale.data_ptr(), G.ROWS_PER_SCALE
            a.residual, a.ldr = self.residual.data_ptr(), self.residual.stride(0)
        elif epi in ("gelu_pre", "quick_pre", "quick"):
            a.bias, a.act = self.bias.data_ptr(), G.ACT_CODE["gelu" if epi == "gelu_pre" else "quick"]
            a.preact = pre.data_ptr() if pre is not None else None
        elif epi in ("dgelu", "dquick"):
            assert self.second.stride(0) == out.stride(0)                  # (the saved pre-activation has the pitch of C)
            a.dact_preact, a.dact = self.second.data_ptr(), G.ACT_CODE["gelu" if epi == "dgelu" else "quick"]
        else:
            assert epi == "plain", epi
        return a

    def launch(self, epi, want_route=None):
        """One launch into fresh NaN-filled outputs; returns (C buffer, pre-activation buffer or None, reported route)."""
        c, L = self.case, _L()
        out = G.nan_out(c.M, c.N, self.dtype, "cuda")
        pre = G.nan_out(c.M, c.N, self.dtype, "cuda") if epi in ("gelu_pre", "quick_pre") else None
        a = self.args(epi, out, pre)
        route = route_of(a)
        if want_route is not None:
            assert route == tuple(want_route), (f"{c.name} {epi}: gg_gemm_nt_route reports {G.ROUTE_NAME[route[0]]} tiles {route[1]} x {route[2]} group_m {route[3]}, the case "
                                                f"records {G.ROUTE_NAME[want_route[0]]} tiles {want_route[1]} x {want_route[2]} group_m {want_route[3]}")
        L.check(getattr(L.lib(), ENTRY[self.dtype])(C.byref(a), L.stream()), ENTRY[self.dtype])
        torch.cuda.synchronize()
        return out, pre, route

    def check(self, epi, want_route=None):
        """Route, result (bit for bit, or the activation gate of tests/act_cases.py), untouched pad columns, and the same bits from a second call."""
        c, N = self.case, self.case.N
        what = f"{c.name} {str(self.dtype)[6:]} {epi}"
        out, pre, route = self.launch(epi, want_route)
        k = route[0]
        if epi == "plain":
            G.assert_bits(out[:, :N], self.want["z"], k, what)
        elif epi == "linear":
            G.assert_bits(out[:, :N], self.want["linear"], k, what)
        elif epi in ("gelu_pre", "quick_pre"):
            G.assert_bits(pre[:, :N], self.want["pre"], k, what + " pre-activation copy")
            G.assert_pad_nan(pre, N, what + " pre-activation copy")
            G.assert_act_gate(out[:, :N], self.want["pre"], "gelu" if epi == "gelu_pre" else "quick", self.dtype, what)
        elif epi == "quick":
            G.assert_act_gate(out[:, :N], self.want["pre"], "quick", self.dtype, what)
        else:
            G.assert_act_gate(out[:, :N], self.second[:, :N], "gelu_grad" if epi == "dgelu" else "quick_grad", self.dtype, what, upstream=self.want["z"])
        G.assert_pad_nan(out, N, what)
        out2, pre2, _ = self.launch(epi, want_route)
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), f"{what}: a second call gave other bits"
        assert pre is None or torch.equal(pre.view(torch.int16), pre2.view(torch.int16)), f"{what}: a second call gave another pre-activation copy"
        return out, pre
