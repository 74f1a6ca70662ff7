"""Memory discipline of the C ABI (include/gg.h: "all pointers are CALLER-OWNED DEVICE pointers", "matrices are row-major with an explicit leading
dimension"): a result may depend only on the LOGICAL elements of the inputs, and only the LOGICAL elements of the outputs may change.

Every tensor of every call here lives in a guarded buffer (tests/guards.py: bands of at least 256 rows / 64 KiB either side, padded rows, column
slices of wider buffers).  Each case is run twice, with the bands / padding / neighbouring columns holding NaN (0xFF bytes) and holding a large finite
value (0x47 bytes), and asserts, under both fills:
  1. every input buffer is bit-identical to before the call (payload, padding, bands);
  2. of every output buffer only the logical elements changed, and all of them were written (they start as NaN);
  3. the logical outputs of the two runs are BIT-IDENTICAL (exemptions -- float atomics -- are named where they apply);
  4. the values match the CPU reference of the kernel's parity test at that test's tolerance.
Scratch and partial buffers have exactly the size the library's capacity function returns.  The calls go through the C ABI (geoguessr_ai_amd._lib),
not ops.py, whose wrappers allocate the outputs themselves.  No pointer leaves a buffer this file owns: nothing here can fault the device.

CASES is the registry of what is called; tests/test_guards_cpu.py::test_every_entry_point_is_guarded_or_exempt holds it (with tests/test_gpu_guards_model.py's
MODEL_ENTRIES and an exemption table) against the header."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests import guards as G

pytestmark = pytest.mark.gpu

BF, F16, F32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int64

# entry points each case function calls (the CPU coverage test reads this without a GPU)
CASES = {}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def _L():
    from geoguessr_ai_amd import _lib as L
    L.require_gpu()
    return L


def rnd(*shape, seed=0, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).float()      # representable in `dtype`, held as fp32


def close(got, ref, rtol, atol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.4g} (ref max {float(ref.abs().max()):.4g})"


def rel_max(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


def rel_l2(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


def run_guarded(call, atomic=()):
    """call(S) -> (outputs {name: Guarded}, check(values {name: cpu tensor})).  Runs it under both fills; asserts 1-4 of the module docstring.
    `atomic`: outputs summed with float atomics, compared at 1e-5 of the largest magnitude (the tolerance of tests/test_gpu_recompute.py)."""
    L = _L()
    got, check = {}, None
    for fill in ("nan", "finite"):
        S = G.GuardSet(fill)
        outs, check = call(S, L)
        S.check()
        got[fill] = {k: v.view.clone() for k, v in outs.items()}
    for k in got["nan"]:
        a, b = got["nan"][k], got["finite"][k]
        if k in atomic:
            assert float((a.double() - b.double()).abs().max()) <= 1e-5 * float(a.double().abs().max()), k
        else:
            G.assert_bit_identical(a, b, k)
    check({k: v.cpu() for k, v in got["finite"].items()})


# ------------------------------------------------------------------------------------------- the helper itself, on the device
def test_helper_flags_a_one_element_overrun_of_a_real_kernel():
    """gg_fill_f32 told n + 1 where the helper was told n: the kernel legitimately writes one element into what the helper believes is the back
    band (or, with a padded row, the row padding).  Inside the test's own allocation; no kernel is broken for it."""
    L = _L()
    for fill in ("nan", "finite"):
        S = G.GuardSet(fill)
        o = S.out("p", 1, 1000, F32)
        L.check(L.lib().gg_fill_f32(o.ptr, 1001, L.f32(3.0), L.stream()), "gg_fill_f32")
        v = S.violations()
        assert len(v) == 1 and "p: output back band changed (4 bytes, first at byte +4000" in v[0], v
        S = G.GuardSet(fill)
        o = S.out("p", 1, 1000, F32, ld=1008)
        L.check(L.lib().gg_fill_f32(o.ptr, 1001, L.f32(3.0), L.stream()), "gg_fill_f32")
        v = S.violations()
        assert len(v) == 1 and "p: output row padding changed (4 bytes, first at byte +4000" in v[0], v
        S = G.GuardSet(fill)
        o = S.out("p", 1, 1000, F32)
        L.check(L.lib().gg_fill_f32(o.ptr, 999, L.f32(3.0), L.stream()), "gg_fill_f32")
        v = S.violations()
        assert len(v) == 1 and "p: output payload has 1 NaN logical elements" in v[0] and "first at [0, 999]" in v[0], v
        S = G.GuardSet(fill)
        i = S.inp("x", torch.ones(1000))
        L.check(L.lib().gg_fill_f32(i.ptr + 4 * 10, 1, L.f32(3.0), L.stream()), "gg_fill_f32")
        v = S.violations()
        assert len(v) == 1 and "x: input payload changed (2 bytes, first at byte +42" in v[0], v      # 1.0 -> 3.0: 0x3F80 -> 0x4040
        S = G.GuardSet(fill)
        o = S.out("p", 1, 1000, F32)
        L.check(L.lib().gg_fill_f32(o.ptr, 1000, L.f32(3.0), L.stream()), "gg_fill_f32")
        S.check()


# ------------------------------------------------------------------------------------------- small kernels
@case("gg_fill_f32", "gg_cast_f32_to_bf16", "gg_cast_bf16_to_f32", "gg_cast_f32_to_f16", "gg_cast_f16_to_f32")
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("mis", [0, 16])
def test_fill_and_casts(n, mis):
    x = rnd(n, seed=n)

    def call(S, L):
        lib, st = L.lib(), L.stream()
        xi = S.inp("x", x, misalign=mis)
        xb = S.inp("xb", x.to(BF), misalign=mis); xh = S.inp("xh", x.to(F16), misalign=mis)
        o = {"fill": S.out("fill", 1, n, F32, misalign=mis), "bf": S.out("bf", 1, n, BF, misalign=mis), "f16": S.out("f16", 1, n, F16, misalign=mis),
             "from_bf": S.out("from_bf", 1, n, F32, misalign=mis), "from_f16": S.out("from_f16", 1, n, F32, misalign=mis)}
        L.check(lib.gg_fill_f32(o["fill"].ptr, n, L.f32(-2.5), st), "fill")
        L.check(lib.gg_cast_f32_to_bf16(xi.ptr, o["bf"].ptr, n, st), "cast")
        L.check(lib.gg_cast_f32_to_f16(xi.ptr, o["f16"].ptr, n, st), "cast")
        L.check(lib.gg_cast_bf16_to_f32(xb.ptr, o["from_bf"].ptr, n, st), "cast")
        L.check(lib.gg_cast_f16_to_f32(xh.ptr, o["from_f16"].ptr, n, st), "cast")

        def check(v):
            assert torch.equal(v["fill"], torch.full((1, n), -2.5))
            assert torch.equal(v["bf"], x.to(BF)[None]) and torch.equal(v["f16"], x.to(F16)[None])          # round to nearest even, as torch
            assert torch.equal(v["from_bf"], x.to(BF).float()[None]) and torch.equal(v["from_f16"], x.to(F16).float()[None])
        return o, check
    run_guarded(call)


@case("gg_transpose_bf16", "gg_transpose_f32", "gg_cast_transpose_f32")
@pytest.mark.parametrize("R,Cc,pad", [(64, 64, 0), (65, 63, 8), (63, 65, 24), (1, 8, 8), (333, 40, 3)])
def test_transposes(R, Cc, pad):
    x = rnd(R, Cc, seed=R + Cc, dtype=BF)
    rs = torch.tensor([2.0, 0.0, 0.5])
    rps = (R + 2) // 3

    def call(S, L):
        lib, st = L.lib(), L.stream()
        xb = S.inp("x_bf16", x.to(BF), ld=Cc + pad, misalign=16)
        xf = S.inp("x_f32", x)                                        # gg_transpose_f32 / gg_cast_transpose_f32 read a dense [R, C]
        r = S.inp("rowscale", rs)
        o = {"t": S.out("t", Cc, R, BF, ld=R + pad), "ts": S.out("ts", Cc, R, BF, ld=R + pad, misalign=16), "t32": S.out("t32", Cc, R, F32, ld=R + pad),
             "c": S.out("c", R, Cc, BF, ld=Cc + pad), "ct": S.out("ct", Cc, R, BF, ld=R + pad)}
        L.check(lib.gg_transpose_bf16(xb.ptr, xb.ld, o["t"].ptr, o["t"].ld, R, Cc, None, 0, st), "transpose")
        L.check(lib.gg_transpose_bf16(xb.ptr, xb.ld, o["ts"].ptr, o["ts"].ld, R, Cc, r.ptr, rps, st), "transpose")
        L.check(lib.gg_transpose_f32(xf.ptr, R, Cc, o["t32"].ptr, o["t32"].ld, st), "transpose_f32")
        L.check(lib.gg_cast_transpose_f32(xf.ptr, R, Cc, o["c"].ptr, o["c"].ld, o["ct"].ptr, o["ct"].ld, st), "cast_transpose")

        def check(v):
            assert torch.equal(v["t"].float(), x.t()) and torch.equal(v["t32"], x.t())                       # tests/test_gpu_kernels.py: rtol 0, atol 0
            assert torch.equal(v["c"].float(), x) and torch.equal(v["ct"].float(), x.t())
            close(v["ts"], (x * rs.repeat_interleave(rps)[:R, None]).t(), 1e-2, 1e-2, "scaled transpose")
        return o, check
    run_guarded(call)


@case("gg_splitk_reduce")
@pytest.mark.parametrize("n,splits,acc", [(4096, 3, 0), (4097, 7, 1), (8, 70, 1), (1, 1, 0), (1536, 68, 0)])
def test_splitk_reduce(n, splits, acc):
    p = rnd(splits, n, seed=n + splits)

    def call(S, L):
        pi = S.inp("partials", p)
        o = S.out("out", 1, n, F32, init=torch.full((n,), 2.0) if acc else None, misalign=16 if n % 2 else 0)
        L.check(L.lib().gg_splitk_reduce(pi.ptr, o.ptr, n, splits, acc, L.f32(0.5), L.stream()), "gg_splitk_reduce")
        return {"out": o}, lambda v: close(v["out"][0], 2.0 * acc + 0.5 * p.double().sum(0), 1e-4, 1e-2, "splitk_reduce")
    run_guarded(call)


@case("gg_adamw_step")
@pytest.mark.parametrize("n", [1, 1021, 4096, 4099])
def test_adamw(n):
    """tests/test_gpu_kernels.py::test_adamw_matches_torch's reference (torch.optim.AdamW, one step) and tolerance."""
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2, scale=0.1)

    def call(S, L):
        # parameters and moments are updated in place: outputs that start from known values
        p = S.out("params", 1, n, F32, init=p0, misalign=16); m = S.out("exp_avg", 1, n, F32, init=torch.zeros(n)); v = S.out("exp_avg_sq", 1, n, F32, init=torch.zeros(n))
        g = S.inp("grads", g0 * 4.0, misalign=16)
        L.check(L.lib().gg_adamw_step(p.ptr, g.ptr, m.ptr, v.ptr, n, 1, L.f32(1e-3), L.f32(0.9), L.f32(0.999), L.f32(1e-8), L.f32(0.01), L.f32(0.25),
                                      L.stream()), "gg_adamw_step")

        def check(val):
            q = torch.nn.Parameter(p0.clone()); q.grad = g0.clone()
            torch.optim.AdamW([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01).step()
            close(val["params"][0], q.detach(), 1e-5, 1e-6, "adamw params")
            close(val["exp_avg"][0], 0.1 * g0, 1e-5, 1e-7, "exp_avg")
        return {"params": p, "exp_avg": m, "exp_avg_sq": v}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- GEMM, nt forms
# (M, N, K, pad of lda / ldb, pad of ldc, column offset of A inside a wider buffer).  gemm.hip's dispatch: 128 x 128 tiles, 128 x 64 when the last N tile would be
# at most half full, BK = 64; the LDS-DMA form (192 x 128 tiles) from M >= 1024, N >= 128, K >= 192; K, lda, ldb multiples of 8.
NT_SHAPES = [(128, 128, 64, 0, 0, 0),        # exact tiles
             (129, 129, 72, 8, 8, 0),        # one past
             (127, 127, 56, 24, 3, 0),       # one short; non-power-of-two pads
             (1, 8, 8, 8, 1, 8),             # the smallest call; A is a column slice
             (130, 200, 136, 24, 8, 16),     # 128 + 72 columns: wide tile, ragged; column slice
             (1030, 200, 192, 8, 8, 8)]      # the LDS-DMA form (bf16 / fp16) with padded rows everywhere


def _gemm_args(L, S, A, B, M, N, K, pad, padc, aoff, dt, out_dt):
    a = L.GemmArgs()
    Ai = S.inp("A", A.to(dt), ld=K + pad + aoff, col_off=aoff, misalign=16)
    Bi = S.inp("B", B.to(dt), ld=K + pad)
    Co = S.out("C", M, N, out_dt, ld=N + padc)
    a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N, a.K = Ai.ptr, Ai.ld, Bi.ptr, Bi.ld, Co.ptr, Co.ld, M, N, K
    a.split_k = 1
    return a, Co


def _gelu_grad(h):
    hh = h.double().clone().requires_grad_(True)
    F.gelu(hh).sum().backward()
    return hh.grad


EPILOGUES = ["plain", "out_f32", "bias_gelu_preact", "quick_gelu", "rowscale_residual", "dact", "colstats"]


def _nt_case(entry, dt, M, N, K, pad, padc, aoff, epi):
    """One epilogue of gg_gemm_nt / _f16 / _f32.  Tolerances: test_gemm_plain / test_gemm_epilogues (bf16: rtol = atol = 1e-2; f32 output 1e-4 / 1e-3; column
    statistics 1e-3 / 0.3), test_f32_gemm_small_m_form_and_split_k (f32: 4e-6 of the largest magnitude, 2e-5 for K > 1000); fp16 has no kernel-level parity test:
    its bound is the format's (f32 accumulation, one rounding to 11 bits: 2^-11 relative, taken as rtol = atol = 1e-3 with operands of unit scale)."""
    A, B = rnd(M, K, seed=M + 1, dtype=dt), rnd(N, K, seed=N + 2, scale=0.1 if dt != F32 else K ** -0.5, dtype=dt)
    bias, res, h = rnd(N, seed=5), rnd(M, N, seed=6, dtype=dt), rnd(M, N, seed=7, dtype=dt)
    rps = max(1, M // 4)
    rs = (torch.rand((M + rps - 1) // rps, generator=torch.Generator().manual_seed(3)) > 0.3).float() * 1.25
    rs_rows = rs.double().repeat_interleave(rps)[:M, None]
    z = A.double() @ B.double().t()
    if dt == F32:
        tol = 2e-5 if K > 1000 else 4e-6
        cmp = lambda got, ref, what: (lambda e: None if e < tol else pytest.fail(f"{what}: rel {e:.3e} >= {tol}"))(rel_max(got, ref))
    elif epi == "out_f32":                                       # exact products, f32 accumulation, f32 store: test_gemm_plain's f32-output bound for either 16-bit type
        cmp = lambda got, ref, what: close(got, ref, 1e-4, 1e-3, what)
    else:
        rt = 1e-2 if dt == BF else 1e-3
        cmp = lambda got, ref, what: close(got, ref, rt, rt, what)

    def call(S, L):
        a, Co = _gemm_args(L, S, A, B, M, N, K, pad, padc, aoff, dt, F32 if (epi == "out_f32" or dt == F32) else dt)
        outs = {"C": Co}
        ref = {"C": z}
        if epi == "out_f32":
            a.out_f32 = 1
            a.bias = S.inp("bias", bias, misalign=16).ptr; ref["C"] = z + bias.double()
        elif epi == "bias_gelu_preact":
            pre = S.out("preact", M, N, dt, ld=N + padc)
            a.bias, a.act, a.preact = S.inp("bias", bias).ptr, 1, pre.ptr
            outs["preact"] = pre; ref["preact"] = z + bias.double(); ref["C"] = F.gelu(z + bias.double())
        elif epi == "quick_gelu":
            a.bias, a.act = S.inp("bias", bias, misalign=16).ptr, 2
            zb = z + bias.double(); ref["C"] = zb * torch.sigmoid(1.702 * zb)
        elif epi == "rowscale_residual":
            r = S.inp("residual", res.to(dt), ld=N + padc + (8 if padc else 0))
            a.bias, a.rowscale, a.rows_per_scale, a.residual, a.ldr = S.inp("bias", bias).ptr, S.inp("rowscale", rs).ptr, rps, r.ptr, r.ld
            ref["C"] = res.double() + rs_rows * (z + bias.double())
        elif epi == "dact":
            a.dact_preact, a.dact = S.inp("dact_preact", h.to(dt), ld=N + padc).ptr, 1
            ref["C"] = z * _gelu_grad(h)
        elif epi == "colstats":
            rows = L.lib().gg_gemm_colstats_rows(M)
            st = S.out("colstats", rows, 2 * N, F32)            # exactly gg_gemm_colstats_rows(M) rows of [2][N]
            a.colstats = st.ptr
            outs["colstats"] = st
        L.check(getattr(L.lib(), entry)(C.byref(a), L.stream()), entry)

        def check(v):
            cmp(v["C"], ref["C"], f"{entry} {epi} C")
            if "preact" in v:
                cmp(v["preact"], ref["preact"], f"{entry} {epi} preact")
            if "colstats" in v:
                raw = v["C"].double()                            # statistics of the stored (rounded) result
                s = v["colstats"].double().view(-1, 2, N).sum(0)
                close(s[0], raw.sum(0), 1e-3, 0.3, "colsum"); close(s[1], (raw * raw).sum(0), 1e-3, 0.3, "colsumsq")
        return outs, check
    run_guarded(call)


@case("gg_gemm_nt")
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("M,N,K,pad,padc,aoff", NT_SHAPES)
def test_gemm_nt_bf16(M, N, K, pad, padc, aoff, epi):
    _nt_case("gg_gemm_nt", BF, M, N, K, pad, padc, aoff, epi)


@case("gg_gemm_nt_f16")
@pytest.mark.parametrize("epi", ["plain", "out_f32", "bias_gelu_preact", "quick_gelu", "rowscale_residual", "dact"])     # colstats / split-K / BatchNorm forms: refused (below)
@pytest.mark.parametrize("M,N,K,pad,padc,aoff", NT_SHAPES)
def test_gemm_nt_f16(M, N, K, pad, padc, aoff, epi):
    _nt_case("gg_gemm_nt_f16", F16, M, N, K, pad, padc, aoff, epi)


# gemm_f32.hip: 128-row tiles, 64 x 64 tiles up to 256 tiles of 128 rows (every shape here but the last), K, lda, ldb multiples of 4; a long contraction of a small launch is
# split into slabs the library owns (70 x 68 x 1028, 8 x 320 x 2056)
NT_F32_SHAPES = NT_SHAPES[:5] + [(65, 63, 52, 4, 1, 4), (70, 68, 1028, 4, 4, 0), (8, 320, 2056, 12, 8, 4),
                                 (16641, 129, 8, 4, 1, 4)]      # 131 x 3 = 393 tiles of 128 x 64 (> 256): the main 128-row kernel's epilogues, ragged in M and N


@case("gg_gemm_nt_f32")
@pytest.mark.parametrize("epi", ["plain", "bias_gelu_preact", "rowscale_residual", "dact", "colstats"])
@pytest.mark.parametrize("M,N,K,pad,padc,aoff", NT_F32_SHAPES)
def test_gemm_nt_f32(M, N, K, pad, padc, aoff, epi):
    _nt_case("gg_gemm_nt_f32", F32, M, N, K, pad, padc, aoff, epi)


@case("gg_gemm_nt", "gg_splitk_reduce")
@pytest.mark.parametrize("M,N,K,split", [(128, 128, 448, 7), (129, 65, 200, 3), (1, 8, 136, 2)])
def test_gemm_nt_caller_split_k(M, N, K, split):
    """GgGemmArgs.split_k > 1: C is f32 [split_k][M][ldc] partials (test_gemm_splitk_and_wgrad_form: rtol 1e-4, atol 1e-2)."""
    A, B = rnd(M, K, seed=11, dtype=BF), rnd(N, K, seed=12, scale=0.1, dtype=BF)

    def call(S, L):
        a = L.GemmArgs()
        Ai, Bi = S.inp("A", A.to(BF), ld=K + 8), S.inp("B", B.to(BF), ld=K + 24)
        P = S.out("partials", split * M, N, F32)
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N, a.K, a.out_f32, a.split_k = Ai.ptr, Ai.ld, Bi.ptr, Bi.ld, P.ptr, N, M, N, K, 1, split
        L.check(L.lib().gg_gemm_nt(C.byref(a), L.stream()), "gg_gemm_nt(split)")
        o = S.out("out", 1, M * N, F32, init=torch.ones(M * N))
        torch.cuda.synchronize()
        Pi = S.inp("partials_in", P.view.cpu())
        L.check(L.lib().gg_splitk_reduce(Pi.ptr, o.ptr, M * N, split, 1, L.f32(1.0), L.stream()), "gg_splitk_reduce")
        return {"partials": P, "out": o}, lambda v: close(v["out"].view(M, N), 1.0 + A.double() @ B.double().t(), 1e-4, 1e-2, "split-k")
    run_guarded(call)


@case("gg_gemm_f32_set_trace", "gg_gemm_nt_f32")
@pytest.mark.parametrize("M,N,K,tiles", [(300, 200, 96, 20), (16641, 129, 8, 393)])
def test_gemm_f32_trace_buffer(M, N, K, tiles):
    """The dev timeline of gg_gemm_nt_f32 (8 x uint64 per workgroup: 5 x 4 tiles of 64 x 64 for the small launch; 131 x 3 tiles of 128 x 64 for the large one, whose
    last 128 columns would hold one: gemm_f32.hip takes the 64-wide tile then): every record
    of a buffer of exactly that size is written, nothing beyond it, and the product is the untraced one.  The records hold hardware clocks: they are the one output here
    that is not compared between the fills.  The hook is process-global state: switched off again whatever happens."""
    A, B = rnd(M, K, seed=5), rnd(N, K, seed=6, scale=K ** -0.5)
    ref = A.double() @ B.double().t()

    def call(S, L):
        lib = L.lib()
        a, Co = _gemm_args(L, S, A, B, M, N, K, 4, 1, 4, F32, F32)
        tr = S.out("trace", tiles, 8, I64)
        try:
            L.check(lib.gg_gemm_f32_set_trace(tr.ptr), "gg_gemm_f32_set_trace")
            L.check(lib.gg_gemm_nt_f32(C.byref(a), L.stream()), "gg_gemm_nt_f32 (traced)")
            torch.cuda.synchronize()
        finally:
            lib.gg_gemm_f32_set_trace(None)
        changed = (tr.view != -1).any(1)          # the logical records start as 0xFF bytes under either fill
        assert bool(changed.all()), f"{int((~changed).sum())} of {tiles} trace records never written"
        return {"C": Co}, lambda v: None if rel_max(v["C"], ref) < 4e-6 else pytest.fail(f"traced gemm rel {rel_max(v['C'], ref):.2e}")
    run_guarded(call)


@case("gg_gemm_nt", "gg_gemm_nt_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("M,K,N,act", [(300, 384, 96, 1), (129, 160, 48, 1), (1, 64, 200, 0), (257, 1024, 129, 2)])
def test_gemm_nt_batchnorm_prologue(dt, M, K, N, act):
    """GgGemmArgs.a_bn_*: A := act(gamma * (A - mean) * rstd + beta) while the tile is staged (test_gemm_batchnorm_prologue: bf16 rtol 2e-2 / atol 3e-2 of
    the bf16-rounded activation; f32 at the f32 GEMM's 2e-5 of the largest magnitude)."""
    y = rnd(M, K, seed=21, dtype=dt); W = rnd(N, K, seed=22, scale=K ** -0.5, dtype=dt)
    mean, rstd = rnd(K, seed=23, scale=0.3), torch.rand(K, generator=torch.Generator().manual_seed(24)) + 0.5
    gamma, beta = rnd(K, seed=25) * 0.5 + 1.0, rnd(K, seed=26, scale=0.2)
    u = (y.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()
    act_u = F.gelu(u) if act == 1 else (u * torch.sigmoid(1.702 * u) if act == 2 else u)

    def call(S, L):
        a, Co = _gemm_args(L, S, y, W, M, N, K, 8, 8, 8, dt, dt)
        a.a_bn_stat = S.inp("a_bn_stat", torch.cat([mean, rstd]), misalign=16).ptr
        a.a_bn_gamma, a.a_bn_beta, a.a_bn_act = S.inp("gamma", gamma).ptr, S.inp("beta", beta).ptr, act
        if dt == BF and act == 2:
            # gg_gemm_nt's prologue has no QuickGELU form: refused on the host, nothing touched (test_unsupported_gemm_forms_are_refused holds the refusal itself);
            # this case keeps its place in the list so that the f32 twin and the bf16 entry point see the same shapes
            assert L.lib().gg_gemm_nt(C.byref(a), L.stream()) < 0 and b"a_bn_act" in L.lib().gg_last_error()
            Co.view.zero_(); Co.before = Co.buf.clone()
            return {"C": Co}, lambda v: None
        L.check((L.lib().gg_gemm_nt if dt == BF else L.lib().gg_gemm_nt_f32)(C.byref(a), L.stream()), "gemm a_bn")

        def check(v):
            if dt == BF:
                close(v["C"], act_u.to(BF).double() @ W.double().t(), 2e-2, 3e-2, "bn prologue bf16")
            else:
                assert rel_max(v["C"], act_u @ W.double().t()) < 2e-5
        return {"C": Co}, check
    run_guarded(call)


@case("gg_gemm_nt", "gg_gemm_nt_f16")
def test_unsupported_gemm_forms_are_refused():
    """Forms a GEMM entry point does not implement are refused on the host with a message, and nothing is touched: gg_gemm_nt's BatchNorm prologue with QuickGELU (it used to
    run silently WITHOUT the activation; gg_gemm_nt_f32 has that form), and gg_gemm_nt_f16 with column statistics, caller split-K or the BatchNorm prologue."""
    L = _L()
    M, N, K = 257, 129, 1024
    A, B, v = rnd(M, K, seed=1, dtype=BF), rnd(N, K, seed=2, scale=0.03, dtype=BF), rnd(2 * K, seed=3).abs() + 0.5
    for fill in ("nan", "finite"):
        for entry, dt, form in (("gg_gemm_nt", BF, "quick_gelu_prologue"), ("gg_gemm_nt_f16", F16, "colstats"), ("gg_gemm_nt_f16", F16, "split_k"), ("gg_gemm_nt_f16", F16, "prologue")):
            S = G.GuardSet(fill)
            a, Co = _gemm_args(L, S, A, B, M, N, K, 8, 8, 8, dt, dt)
            if form in ("quick_gelu_prologue", "prologue"):
                a.a_bn_stat, a.a_bn_gamma, a.a_bn_beta = S.inp("stat", v).ptr, S.inp("gamma", v[:K]).ptr, S.inp("beta", v[K:]).ptr
                a.a_bn_act = 2 if form == "quick_gelu_prologue" else 1
            elif form == "colstats":
                a.colstats = S.out("colstats", L.lib().gg_gemm_colstats_rows(M), 2 * N, F32).ptr
            else:
                a.split_k, a.out_f32 = 2, 1
            assert getattr(L.lib(), entry)(C.byref(a), L.stream()) < 0, (entry, form)
            msg = L.lib().gg_last_error()
            assert (b"a_bn_act" in msg) if form == "quick_gelu_prologue" else (b"gg_gemm_nt_f16" in msg), msg
            torch.cuda.synchronize()
            for g in S.tensors:
                assert not any(g.regions().values()), (entry, form, g.name)          # refused before any launch: every byte as before


@case("gg_gemm_nt")
@pytest.mark.parametrize("M,N,ks", [(300, 96, 128), (129, 64, 64), (1, 8, 64)])
def test_gemm_nt_two_source(M, N, ks):
    """GgGemmArgs.A2 / k_split: contraction columns k >= k_split come from A2 (same lda).  C = [A | A2] . B^T + bias (bf16 GEMM tolerance of test_gemm_epilogues)."""
    dt = BF
    K = 2 * ks
    A1, A2, B, bias = rnd(M, ks, seed=31, dtype=dt), rnd(M, ks, seed=32, dtype=dt), rnd(N, K, seed=33, scale=0.1, dtype=dt), rnd(N, seed=34)
    ref = torch.cat([A1, A2], 1).double() @ B.double().t() + bias.double()

    def call(S, L):
        a = L.GemmArgs()
        Ai, A2i = S.inp("A", A1.to(dt), ld=ks + 8, misalign=16), S.inp("A2", A2.to(dt), ld=ks + 8)
        Bi, Co = S.inp("B", B.to(dt), ld=K + 8), S.out("C", M, N, dt, ld=N + 8)
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N, a.K, a.split_k = Ai.ptr, Ai.ld, Bi.ptr, Bi.ld, Co.ptr, Co.ld, M, N, K, 1
        a.A2, a.k_split, a.bias = A2i.ptr, ks, S.inp("bias", bias).ptr
        L.check(L.lib().gg_gemm_nt(C.byref(a), L.stream()), "gemm A2")
        return {"C": Co}, lambda v: close(v["C"], ref, 1e-2, 1e-2, "two-source")
    run_guarded(call)


# ------------------------------------------------------------------------------------------- split-product GEMM, nt forms
def _planes_ref(x):
    """x = p1 + p2 + p3, each term the bf16 rounding of what is left (what gg_split3_bf16 computes)."""
    p1 = x.to(BF); r = x - p1.float(); p2 = r.to(BF); p3 = (r - p2.float()).to(BF)
    return torch.stack([p1, p2, p3])


@case("gg_split3_bf16")
@pytest.mark.parametrize("rows,cols,pad", [(128, 64, 0), (129, 68, 4), (1, 8, 4), (300, 96, 24), (257, 4, 12)])
def test_split3_planes(rows, cols, pad):
    x = rnd(rows, cols, seed=rows)

    def call(S, L):
        xi = S.inp("x", x, ld=cols + pad, misalign=16 if pad else 0)
        P = S.out("planes", 3 * rows, cols, BF)
        L.check(L.lib().gg_split3_bf16(xi.ptr, rows, cols, xi.ld, P.ptr, L.stream()), "gg_split3_bf16")

        def check(v):
            resid = (x.double() - v["planes"].double().view(3, rows, cols).sum(0)).abs().max() / x.abs().max()
            assert float(resid) < 2 ** -22, float(resid)          # test_split3_gemm_is_fp32_accurate's criterion
        return {"planes": P}, check
    run_guarded(call)


S3_SHAPES = [(128, 128, 32, 0, 0), (129, 129, 40, 8, 8), (127, 127, 24, 24, 3), (1, 8, 8, 8, 1), (300, 200, 96, 8, 8), (257, 90, 416, 24, 8), (130, 192, 392, 8, 0)]


@case("gg_gemm_nt_split3", "gg_gemm_nt_split3_ex", "gg_gemm_nt_split3_af32")
@pytest.mark.parametrize("epi", ["bias", "bias_gelu_preact", "rowscale_residual", "dact", "planes_out"])
@pytest.mark.parametrize("M,N,K,pad,padc", S3_SHAPES)
def test_split3_gemm_forms(M, N, K, pad, padc, epi):
    """The plane-fed kernel and the f32-activation form on the same operands: f32-accurate against fp64 (rel-L2 < 1e-6: test_split3_gemm_is_fp32_accurate),
    epilogues at test_split3_gemm_with_f32_activation_operand's 1e-5, and af32 bit-identical to the plane-fed call (same products, same order).
    The weight planes sit b_plane_stride apart (a gap of one padded row more than N * ldb)."""
    A, B = rnd(M, K, seed=M + K), rnd(N, K, seed=N + K, scale=K ** -0.5)
    bias, res, h = rnd(N, seed=5), rnd(M, N, seed=6), rnd(M, N, seed=7)
    rps = max(1, M // 3)
    rs = torch.tensor([1.0 / 0.7, 0.0, 1.0 / 0.7, 1.0 / 0.7])[:(M + rps - 1) // rps]
    rs_rows = rs.double().repeat_interleave(rps)[:M, None]
    z = A.double() @ B.double().t()
    Ap, Bp = _planes_ref(A), _planes_ref(B)
    ldb = K + pad
    bstride = (N + 1) * ldb

    def call(S, L):
        lib, st = L.lib(), L.stream()
        Api = S.inp("a_planes", Ap.reshape(3 * M, K), ld=K + pad)
        Bw = torch.zeros(3, N + 1, K, dtype=BF); Bw[:, :N] = Bp                    # plane stride (N + 1) * ldb
        Bpi = S.inp("b_planes", Bw.reshape(3 * (N + 1), K), ld=ldb)
        Bd = S.inp("b_planes_dense", Bp.reshape(3 * N, K), ld=ldb)
        Ai = S.inp("A", A, ld=K + pad + 4, col_off=4, misalign=16)
        outs, ref = {}, {}
        if epi == "bias":
            o = S.out("C_basic", M, N, F32, ld=N + padc)
            L.check(lib.gg_gemm_nt_split3(Api.ptr, Api.ld, Bd.ptr, ldb, o.ptr, o.ld, M, N, K, S.inp("bias0", bias).ptr, st), "gg_gemm_nt_split3")
            outs["C_basic"] = o; ref["C_basic"] = z + bias.double()
        for form in ("ex", "af32"):
            a = L.Split3Args()
            a.a_planes, a.lda, a.M, a.N, a.K = Api.ptr, Api.ld, M, N, K
            a.b_planes, a.ldb = (Bd.ptr, ldb) if form == "ex" else (Bpi.ptr, ldb)
            if epi != "planes_out":
                o = S.out("C_" + form, M, N, F32, ld=N + padc); a.C, a.ldc = o.ptr, o.ld
                outs["C_" + form] = o
            a.bias = S.inp("bias", bias, misalign=16).ptr if epi != "dact" else None
            ref["C_" + form] = z + bias.double()
            if epi == "bias_gelu_preact":
                pre = S.out("preact_" + form, M, N, F32, ld=N + padc); a.act, a.preact = 1, pre.ptr
                outs["preact_" + form] = pre; ref["preact_" + form] = z + bias.double(); ref["C_" + form] = F.gelu(z + bias.double())
            elif epi == "rowscale_residual":
                r = S.inp("residual", res, ld=N + 12)
                a.rowscale, a.rows_per_scale, a.residual, a.ldr = S.inp("rowscale", rs).ptr, rps, r.ptr, r.ld
                ref["C_" + form] = res.double() + rs_rows * (z + bias.double())
            elif epi == "dact":
                a.ldc = a.ldc or N + padc
                a.dact_preact, a.dact = S.inp("dact_preact", h, ld=N + padc).ptr, 1
                ref["C_" + form] = z * _gelu_grad(h)
            elif epi == "planes_out":
                cp = S.out("c_planes_" + form, 3 * M, N, BF, ld=N + 8); a.c_planes, a.ldp = cp.ptr, cp.ld
                outs["c_planes_" + form] = cp
            if form == "ex":
                L.check(lib.gg_gemm_nt_split3_ex(C.byref(a), st), "gg_gemm_nt_split3_ex")
            else:
                L.check(lib.gg_gemm_nt_split3_af32(C.byref(a), Ai.ptr, Ai.ld, bstride, st), "gg_gemm_nt_split3_af32")

        def check(v):
            for k in v:
                if k.startswith("c_planes"):
                    got = v[k].double().view(3, M, N).sum(0)
                    assert rel_l2(got, z + bias.double()) < 1e-6, k
                else:
                    e = rel_l2(v[k], ref[k])
                    assert e < (1e-6 if epi == "bias" else 1e-5), (k, e)
            for k in [k for k in v if k.endswith("_ex")]:
                G.assert_bit_identical(v[k], v[k[:-3] + "_af32"], k + " vs af32")
        return outs, check
    run_guarded(call)


@case("gg_gemm_nt_split3_af32_stats", "gg_gemm_nt_split3_af32_pro")
@pytest.mark.parametrize("M,N,K,act", [(300, 96, 384, 1), (129, 200, 416, 1), (1, 8, 384, 0), (257, 129, 1024, 2)])
def test_split3_gemm_batchnorm_forms(M, N, K, act):
    """colstats of the result (test_split3_gemm_batchnorm_partials) and the BatchNorm + activation prologue (test_split3_gemm_batchnorm_act_prologue):
    rel-L2 < 1e-6 / 1e-5 against fp64; column sums at the bf16 GEMM test's rtol 1e-3."""
    y = rnd(M, K, seed=41); W = rnd(N, K, seed=42, scale=K ** -0.5)
    mean, rstd = rnd(K, seed=43, scale=0.3), torch.rand(K, generator=torch.Generator().manual_seed(44)) + 0.5
    gamma, beta = rnd(K, seed=45) * 0.5 + 1.0, rnd(K, seed=46, scale=0.2)
    u = (y.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()
    act_u = F.gelu(u) if act == 1 else (u * torch.sigmoid(1.702 * u) if act == 2 else u)
    Wp = _planes_ref(W)

    def call(S, L):
        lib, st = L.lib(), L.stream()
        rows = lib.gg_gemm_colstats_rows(M)
        Yi = S.inp("A", y, ld=K + 12, col_off=4)
        Bi = S.inp("b_planes", Wp.reshape(3 * N, K), ld=K + 8)
        outs = {}
        for form in ("stats", "pro"):
            a = L.Split3Args()
            o = S.out("C_" + form, M, N, F32, ld=N + 3); cs = S.out("colstats_" + form, rows, 2 * N, F32)
            a.b_planes, a.ldb, a.M, a.N, a.K, a.C, a.ldc = Bi.ptr, Bi.ld, M, N, K, o.ptr, o.ld
            if form == "stats":
                L.check(lib.gg_gemm_nt_split3_af32_stats(C.byref(a), Yi.ptr, Yi.ld, 0, cs.ptr, st), "af32_stats")
            else:
                L.check(lib.gg_gemm_nt_split3_af32_pro(C.byref(a), Yi.ptr, Yi.ld, 0, S.inp("bn_stat", torch.cat([mean, rstd])).ptr, S.inp("gamma", gamma).ptr,
                                                       S.inp("beta", beta).ptr, act, cs.ptr, st), "af32_pro")
            outs["C_" + form] = o; outs["colstats_" + form] = cs

        def check(v):
            assert rel_l2(v["C_stats"], y.double() @ W.double().t()) < 1e-6
            assert rel_l2(v["C_pro"], act_u @ W.double().t()) < 1e-5
            for form in ("stats", "pro"):
                raw = v["C_" + form].double(); s = v["colstats_" + form].double().view(-1, 2, N).sum(0)
                close(s[0], raw.sum(0), 1e-3, 0.3, "colsum " + form); close(s[1], (raw * raw).sum(0), 1e-3, 0.3, "colsumsq " + form)
        return outs, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- weight-gradient (tn) forms
TN_SHAPES = [(256, 64, 64, 0, 0), (257, 72, 56, 8, 0), (255, 8, 8, 24, 7), (1, 8, 8, 8, 0), (1100, 96, 40, 8, 64), (5003, 48, 32, 24, 49)]


@case("gg_gemm_tn", "gg_gemm_tn_f32", "gg_gemm_tn_split3", "gg_gemm_tn_bn", "gg_gemm_tn_bn_f32", "gg_splitk_reduce")
@pytest.mark.parametrize("form", ["bf16", "f32", "split3", "bn_bf16", "bn_f32"])
@pytest.mark.parametrize("M,N,K,pad,rps", TN_SHAPES)
def test_gemm_tn_forms(M, N, K, pad, rps, form):
    """partials [splits][N][K] with splits from the matching *_splits function, reduced by gg_splitk_reduce.  Tolerances: test_gemm_tn_weight_gradient /
    test_gemm_tn_with_batchnorm_apply_on_load (bf16: rtol 1e-4 / 2e-3, atol 2e-2), test_split3_weight_gradient_gemm (rel-L2 < 2e-6 against fp64) and
    test_f32_gemm_tn_with_batchnorm_apply_on_load (f32: 2e-5 of the largest magnitude)."""
    bn = form.startswith("bn")
    dt = BF if form in ("bf16", "bn_bf16") else F32
    dY, X = rnd(M, N, seed=51, scale=0.1, dtype=dt), rnd(M, K, seed=52, dtype=dt)
    yv, coef = rnd(M, N, seed=53, dtype=dt), rnd(3, N, seed=54, scale=0.5)
    rs = (torch.rand((M + max(rps, 1) - 1) // max(rps, 1), generator=torch.Generator().manual_seed(55)) > 0.3).float() * 1.25 if rps and not bn else None
    dy_eff = (coef[0].double() * dY.double() + coef[1].double() * yv.double() + coef[2].double()) if bn else dY.double()
    if rs is not None:
        dy_eff = dy_eff * rs.double().repeat_interleave(rps)[:M, None]
    if dt == BF and (bn or rs is not None):
        dy_eff = dy_eff.float().to(BF).double()                 # the bf16 kernels round the formed dY to bf16 for the MFMA (the parity tests' reference does the same)
    ref = dy_eff.t() @ X.double()

    def call(S, L):
        lib, st = L.lib(), L.stream()
        splits = {"bf16": lib.gg_gemm_tn_splits, "bn_bf16": lib.gg_gemm_tn_splits, "f32": lib.gg_gemm_tn_f32_splits, "bn_f32": lib.gg_gemm_tn_f32_splits,
                  "split3": lib.gg_gemm_tn_split3_splits}[form](M, N, K)
        assert splits >= 1
        dYi, Xi = S.inp("dY", dY.to(dt), ld=N + pad, misalign=16), S.inp("X", X.to(dt), ld=K + pad + 8, col_off=8)
        P = S.out("partials", splits * N, K, F32)
        r = S.inp("rowscale", rs).ptr if rs is not None else None
        if form == "bf16":
            L.check(lib.gg_gemm_tn(dYi.ptr, dYi.ld, Xi.ptr, Xi.ld, M, N, K, r, rps if rs is not None else 0, P.ptr, splits, st), form)
        elif form == "f32":
            L.check(lib.gg_gemm_tn_f32(dYi.ptr, dYi.ld, Xi.ptr, Xi.ld, M, N, K, r, rps if rs is not None else 0, P.ptr, splits, st), form)
        elif form == "split3":
            L.check(lib.gg_gemm_tn_split3(dYi.ptr, dYi.ld, Xi.ptr, Xi.ld, M, N, K, r, rps if rs is not None else 0, P.ptr, splits, st), form)
        else:
            yi, ci = S.inp("y", yv.to(dt), ld=N + pad, misalign=16), S.inp("coef", coef)
            fn = lib.gg_gemm_tn_bn if form == "bn_bf16" else lib.gg_gemm_tn_bn_f32
            L.check(fn(dYi.ptr, yi.ptr, dYi.ld, ci.ptr, Xi.ptr, Xi.ld, M, N, K, P.ptr, splits, st), form)
        torch.cuda.synchronize()
        Pi = S.inp("partials_in", P.view.cpu())
        o = S.out("dW", 1, N * K, F32)
        L.check(lib.gg_splitk_reduce(Pi.ptr, o.ptr, N * K, splits, 0, L.f32(1.0), st), "gg_splitk_reduce")

        def check(v):
            got = v["dW"].view(N, K)
            if dt == BF:
                close(got, ref, 2e-3 if bn else 1e-4, 2e-2, form)
            elif form == "split3":
                assert rel_l2(got, ref) < 2e-6, (form, rel_l2(got, ref))
            else:
                assert rel_max(got, ref) < 2e-5, (form, rel_max(got, ref))
        return {"partials": P, "dW": o}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- LayerNorm
def _ln_ref(x, gamma, beta, eps):
    x = x.double()
    mu = x.mean(1, keepdim=True); var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mu) * rstd * gamma.double() + beta.double(), mu[:, 0], rstd[:, 0]


@case("gg_layernorm_fwd_split3", "gg_layernorm_fwd_bn_split3")
@pytest.mark.parametrize("M,Cc", [(64, 64), (65, 192), (1, 8), (333, 40), (77, 576), (127, 320)])
def test_layernorm_split3(M, Cc):
    """f32 LayerNorm whose result leaves as three bf16 planes: the planes sum to the fp64 LayerNorm's f32 result to 24 bits (test_split3_gemm_is_fp32_accurate's
    criterion for gg_split3_bf16: residual < 2^-22 of the largest magnitude, here on top of the f32 LayerNorm's own rounding, which test_layernorm bounds at
    1e-5 absolute for f32 storage -- both are asserted: planes vs the kernel's own f32 arithmetic through mean / rstd, and vs fp64)."""
    eps = 1e-5
    x, gamma, beta = rnd(M, Cc, seed=M + Cc), rnd(Cc, seed=61) * 0.2 + 1.0, rnd(Cc, seed=62, scale=0.1)
    bn_stat = torch.cat([rnd(Cc, seed=63, scale=0.3), torch.rand(Cc, generator=torch.Generator().manual_seed(64)) + 0.5])
    bg, bb = rnd(Cc, seed=65) * 0.3 + 1.0, rnd(Cc, seed=66, scale=0.2)
    xbn = ((x.double() - bn_stat[:Cc].double()) * bn_stat[Cc:].double() * bg.double() + bb.double())

    def call(S, L):
        lib, st = L.lib(), L.stream()
        xi, gi, bi = S.inp("x", x, misalign=16 if Cc % 64 else 0), S.inp("gamma", gamma), S.inp("beta", beta, misalign=16)
        o = {"planes": S.out("planes", 3 * M, Cc, BF), "mean": S.out("mean", 1, M, F32), "rstd": S.out("rstd", 1, M, F32),
             "planes_bn": S.out("planes_bn", 3 * M, Cc, BF), "xout": S.out("xout", M, Cc, F32), "mean_bn": S.out("mean_bn", 1, M, F32),
             "rstd_bn": S.out("rstd_bn", 1, M, F32)}
        L.check(lib.gg_layernorm_fwd_split3(xi.ptr, gi.ptr, bi.ptr, M, Cc, L.f32(eps), o["planes"].ptr, o["mean"].ptr, o["rstd"].ptr, st), "ln_split3")
        L.check(lib.gg_layernorm_fwd_bn_split3(xi.ptr, S.inp("bn_stat", bn_stat).ptr, S.inp("bn_gamma", bg).ptr, S.inp("bn_beta", bb).ptr, o["xout"].ptr, gi.ptr, bi.ptr,
                                               M, Cc, L.f32(eps), o["planes_bn"].ptr, o["mean_bn"].ptr, o["rstd_bn"].ptr, st), "ln_bn_split3")

        def check(v):
            for tag, src in (("", x.double()), ("_bn", xbn)):
                ref, mu, rstd = _ln_ref(src, gamma, beta, eps)
                got = v["planes" + tag].double().view(3, M, Cc).sum(0)
                scale = float(ref.abs().max())
                # the f32 result the planes must carry: the kernel's own statistics applied in f32 (what an f32 LayerNorm stores)
                src32 = v["xout"] if tag else x
                own = ((src32 - v["mean" + tag].view(M, 1)) * v["rstd" + tag].view(M, 1) * gamma + beta).double()
                assert float((got - own).abs().max()) < 2 ** -22 * scale + 2 ** -21 * scale, (tag, float((got - own).abs().max()))   # + the f32 expression's own 2-3 roundings
                close(got, ref, 0, 1e-5 * max(1.0, scale), "ln planes vs fp64" + tag)
                close(v["mean" + tag][0], mu, 1e-5, 1e-5, "mean" + tag); close(v["rstd" + tag][0], rstd, 1e-5, 1e-5, "rstd" + tag)
            close(v["xout"], xbn, 1e-6, 1e-5, "xout")
        return o, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- hierarchical head
@case("gg_pe_add_f32", "gg_mha_q0_fwd", "gg_mha_q0_bwd")
@pytest.mark.parametrize("N,V,Cc,H,mask", [(1, 1, 64, 16, None), (3, 4, 64, 16, None), (2, 4, 128, 16, "one"), (5, 7, 48, 4, "drop"), (1, 2, 8, 1, None), (4, 1, 32, 2, "drop")])
def test_mha_query0(N, V, Cc, H, mask):
    """nn.MultiheadAttention's attention of query token 0 (the projections are GEMMs): fp64 torch single-query attention with autograd.  fp32 kernel:
    rtol = atol = 1e-5 (a softmax over at most 7 keys and a dot product of C / H terms: a few f32 roundings of O(1) values).  `one`: a probability mask that
    hides all but one view; `drop`: dropout scales keep / (1 - p)."""
    d = Cc // H
    qkv = rnd(N * V, 3 * Cc, seed=N * 10 + V)
    do0 = rnd(N, Cc, seed=71)
    g = torch.Generator().manual_seed(72)
    pm = None
    if mask == "one":
        pm = torch.zeros(N, H, V); pm[:, :, V - 1] = 1.0
    elif mask == "drop":
        pm = (torch.rand(N, H, V, generator=g) > 0.25).float() / 0.75
    x, pe = rnd(N, V, Cc, seed=73), rnd(N + 2, Cc, seed=74)
    em = (torch.rand(N, V, Cc, generator=g) > 0.1).float() / 0.9 if mask else None

    q = qkv.double().clone().requires_grad_(True)
    t = q.view(N, V, 3, H, d)
    s = torch.einsum("nhd,nvhd->nhv", t[:, 0, 0], t[:, :, 1]) / math.sqrt(d)
    p = torch.softmax(s, -1)
    pd = p * pm.double() if pm is not None else p
    o_ref = torch.einsum("nhv,nvhd->nhd", pd, t[:, :, 2]).reshape(N, Cc)
    (o_ref * do0.double()).sum().backward()

    def call(S, L):
        lib, st = L.lib(), L.stream()
        qi = S.inp("qkv", qkv, misalign=16)
        pmi = S.inp("pmask", pm.reshape(N, H * V)) if pm is not None else None
        o0, probs = S.out("o0", N, Cc, F32), S.out("probs", N, H * V, F32)
        L.check(lib.gg_mha_q0_fwd(qi.ptr, pmi.ptr if pmi else None, o0.ptr, probs.ptr, N, V, Cc, H, st), "gg_mha_q0_fwd")
        torch.cuda.synchronize()
        pri = S.inp("probs_in", probs.view.cpu(), misalign=16)
        dq = S.out("dqkv", N * V, 3 * Cc, F32)
        L.check(lib.gg_mha_q0_bwd(qi.ptr, pri.ptr, pmi.ptr if pmi else None, S.inp("do0", do0).ptr, dq.ptr, N, V, Cc, H, st), "gg_mha_q0_bwd")
        xi, pei = S.inp("x", x.reshape(N * V, Cc)), S.inp("pe", pe, misalign=16)
        emi = S.inp("mask", em.reshape(N * V, Cc)) if em is not None else None
        po = S.out("pe_out", N * V, Cc, F32)
        L.check(lib.gg_pe_add_f32(xi.ptr, pei.ptr, emi.ptr if emi else None, po.ptr, N, V, Cc, st), "gg_pe_add_f32")

        def check(v):
            close(v["o0"], o_ref.detach(), 1e-5, 1e-5, "o0")
            close(v["probs"].view(N, H, V), p.detach(), 1e-5, 1e-5, "probs")
            close(v["dqkv"], q.grad, 1e-5, 1e-5, "dqkv")
            pref = x + pe[:N, None, :]                           # position = batch index (models/layers/positional_encoder.py:44)
            close(v["pe_out"].view(N, V, Cc), pref * em if em is not None else pref, 1e-6, 1e-6, "pe_add")
        return {"o0": o0, "probs": probs, "dqkv": dq, "pe_out": po}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- attention
def _attn_geometry(nh, D, ws, map_hw, batch, linearN, layout):
    if ws:
        N, nw = ws * ws, batch * (map_hw // ws) ** 2
    else:
        N, nw = linearN, batch
    if layout == "interleaved":
        hs, offs = 3 * D, (0, D, 2 * D)                        # TinyViT: per-head [q|k|v]
    else:
        hs, offs = D, (0, nh * D, 2 * nh * D)                  # CLIP: [q|k|v] blocks of all heads
    return N, nw, hs, offs


# (nh, D, ws, map_hw, batch, linearN, layout, pad): 7 x 7 / 12 x 12 / 14 x 14 windows at head dim 32 (fp32: the split-product kernels of attention_split.h), 16 x 16 (256 tokens:
# the largest single-pass window), 18 x 18 (324 tokens: two-pass backward, ds_scratch), several windows per side (map 18 / ws 9, map 42 / ws 7, map 14 / ws 7),
# linear 1 / 17 / 50 / 257 tokens at head dim 64; both [q|k|v] layouts; ld, ldo, lddo beyond the packed width by 8 and by 24
FLASH_SHAPES = [(2, 32, 7, 7, 1, 0, "interleaved", 0), (2, 32, 7, 14, 2, 0, "interleaved", 8), (3, 32, 7, 42, 1, 0, "interleaved", 24), (1, 32, 12, 12, 2, 0, "interleaved", 8),
                (2, 32, 14, 14, 1, 0, "blocks", 24), (1, 32, 16, 16, 1, 0, "interleaved", 8), (1, 32, 18, 18, 1, 0, "interleaved", 8), (2, 32, 9, 18, 1, 0, "blocks", 8),
                (1, 64, 0, 0, 2, 1, "blocks", 8), (2, 64, 0, 0, 2, 17, "blocks", 24), (3, 64, 0, 0, 1, 50, "blocks", 8), (1, 64, 0, 0, 1, 257, "interleaved", 8)]


@case("gg_attention_flash_fwd", "gg_attention_flash_bwd")
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("nh,D,ws,map_hw,batch,linearN,layout,pad", FLASH_SHAPES)
def test_flash_attention(dtype, nh, D, ws, map_hw, batch, linearN, layout, pad):
    """gg_attention_flash_fwd / _bwd in the three storage types (2 = fp16: forward only).  Reference and tolerances: test_flash_attention_forward_backward
    (f32: 2e-5, dbias 5e-5; bf16: 1.5e-2, dbias 2e-2) and test_clip_attention_fwd_fp16 (2e-3).  qkv is a column slice of a wider buffer; lse, dbias_scratch and
    ds_scratch have exactly the sizes the header / capacity functions give.  dbias is ACCUMULATED (starts from ones).  It is the one output exempt from
    bit-identity, with and without dbias_scratch: a workgroup sums its bins with float atomics in LDS (atomicAdd on dbt in attention_flash.hip's backward kernels
    and attention_split.h), and without the scratch the windows' sums also meet in atomicAdd(&p.dbias[...]); dbias_scratch only makes the second, cross-window
    stage ordered (test_flash_attention_forward_backward says the same).  Tolerance: 1e-5 of the largest magnitude, as tests/test_gpu_recompute.py."""
    from tests.test_gpu_precision import _attn_ref as flash_ref, relerr
    dt = {0: BF, 1: F32, 2: F16}[dtype]
    N, nw, hs, (q_off, k_off, v_off) = _attn_geometry(nh, D, ws, map_hw, batch, linearN, layout)
    tokens, width = nw * N, 3 * nh * D
    qkv, dout = rnd(tokens, width, seed=31, dtype=dt), rnd(tokens, nh * D, seed=32, dtype=dt)
    table = rnd(nh, ws * ws, seed=30, scale=0.5) if ws else None
    ref, dq_ref, dt_ref = flash_ref(qkv, nh, D, N, nw, ws, map_hw, table, q_off, k_off, v_off, hs, dout)
    tol = {0: 1.5e-2, 1: 2e-5, 2: 2e-3}[dtype]
    # row log-sum-exp of scale * q.k (+ bias) on the same token layout as the reference of the outputs
    if ws:
        idx = torch.arange(tokens).view(nw // (map_hw // ws) ** 2, map_hw // ws, ws, map_hw // ws, ws).permute(0, 1, 3, 2, 4).reshape(nw, N)
        yy, xx = torch.arange(N) // ws, torch.arange(N) % ws
        bidx = (yy[:, None] - yy[None, :]).abs() * ws + (xx[:, None] - xx[None, :]).abs()
    else:
        idx = torch.arange(tokens).view(nw, N)
    lse_ref = torch.zeros(tokens, nh, dtype=torch.float64)
    for h in range(nh):
        sc = qkv[:, q_off + h * hs:q_off + h * hs + D].double()[idx] @ qkv[:, k_off + h * hs:k_off + h * hs + D].double()[idx].transpose(1, 2) * D ** -0.5
        if ws:
            sc = sc + table[h].double()[bidx]
        lse_ref[idx.reshape(-1), h] = torch.logsumexp(sc, -1).reshape(-1)

    def run(scratch):
        def call(S, L):
            lib, st = L.lib(), L.stream()
            a = L.AttnArgs()
            qi = S.inp("qkv", qkv.to(dt), ld=width + pad + 8, col_off=8)
            a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, q_off, k_off, v_off, hs, D
            a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w = nh, nw, N, ws, map_hw, map_hw
            a.scale = D ** -0.5
            a.bias_table = S.inp("bias_table", table).ptr if ws else None
            out, lse = S.out("out", tokens, nh * D, dt, ld=nh * D + pad), S.out("lse", tokens, nh, F32)
            a.out, a.ldo, a.lse = out.ptr, out.ld, lse.ptr
            L.check(lib.gg_attention_flash_fwd(C.byref(a), dtype, st), "gg_attention_flash_fwd")
            outs = {"out": out, "lse": lse}
            if dtype != 2:
                torch.cuda.synchronize()
                oi, li = S.inp("out_in", out.view.cpu(), ld=out.ld), S.inp("lse_in", lse.view.cpu())
                di = S.inp("dout", dout.to(dt), ld=nh * D + (24 if pad else 0))
                dq = S.out("dqkv", tokens, width, dt, ld=qi.ld, col_off=8)             # "same layout as qkv"
                a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv = oi.ptr, oi.ld, li.ptr, di.ptr, di.ld, dq.ptr
                outs["dqkv"] = dq
                if ws:
                    db = S.out("dbias", nh, ws * ws, F32, init=torch.ones(nh, ws * ws))
                    a.dbias = db.ptr
                    outs["dbias"] = db
                    if scratch:
                        a.dbias_scratch = S.scratch("dbias_scratch", 4 * lib.gg_attention_flash_dbias_rows(nw, N) * nh * ws * ws, row_bytes=4 * nh * ws * ws).ptr
                if scratch and not lib.gg_attention_flash_single_pass(N, D, ws, int(bool(ws))):
                    a.ds_scratch = S.scratch("ds_scratch", 4 * lib.gg_attention_flash_ds_scratch_floats(nw, nh, N), row_bytes=4 * 16 * ((N + 15) // 16)).ptr
                L.check(lib.gg_attention_flash_bwd(C.byref(a), dtype, st), "gg_attention_flash_bwd")

            def check(v):
                close(v["out"], ref, tol, tol, f"flash fwd dtype {dtype}")
                lt = {0: 1.5e-2, 1: 2e-5, 2: 1e-3}[dtype]     # lse at the forward's tolerance (fp16: test_clip_attention_fwd_fp16's 1e-3 for lse)
                close(v["lse"], lse_ref, lt, lt, f"flash lse dtype {dtype}")
                if dtype == 2:
                    return
                assert relerr(v["dqkv"], dq_ref) < tol, relerr(v["dqkv"], dq_ref)
                if ws:
                    e = relerr(v["dbias"] - 1.0, dt_ref)
                    assert e < (5e-5 if dtype == 1 else 2e-2), e
            return outs, check
        return call
    run_guarded(run(True), atomic=("dbias",))
    if ws and dtype != 2:
        run_guarded(run(False), atomic=("dbias",))


WIN_SHAPES = [(2, 7, 7, 1, 0), (2, 7, 14, 3, 8), (3, 7, 42, 1, 24), (1, 12, 12, 2, 8), (2, 14, 14, 1, 8), (1, 16, 16, 1, 24), (2, 9, 18, 1, 8)]


@case("gg_attention_fwd", "gg_attention_bwd", "gg_attention_expand_bias")
@pytest.mark.parametrize("nh,ws,map_hw,batch,pad", WIN_SHAPES)
def test_window_attention_bf16(nh, ws, map_hw, batch, pad):
    """gg_attention_expand_bias + gg_attention_fwd / _bwd (bf16, head dim 32, both bias forms given as the header asks).  Tolerances of
    test_window_attention_fwd_bwd: forward 2e-2, dqkv 3e-2, dbias rtol 3e-2 / atol 5e-2.  dbias_scratch: f32 [(num_windows + 64) * num_heads * ws * ws] (header)."""
    from tests.test_gpu_precision import _attn_ref as flash_ref
    D = 32
    N, nw, hs, (q_off, k_off, v_off) = _attn_geometry(nh, D, ws, map_hw, batch, 0, "interleaved")
    tokens, width = nw * N, 3 * nh * D
    qkv, dout, table = rnd(tokens, width, seed=60, dtype=BF), rnd(tokens, nh * D, seed=62, dtype=BF), rnd(nh, ws * ws, seed=61, scale=0.5)
    ref, dq_ref, dt_ref = flash_ref(qkv, nh, D, N, nw, ws, map_hw, table, q_off, k_off, v_off, hs, dout)
    scale = D ** -0.5

    def run(scratch):
        def call(S, L):
            lib, st = L.lib(), L.stream()
            Np = lib.gg_attention_padded_tokens(N)
            ti = S.inp("bias_table", table, misalign=16)
            full = S.out("bias_full", nh * Np, Np, BF)
            L.check(lib.gg_attention_expand_bias(ti.ptr, nh, ws, L.f32(scale), full.ptr, st), "gg_attention_expand_bias")
            torch.cuda.synchronize()
            fi = S.inp("bias_full_in", full.view.cpu())
            a = L.AttnArgs()
            qi = S.inp("qkv", qkv.to(BF), ld=width + pad + 8, col_off=8)
            a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, q_off, k_off, v_off, hs, D
            a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w = nh, nw, N, ws, map_hw, map_hw
            a.scale, a.bias, a.bias_table = scale, fi.ptr, ti.ptr
            out, lse = S.out("out", tokens, nh * D, BF, ld=nh * D + pad), S.out("lse", tokens, nh, F32)
            a.out, a.ldo, a.lse = out.ptr, out.ld, lse.ptr
            L.check(lib.gg_attention_fwd(C.byref(a), st), "gg_attention_fwd")
            torch.cuda.synchronize()
            oi, li = S.inp("out_in", out.view.cpu(), ld=out.ld), S.inp("lse_in", lse.view.cpu())
            di = S.inp("dout", dout.to(BF), ld=nh * D + (24 if pad else 0))
            dq = S.out("dqkv", tokens, width, BF, ld=qi.ld, col_off=8)
            db = S.out("dbias", nh, ws * ws, F32, init=torch.ones(nh, ws * ws))
            a.out, a.ldo, a.lse, a.dout, a.lddo, a.dqkv, a.dbias = oi.ptr, oi.ld, li.ptr, di.ptr, di.ld, dq.ptr, db.ptr
            if scratch:
                a.dbias_scratch = S.scratch("dbias_scratch", 4 * (nw + 64) * nh * ws * ws, row_bytes=4 * nh * ws * ws).ptr
            L.check(lib.gg_attention_bwd(C.byref(a), st), "gg_attention_bwd")

            def check(v):
                f = v["bias_full"].float().view(nh, Np, Np)
                yy, xx = torch.arange(N) // ws, torch.arange(N) % ws
                bidx = (yy[:, None] - yy[None, :]).abs() * ws + (xx[:, None] - xx[None, :]).abs()
                assert torch.equal(f[:, :N, :N], (table[:, bidx] * (1.0 / torch.tensor(scale, dtype=F32))).to(BF).float())
                assert bool(torch.isinf(f[:, :, N:]).all())                                     # -inf for padded keys
                close(v["out"], ref, 2e-2, 2e-2, "attn fwd"); close(v["dqkv"], dq_ref, 3e-2, 3e-2, "attn dqkv"); close(v["dbias"] - 1.0, dt_ref, 3e-2, 5e-2, "attn dbias")
            return {"bias_full": full, "out": out, "lse": lse, "dqkv": dq, "dbias": db}, check
        return call
    # dbias: float atomics in LDS inside a workgroup (atomicAdd(&dbias_s[...]) in attention.hip, dbt in attention_split.h) with or without the scratch, plus
    # atomicAdd(&p.dbias[...]) across windows without it: the one exemption from bit-identity, at 1e-5 of the largest magnitude
    run_guarded(run(True), atomic=("dbias",))
    run_guarded(run(False), atomic=("dbias",))


@case("gg_attention_fwd", "gg_attention_fwd_f16")
@pytest.mark.parametrize("dt", [BF, F16])
@pytest.mark.parametrize("B,T,nh,hd,pad", [(2, 50, 3, 64, 8), (1, 1, 1, 64, 8), (2, 17, 2, 64, 24), (1, 256, 1, 64, 0), (1, 257, 1, 64, 8), (3, 49, 2, 32, 8)])
def test_linear_attention_forward(dt, B, T, nh, hd, pad):
    """CLIP MHSA through gg_attention_fwd (bf16: test_clip_attention_fwd, 2e-2) and gg_attention_fwd_f16 (test_clip_attention_fwd_fp16: 2e-3, lse 1e-3); 257 tokens
    forward to the online-softmax kernels."""
    from tests.test_gpu_precision import _attn_ref as flash_ref
    Dm = nh * hd
    qkv = rnd(B * T, 3 * Dm, seed=63, dtype=dt)
    ref = flash_ref(qkv, nh, hd, T, B, 0, 0, None, 0, Dm, 2 * Dm, hd)
    tol = 2e-2 if dt == BF else 2e-3

    def call(S, L):
        a = L.AttnArgs()
        qi = S.inp("qkv", qkv.to(dt), ld=3 * Dm + pad + 8, col_off=8, misalign=16)
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qi.ptr, qi.ld, 0, Dm, 2 * Dm, hd, hd
        a.num_heads, a.num_windows, a.tokens_per_window, a.scale = nh, B, T, hd ** -0.5
        out, lse = S.out("out", B * T, Dm, dt, ld=Dm + pad), S.out("lse", B * T, nh, F32)
        a.out, a.ldo, a.lse = out.ptr, out.ld, lse.ptr
        fn = L.lib().gg_attention_fwd if dt == BF else L.lib().gg_attention_fwd_f16
        L.check(fn(C.byref(a), L.stream()), "attention fwd")

        def check(v):
            close(v["out"], ref, tol, tol, "linear attn")
            q = qkv[:, :Dm].double().view(B, T, nh, hd).permute(0, 2, 1, 3); k = qkv[:, Dm:2 * Dm].double().view(B, T, nh, hd).permute(0, 2, 1, 3)
            lse_ref = torch.logsumexp((q @ k.transpose(-1, -2)) * hd ** -0.5, dim=-1).permute(0, 2, 1).reshape(B * T, nh)
            close(v["lse"], lse_ref, 1e-3 if dt == F16 else 2e-2, 1e-3 if dt == F16 else 2e-2, "lse")
        return {"out": out, "lse": lse}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- LayerNorm, pooling, column sums
@case("gg_layernorm_fwd", "gg_layernorm_bwd", "gg_layernorm_bwd_colsum", "gg_layernorm_fwd_f16")
@pytest.mark.parametrize("dt", [BF, F32, F16])
@pytest.mark.parametrize("M,Cc", [(64, 64), (65, 192), (1, 8), (301, 160), (77, 576), (33, 1024)])
def test_layernorm_forward_backward(dt, M, Cc):
    """test_layernorm's reference (torch layer_norm + autograd) and tolerances: forward / dx 1e-4 (f32), 1e-2 / 2e-2 (bf16), mean 1e-5, dgamma / dbeta rtol 1e-2 atol 0.3
    (ACCUMULATED: they start from ones); fp16 forward at test_clip_attention_fwd_fp16's fp16 tolerance 2e-3 of O(1) values.  gg_layernorm_bwd_colsum's dx against
    gg_layernorm_bwd's at test_layernorm_bwd_with_batchnorm_column_sums' 1e-6 / 8e-3; its part buffer is (gg_layernorm_bwd_colsum_rows(M) + 64) rows (header)."""
    x = (rnd(M, Cc, seed=40, scale=1.5) + 0.3).to(BF).float()
    gamma, beta = 1 + 0.2 * rnd(Cc, seed=41), 0.1 * rnd(Cc, seed=42)
    dout, dres = rnd(M, Cc, seed=43, dtype=dt), rnd(M, Cc, seed=44, dtype=dt)
    xr, g_, b_ = x.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    ref = F.layer_norm(xr, (Cc,), g_, b_, 1e-5)
    ref.backward(dout.double())
    f32 = dt == F32

    def call(S, L):
        lib, st = L.lib(), L.stream()
        xi, gi, bi = S.inp("x", x.to(dt), misalign=16), S.inp("gamma", gamma), S.inp("beta", beta, misalign=16)
        out = S.out("out", M, Cc, dt)
        if dt == F16:
            L.check(lib.gg_layernorm_fwd_f16(xi.ptr, gi.ptr, bi.ptr, M, Cc, L.f32(1e-5), out.ptr, st), "gg_layernorm_fwd_f16")
            return {"out": out}, lambda v: close(v["out"], ref.detach(), 2e-3, 2e-3, "ln fwd fp16")
        mean, rstd = S.out("mean", 1, M, F32), S.out("rstd", 1, M, F32)
        L.check(lib.gg_layernorm_fwd(xi.ptr, int(f32), gi.ptr, bi.ptr, M, Cc, L.f32(1e-5), out.ptr, int(f32), mean.ptr, rstd.ptr, st), "gg_layernorm_fwd")
        torch.cuda.synchronize()
        mi, ri = S.inp("mean_in", mean.view.cpu()), S.inp("rstd_in", rstd.view.cpu())
        di, dri = S.inp("dout", dout.to(dt)), S.inp("dres", dres.to(dt), misalign=16)
        dx, dg, db = S.out("dx", M, Cc, dt), S.out("dgamma", 1, Cc, F32, init=torch.ones(Cc)), S.out("dbeta", 1, Cc, F32, init=torch.ones(Cc))
        sc = S.scratch("scratch", 4 * lib.gg_layernorm_bwd_scratch_floats(M, Cc), row_bytes=8 * Cc)
        L.check(lib.gg_layernorm_bwd(di.ptr, xi.ptr, int(f32), mi.ptr, ri.ptr, gi.ptr, M, Cc, dri.ptr, dx.ptr, sc.ptr, dg.ptr, db.ptr, 1, st), "gg_layernorm_bwd")
        outs = {"out": out, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": dg, "dbeta": db}
        if Cc <= 640:
            dx2 = S.out("dx_colsum", M, Cc, dt)
            part = S.scratch("part", 4 * (lib.gg_layernorm_bwd_colsum_rows(M) + 64) * 2 * Cc, row_bytes=8 * Cc)
            L.check(lib.gg_layernorm_bwd_colsum(di.ptr, xi.ptr, int(f32), mi.ptr, ri.ptr, gi.ptr, M, Cc, dri.ptr, dx2.ptr, part.ptr, st), "gg_layernorm_bwd_colsum")
            outs["dx_colsum"] = dx2

        def check(v):
            t1, t2 = (1e-4, 1e-4) if f32 else (1e-2, 2e-2)
            close(v["out"], ref.detach(), t1, t1, "ln fwd"); close(v["mean"][0], x.double().mean(1), 1e-5, 1e-5, "ln mean")
            close(v["dx"], xr.grad + dres.double(), t2, t2, "ln dx")
            close(v["dgamma"][0] - 1.0, g_.grad, 1e-2, 0.3, "ln dgamma"); close(v["dbeta"][0] - 1.0, b_.grad, 1e-2, 0.3, "ln dbeta")
            if "dx_colsum" in v:
                close(v["dx_colsum"], v["dx"].double(), 1e-6 if f32 else 8e-3, 1e-6 if f32 else 1e-3, "dx of the colsum form")
        return outs, check
    run_guarded(call)


@case("gg_layernorm_fwd_bn", "gg_layernorm_fwd_bn_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("M,Cc", [(64, 64), (65, 192), (1, 8), (50, 40), (77, 576)])
def test_layernorm_of_batchnorm(dt, M, Cc):
    """LN(BN(y)) with the applied stream written by the same kernel.  test_(f32_)layernorm_with_batchnorm_apply_on_load: stream 1e-6 (f32) / rtol 8e-3 atol 1e-3
    (bf16), LayerNorm against torch on the stream 1e-4 (f32) / 1e-2 (bf16), mean 1e-5 / 1e-4."""
    y = rnd(M, Cc, seed=70, scale=2.0, dtype=dt)
    mean, var = rnd(Cc, seed=71, scale=0.5), rnd(Cc, seed=72).abs() + 0.5
    stat = torch.stack([mean, (var + 1e-5).rsqrt()])
    bg, bb, g, b = rnd(Cc, seed=73) + 1.0, rnd(Cc, seed=74, scale=0.3), rnd(Cc, seed=75) + 1.0, rnd(Cc, seed=76, scale=0.2)
    xt = (y.double() - mean.double()) * stat[1].double() * bg.double() + bb.double()

    def call(S, L):
        yi = S.inp("y", y.to(dt), misalign=16)
        o = {"xout": S.out("xout", M, Cc, dt), "out": S.out("out", M, Cc, dt), "mean": S.out("mean", 1, M, F32), "rstd": S.out("rstd", 1, M, F32)}
        fn = L.lib().gg_layernorm_fwd_bn_f32 if dt == F32 else L.lib().gg_layernorm_fwd_bn
        L.check(fn(yi.ptr, S.inp("bn_stat", stat.reshape(-1)).ptr, S.inp("bn_gamma", bg).ptr, S.inp("bn_beta", bb).ptr, o["xout"].ptr, S.inp("gamma", g).ptr,
                   S.inp("beta", b).ptr, M, Cc, L.f32(1e-5), o["out"].ptr, o["mean"].ptr, o["rstd"].ptr, L.stream()), "gg_layernorm_fwd_bn")

        def check(v):
            f32 = dt == F32
            close(v["xout"], xt, 1e-6 if f32 else 8e-3, 1e-6 if f32 else 1e-3, "bn-applied stream")
            x32 = v["xout"].double()
            close(v["out"], F.layer_norm(x32, (Cc,), g.double(), b.double(), 1e-5), 1e-4 if f32 else 1e-2, 1e-4 if f32 else 1e-2, "ln on the written stream")
            close(v["mean"][0], x32.mean(1), 1e-5 if f32 else 1e-4, 1e-5 if f32 else 1e-4, "ln mean")
        return o, check
    run_guarded(call)


@case("gg_token_mean_fwd", "gg_token_mean_bwd", "gg_token_mean_fwd_f32", "gg_token_mean_bwd_f32", "gg_token_mean_fwd_f16")
@pytest.mark.parametrize("B,T,Cc", [(5, 49, 64), (1, 1, 8), (3, 50, 40), (2, 257, 72)])
def test_token_mean(B, T, Cc):
    """test_pooling: forward rtol = atol = 1e-5 of the mean of the stored values; backward rtol = atol = 1e-2 in bf16 (that test's default), f32 at the forward's 1e-5."""
    x, d = rnd(B * T, Cc, seed=50), rnd(B, Cc, seed=51)

    def call(S, L):
        lib, st = L.lib(), L.stream()
        o = {}
        for tag, dt, fwd, bwd in (("bf16", BF, lib.gg_token_mean_fwd, lib.gg_token_mean_bwd), ("f32", F32, lib.gg_token_mean_fwd_f32, lib.gg_token_mean_bwd_f32),
                                  ("f16", F16, lib.gg_token_mean_fwd_f16, None)):
            xi = S.inp("x_" + tag, x.to(dt), misalign=16)
            o["mean_" + tag] = S.out("mean_" + tag, B, Cc, F32)
            L.check(fwd(xi.ptr, o["mean_" + tag].ptr, B, T, Cc, st), "token_mean_fwd " + tag)
            if bwd is not None:
                o["dx_" + tag] = S.out("dx_" + tag, B * T, Cc, dt, misalign=16)
                L.check(bwd(S.inp("dout", d).ptr, o["dx_" + tag].ptr, B, T, Cc, st), "token_mean_bwd " + tag)

        def check(v):
            for tag, dt in (("bf16", BF), ("f32", F32), ("f16", F16)):
                close(v["mean_" + tag], x.to(dt).double().view(B, T, Cc).mean(1), 1e-5, 1e-5, "token mean " + tag)
            close(v["dx_bf16"], (d.double() / T).repeat_interleave(T, 0), 1e-2, 1e-2, "token mean bwd")
            close(v["dx_f32"], (d.double() / T).repeat_interleave(T, 0), 1e-5, 1e-5, "token mean bwd f32")
        return o, check
    run_guarded(call)


@case("gg_view_mean_fwd", "gg_view_mean_bwd", "gg_view_mean_fwd_f32", "gg_view_mean_bwd_f32")
@pytest.mark.parametrize("N,V,Cc,pad", [(2, 4, 64, 0), (1, 1, 8, 8), (3, 4, 576, 24), (5, 7, 40, 8)])
def test_view_mean(N, V, Cc, pad):
    """mean over the V views (models/super_guessr.py:347), summed in view order, and its backward (dmean / V to every view).  f32: test_pooling's 1e-5; bf16 output /
    input: that test's bf16 default 1e-2."""
    emb, dm = rnd(N * V, Cc, seed=52), rnd(N, Cc, seed=53, dtype=BF)

    def call(S, L):
        lib, st = L.lib(), L.stream()
        ei = S.inp("emb", emb, misalign=16)
        o = {"mean_bf16": S.out("mean_bf16", N, Cc, BF, ld=Cc + pad), "mean_f32": S.out("mean_f32", N, Cc, F32, ld=Cc + pad),
             "demb_from_bf16": S.out("demb_from_bf16", N * V, Cc, F32), "demb_from_f32": S.out("demb_from_f32", N * V, Cc, F32)}
        L.check(lib.gg_view_mean_fwd(ei.ptr, o["mean_bf16"].ptr, Cc + pad, N, V, Cc, st), "gg_view_mean_fwd")
        L.check(lib.gg_view_mean_fwd_f32(ei.ptr, o["mean_f32"].ptr, Cc + pad, N, V, Cc, st), "gg_view_mean_fwd_f32")
        db, df = S.inp("dmean_bf16", dm.to(BF), ld=Cc + pad + 8, col_off=8), S.inp("dmean_f32", dm, ld=Cc + pad + 8, col_off=8)
        L.check(lib.gg_view_mean_bwd(db.ptr, db.ld, o["demb_from_bf16"].ptr, N, V, Cc, st), "gg_view_mean_bwd")
        L.check(lib.gg_view_mean_bwd_f32(df.ptr, df.ld, o["demb_from_f32"].ptr, N, V, Cc, st), "gg_view_mean_bwd_f32")

        def check(v):
            m = emb.double().view(N, V, Cc).mean(1)
            close(v["mean_f32"], m, 1e-5, 1e-5, "view mean f32"); close(v["mean_bf16"], m, 1e-2, 1e-2, "view mean bf16")
            r = (dm.double() / V).repeat_interleave(V, 0)
            close(v["demb_from_f32"], r, 1e-5, 1e-5, "view mean bwd f32"); close(v["demb_from_bf16"], r, 1e-5, 1e-5, "view mean bwd (bf16 dmean, f32 result)")
        return o, check
    run_guarded(call)


@case("gg_colsum_bf16", "gg_colsum_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("M,Cc,pad,rps,acc", [(512, 64, 0, 0, 0), (513, 40, 8, 171, 1), (511, 72, 24, 0, 1), (1, 8, 8, 1, 0), (1100, 200, 8, 111, 0)])
def test_column_sums(dt, M, Cc, pad, rps, acc):
    """test_gemm_splitk_and_wgrad_form's colsum check (rtol 1e-4, atol 1e-3); scratch of exactly gg_colsum_scratch_floats(M, C) floats; out ACCUMULATED on request."""
    x = rnd(M, Cc, seed=10, dtype=dt)
    rs = torch.tensor([2.0, 0.0, 0.5, 1.0, 1.5, 0.25, 3.0, 1.0, 0.0, 2.0])[:(M + rps - 1) // rps] if rps else None
    w = rs.double().repeat_interleave(rps)[:M, None] if rps else 1.0

    def call(S, L):
        lib, st = L.lib(), L.stream()
        xi = S.inp("x", x.to(dt), ld=Cc + pad + 8, col_off=8, misalign=16)
        sc = S.scratch("scratch", 4 * lib.gg_colsum_scratch_floats(M, Cc), row_bytes=4 * Cc)
        o = S.out("out", 1, Cc, F32, init=torch.full((Cc,), 2.0) if acc else None)
        fn = lib.gg_colsum_bf16 if dt == BF else lib.gg_colsum_f32
        L.check(fn(xi.ptr, xi.ld, M, Cc, S.inp("rowscale", rs).ptr if rps else None, rps, sc.ptr, o.ptr, acc, st), "gg_colsum")
        return {"out": o}, lambda v: close(v["out"][0], 2.0 * acc + (x.double() * w).sum(0), 1e-4, 1e-3, "colsum")
    run_guarded(call)


# ------------------------------------------------------------------------------------------- convolution family
@case("gg_dwconv3x3_fwd", "gg_dwconv3x3_bwd_data", "gg_dwconv3x3_bwd_weight", "gg_dwconv3x3_fwd_f32", "gg_dwconv3x3_bwd_data_f32", "gg_dwconv3x3_bwd_weight_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("B,H,W,Cc,stride", [(2, 8, 8, 8, 1), (1, 7, 7, 40, 1), (3, 9, 9, 24, 2), (2, 14, 14, 48, 2), (1, 15, 13, 40, 2), (1, 1, 1, 8, 1), (2, 12, 6, 16, 1)])
def test_depthwise_conv(dt, B, H, W, Cc, stride):
    """Depthwise 3 x 3 forward (with BatchNorm partials: gg_dwconv_stat_rows / gg_dwconv_f32_stat_rows rows exactly), data gradient, weight gradient (scratch of
    gg_dwconv_(f32_)wgrad_scratch_floats; grad ACCUMULATED from ones).  test_dwconv's reference (torch conv2d + autograd) and tolerances: 1e-2 / 1e-2, weight gradient
    and column sums rtol 1e-3 atol 1e-2 (of the stored result)."""
    x, w = rnd(B, H, W, Cc, seed=20, dtype=dt), rnd(Cc, 1, 3, 3, seed=21, scale=0.4)
    taps = w.view(Cc, 9).t().contiguous()
    xr, wr = x.permute(0, 3, 1, 2).double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
    yref = F.conv2d(xr, wr, None, stride, 1, 1, Cc)
    Ho, Wo = yref.shape[-2:]
    dy = rnd(B, Ho, Wo, Cc, seed=22, dtype=dt)
    yref.backward(dy.permute(0, 3, 1, 2).double())
    f32 = dt == F32

    def call(S, L):
        lib, st = L.lib(), L.stream()
        xi, ti = S.inp("x", x.to(dt).reshape(-1, Cc), misalign=16), S.inp("taps", taps)
        rows = (lib.gg_dwconv_f32_stat_rows if f32 else lib.gg_dwconv_stat_rows)(B, Ho, Wo, Cc, stride)
        y, cs = S.out("y", B * Ho * Wo, Cc, dt), S.out("colstats", rows, 2 * Cc, F32)
        L.check((lib.gg_dwconv3x3_fwd_f32 if f32 else lib.gg_dwconv3x3_fwd)(xi.ptr, ti.ptr, y.ptr, B, H, W, Cc, stride, cs.ptr, st), "dwconv fwd")
        dyi = S.inp("dy", dy.to(dt).reshape(-1, Cc), misalign=16)
        dx = S.out("dx", B * H * W, Cc, dt)
        L.check((lib.gg_dwconv3x3_bwd_data_f32 if f32 else lib.gg_dwconv3x3_bwd_data)(dyi.ptr, ti.ptr, dx.ptr, B, H, W, Cc, stride, st), "dwconv dgrad")
        nscr = (lib.gg_dwconv_f32_wgrad_scratch_floats if f32 else lib.gg_dwconv_wgrad_scratch_floats)(B, H, W, Cc, stride)
        sc = S.scratch("wgrad scratch", 4 * nscr, row_bytes=4 * 9 * Cc)
        dw = S.out("dw", Cc, 9, F32, init=torch.ones(Cc, 9))
        L.check((lib.gg_dwconv3x3_bwd_weight_f32 if f32 else lib.gg_dwconv3x3_bwd_weight)(xi.ptr, dyi.ptr, B, H, W, Cc, stride, sc.ptr, dw.ptr, 1, st), "dwconv wgrad")

        def check(v):
            close(v["y"].view(B, Ho, Wo, Cc).permute(0, 3, 1, 2), yref.detach(), 1e-2, 1e-2, "dwconv fwd")
            yq = v["y"].double(); s = v["colstats"].double().view(-1, 2, Cc).sum(0)
            close(s[0], yq.sum(0), 1e-3, 1e-2, "dw colsum"); close(s[1], (yq * yq).sum(0), 1e-3, 1e-2, "dw colsumsq")
            close(v["dx"].view(B, H, W, Cc).permute(0, 3, 1, 2), xr.grad, 1e-2, 1e-2, "dwconv dgrad")
            close(v["dw"].view(Cc, 1, 3, 3) - 1.0, wr.grad, 1e-3, 1e-2, "dwconv wgrad")
        return {"y": y, "colstats": cs, "dx": dx, "dw": dw}, check
    run_guarded(call)


@case("gg_im2col_nchw3_f32", "gg_im2col_nchw3_f32_f32", "gg_im2col_nhwc_bf16", "gg_im2col_nhwc_f32", "gg_col2im_nhwc_bf16", "gg_col2im_nhwc_f32")
@pytest.mark.parametrize("B,H,W,Cc,stride", [(2, 20, 20, 16, 2), (1, 18, 18, 8, 2), (2, 9, 7, 40, 2), (1, 8, 8, 8, 1), (1, 1, 1, 8, 2), (1, 15, 13, 24, 1)])
def test_im2col_col2im(B, H, W, Cc, stride):
    """im2col gathers and col2im (its adjoint) are pure data movement: exact against torch unfold / its autograd in f32, bf16 col2im (a sum of up to nine bf16
    values, stored in bf16) at test_im2col_matches_conv's default 1e-2.  k order (ky, kx, ci); the NCHW3 form pads k = 27 to 32 with zeros."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x3, xh = rnd(B, 3, H, W, seed=11, dtype=BF), rnd(B, H, W, Cc, seed=13, dtype=BF)
    d = rnd(B * Ho * Wo, 9 * Cc, seed=15, dtype=BF)

    def unfold(x_nchw, c):
        cols = F.unfold(x_nchw, 3, padding=1, stride=stride)
        return cols.view(B, c, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * c)
    xr = xh.double().clone().requires_grad_(True)
    cols_ref = unfold(xr.permute(0, 3, 1, 2), Cc)
    (cols_ref * d.double()).sum().backward()
    col3_ref = torch.zeros(B * Ho * Wo, 32, dtype=torch.float64); col3_ref[:, :27] = unfold(x3.double(), 3)

    def call(S, L):
        lib, st = L.lib(), L.stream()
        x3i = S.inp("x_nchw3", x3.reshape(-1, W), misalign=16)
        o = {"col3_bf16": S.out("col3_bf16", B * Ho * Wo, 32, BF), "col3_f32": S.out("col3_f32", B * Ho * Wo, 32, F32)}
        L.check(lib.gg_im2col_nchw3_f32(x3i.ptr, o["col3_bf16"].ptr, B, H, W, stride, st), "im2col_nchw3")
        L.check(lib.gg_im2col_nchw3_f32_f32(x3i.ptr, o["col3_f32"].ptr, B, H, W, stride, st), "im2col_nchw3_f32")
        for tag, dt in (("bf16", BF), ("f32", F32)):
            xi, di = S.inp("x_" + tag, xh.to(dt).reshape(-1, Cc), misalign=16), S.inp("dcol_" + tag, d.to(dt))
            o["col_" + tag], o["dx_" + tag] = S.out("col_" + tag, B * Ho * Wo, 9 * Cc, dt), S.out("dx_" + tag, B * H * W, Cc, dt)
            if dt == BF:
                L.check(lib.gg_im2col_nhwc_bf16(xi.ptr, o["col_bf16"].ptr, B, H, W, Cc, stride, st), "im2col_nhwc")
                L.check(lib.gg_col2im_nhwc_bf16(di.ptr, o["dx_bf16"].ptr, B, H, W, Cc, stride, st), "col2im_nhwc")
            else:
                L.check(lib.gg_im2col_nhwc_f32(xi.ptr, None, None, None, 0, o["col_f32"].ptr, B, H, W, Cc, stride, st), "im2col_nhwc_f32")
                L.check(lib.gg_col2im_nhwc_f32(di.ptr, o["dx_f32"].ptr, B, H, W, Cc, stride, st), "col2im_nhwc_f32")

        def check(v):
            for tag in ("bf16", "f32"):
                assert torch.equal(v["col3_" + tag].double(), col3_ref), "col3 " + tag
                assert torch.equal(v["col_" + tag].double(), cols_ref.detach()), "col " + tag
            close(v["dx_f32"].view(B, H, W, Cc), xr.grad, 1e-6, 1e-6, "col2im f32"); close(v["dx_bf16"].view(B, H, W, Cc), xr.grad, 1e-2, 1e-2, "col2im bf16")
        return o, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- BatchNorm
@case("gg_bn_finalize", "gg_bn_eval_stat", "gg_bn_apply", "gg_bn_apply_f32", "gg_bn_bwd", "gg_bn_bwd_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("M,Cc,act,with_res", [(840, 48, 0, False), (129, 40, 1, True), (1, 8, 1, False), (257, 8, 0, True), (300, 576, 1, True)])
def test_batchnorm(dt, M, Cc, act, with_res):
    """test_batchnorm_train's reference (torch batch_norm in training mode + autograd) and tolerances: statistics 1e-5 / 1e-4, running buffers 1e-5 / 1e-4, apply
    1e-2, dy rtol 2e-2 atol 1e-2, dgamma / dbeta rtol 1e-2 atol 0.5 (ACCUMULATED from ones).  partials: gg_stat_rows_capacity(nparts) rows exactly (the header's
    capacity), the rows beyond nparts hold the fill; scratch: gg_bn_bwd_scratch_floats."""
    T = max(1, M // 4)
    y = (rnd(M, Cc, seed=30, scale=2.0) + 0.5).to(BF).float()
    gamma, beta, res, dout = 1 + 0.2 * rnd(Cc, seed=31), 0.1 * rnd(Cc, seed=32), rnd(M, Cc, seed=33, dtype=dt), rnd(M, Cc, seed=34, dtype=dt)
    rs = torch.tensor([1.25, 0.0, 1.25, 1.25, 1.25])[:(M + T - 1) // T]
    rsr = rs.double().repeat_interleave(T)[:M, None]
    parts = torch.stack([torch.stack([y[i:i + 128].sum(0), (y[i:i + 128] ** 2).sum(0)]) for i in range(0, M, 128)])
    nparts = parts.shape[0]
    mean, var = y.double().mean(0), y.double().var(0, unbiased=False)
    yr, g_, b_ = y.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    if M > 1:
        z = F.batch_norm(yr, None, None, g_, b_, True, 0.1, 1e-5)
        if with_res:
            z = res.double() + rsr * z
        out_ref = F.gelu(z) if act else z
        out_ref.backward(dout.double())
    f32 = dt == F32

    def call(S, L):
        lib, st = L.lib(), L.stream()
        cap = lib.gg_stat_rows_capacity(nparts)
        pb = S.out("partials", cap, 2 * Cc, F32, written=False)               # in / scratch: the valid rows are given, the reduction scratch rows are free
        pb.view[:nparts].copy_(parts.reshape(nparts, 2 * Cc)); pb.before = pb.buf.clone()
        stat = S.out("stat", 2, Cc, F32)
        rm, rv = S.out("running_mean", 1, Cc, F32, init=torch.zeros(Cc)), S.out("running_var", 1, Cc, F32, init=torch.ones(Cc))
        L.check(lib.gg_bn_finalize(pb.ptr, nparts, Cc, M, L.f32(1e-5), L.f32(0.1), stat.ptr, rm.ptr, rv.ptr, st), "gg_bn_finalize")
        ev = S.out("eval_stat", 2, Cc, F32)
        L.check(lib.gg_bn_eval_stat(S.inp("rm_in", mean.float()).ptr, S.inp("rv_in", var.float() + 0.5).ptr, Cc, L.f32(1e-5), ev.ptr, st), "gg_bn_eval_stat")
        outs = {"stat": stat, "running_mean": rm, "running_var": rv, "eval_stat": ev}
        if M > 1:
            torch.cuda.synchronize()
            si = S.inp("stat_in", stat.view.cpu().reshape(-1), misalign=16)
            yi, gi, bi = S.inp("y", y.to(dt), misalign=16), S.inp("gamma", gamma), S.inp("beta", beta)
            ri = S.inp("residual", res.to(dt)) if with_res else None
            rsi = S.inp("rowscale", rs) if with_res else None
            out, dz, dy = S.out("out", M, Cc, dt), S.out("dz", M, Cc, dt), S.out("dy", M, Cc, dt)
            dg, db = S.out("dgamma", 1, Cc, F32, init=torch.ones(Cc)), S.out("dbeta", 1, Cc, F32, init=torch.ones(Cc))
            L.check((lib.gg_bn_apply_f32 if f32 else lib.gg_bn_apply)(yi.ptr, si.ptr, gi.ptr, bi.ptr, M, Cc, act, ri.ptr if ri else None, rsi.ptr if rsi else None, T,
                                                                      out.ptr, st), "gg_bn_apply")
            sc = S.scratch("scratch", 4 * lib.gg_bn_bwd_scratch_floats(M, Cc), row_bytes=8 * Cc)
            L.check((lib.gg_bn_bwd_f32 if f32 else lib.gg_bn_bwd)(S.inp("dout", dout.to(dt)).ptr, yi.ptr, si.ptr, gi.ptr, bi.ptr, M, Cc, act, ri.ptr if ri else None,
                                                                  rsi.ptr if rsi else None, T, dz.ptr, dy.ptr, sc.ptr, dg.ptr, db.ptr, 1, st), "gg_bn_bwd")
            outs.update(out=out, dz=dz, dy=dy, dgamma=dg, dbeta=db)

        def check(v):
            close(v["stat"][0], mean, 1e-5, 1e-5, "bn mean"); close(v["stat"][1], torch.rsqrt(var + 1e-5), 1e-4, 1e-5, "bn rstd")
            close(v["running_mean"][0], 0.1 * mean, 1e-5, 1e-6, "running_mean")
            if M > 1:
                close(v["running_var"][0], 0.9 + 0.1 * y.double().var(0, unbiased=True), 1e-4, 1e-6, "running_var")
            close(v["eval_stat"][0], mean.float(), 1e-6, 1e-6, "eval mean"); close(v["eval_stat"][1], torch.rsqrt(var.float().double() + 0.5 + 1e-5), 1e-4, 1e-5, "eval rstd")
            if M > 1:
                close(v["out"], out_ref.detach(), 1e-2, 1e-2, "bn apply"); close(v["dy"], yr.grad, 2e-2, 1e-2, "bn dy")
                close(v["dgamma"][0] - 1.0, g_.grad, 1e-2, 0.5, "bn dgamma"); close(v["dbeta"][0] - 1.0, b_.grad, 1e-2, 0.5, "bn dbeta")
        return outs, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- head, loss, scoring
@case("gg_geo_head", "gg_haversine_matrix")
@pytest.mark.parametrize("N,K,f32", [(3, 12647, False), (2, 12647, True), (1, 1000, False), (5, 8, True), (4, 1001, False)])
def test_geo_head(centroids, N, K, f32):
    """The fused head epilogue at K = 12647 (dlogits pitch 12648: "columns K..ldd zeroed" is asserted as the header states it) and small / ragged K, bf16 and f32
    dlogits, logits with a padded pitch.  Reference: oracle.geo_ref (soft_ce, log_softmax, haversine_matrix) at the tolerances of
    test_geo_head_small_k_and_edge_rows / test_geo_head_matches_oracle_and_reference_golden: loss 1e-4, dlogits rtol 2e-2 atol 1e-5 (bf16) / rtol 1e-3 atol 1e-8 with
    rel-L2 < 2e-5 (f32), top-k probabilities 1e-4, distances rtol 2e-4 atol 0.05 km."""
    import numpy as np
    from oracle import geo_ref as GR
    rng = np.random.default_rng(K + N)
    cent = centroids[:K].astype(np.float32) if K <= centroids.shape[0] and K > 8 else np.stack([rng.uniform(-180, 180, K), rng.uniform(-90, 90, K)], 1).astype(np.float32)
    logits = rng.standard_normal((N, K), dtype=np.float32)
    labels = (cent[rng.integers(0, K, N)] + rng.uniform(-0.5, 0.5, (N, 2))).astype(np.float32)
    labels[:, 1] = np.clip(labels[:, 1], -89.5, 89.5)
    loss, dl, _, _ = GR.soft_ce(logits, labels, cent)
    lp = GR.log_softmax(logits)
    nc = min(5, K)
    idx = np.argsort(-lp, axis=-1, kind="stable")[:, :nc]
    ldd = (K + 7) // 8 * 8 + (8 if K < 12647 else 0)

    def call(S, L):
        a = L.GeoHeadArgs()
        li = S.inp("logits", torch.from_numpy(logits), ld=K + 5, misalign=16)
        ci, lab = S.inp("centroids", torch.from_numpy(cent).reshape(-1)), S.inp("labels", torch.from_numpy(labels).reshape(-1))
        o = {"loss_rows": S.out("loss_rows", 1, N, F32), "loss": S.out("loss", 1, 1, F32), "preds": S.out("preds", 1, N, I64), "llh": S.out("llh", N, 2, F32),
             "topk_vals": S.out("topk_vals", N, nc, F32), "topk_idx": S.out("topk_idx", N, nc, I64), "nearest": S.out("nearest", 1, N, I64),
             "dlogits": S.out("dlogits", N, ldd, F32 if f32 else BF)}               # the whole pitch is the kernel's: it writes columns 0..K and zeroes K..ldd
        a.logits, a.ldl, a.N, a.K, a.labels, a.centroids, a.mode, a.smoothing_km, a.grad_scale = li.ptr, li.ld, N, K, lab.ptr, ci.ptr, 1, 65.0, 1.0 / N
        a.loss_rows, a.loss, a.dlogits, a.ldd, a.dlogits_f32 = o["loss_rows"].ptr, o["loss"].ptr, o["dlogits"].ptr, ldd, int(f32)
        a.preds, a.llh, a.topk_vals, a.topk_idx, a.num_candidates, a.nearest = o["preds"].ptr, o["llh"].ptr, o["topk_vals"].ptr, o["topk_idx"].ptr, nc, o["nearest"].ptr
        L.check(L.lib().gg_geo_head(C.byref(a), L.stream()), "gg_geo_head")
        o["dist"] = S.out("dist", N, K, F32)
        L.check(L.lib().gg_haversine_matrix(lab.ptr, ci.ptr, o["dist"].ptr, N, K, L.stream()), "gg_haversine_matrix")

        def check(v):
            np.testing.assert_allclose(float(v["loss"]), loss, rtol=1e-4)
            d = v["dlogits"].float().numpy()
            assert not d[:, K:].any(), "dlogits columns K..ldd must be zero"
            if f32:
                np.testing.assert_allclose(d[:, :K], dl, rtol=1e-3, atol=1e-8)
                assert np.linalg.norm((d[:, :K] - dl).astype(np.float64)) / np.linalg.norm(dl.astype(np.float64)) < 2e-5
            else:
                np.testing.assert_allclose(d[:, :K], dl, rtol=2e-2, atol=1e-5)
            np.testing.assert_array_equal(v["topk_idx"].numpy(), idx); np.testing.assert_array_equal(v["preds"].numpy()[0], idx[:, 0])
            np.testing.assert_allclose(v["topk_vals"].numpy(), np.exp(np.take_along_axis(lp, idx, -1)), rtol=1e-4)
            np.testing.assert_allclose(v["llh"].numpy(), cent[idx[:, 0]])
            dref = GR.haversine_matrix(labels, cent.T.copy())
            np.testing.assert_allclose(v["dist"].numpy(), dref, rtol=2e-4, atol=0.05)
            near = v["nearest"].numpy()[0]
            np.testing.assert_allclose(dref[np.arange(N), near], dref.min(1), atol=0.05)
        return o, check
    run_guarded(call)


@case("gg_geoguessr_score", "gg_geoguessr_score_f64")
@pytest.mark.parametrize("take", [None, 1, 257])
def test_scoring(golden_dir, take):
    """run_benchmark.py:25-65 on the inputs of tests/golden/score.npz (test_scoring_matches_reference_golden: distances rtol 1e-8 atol 1e-9 for float64 coordinates,
    INTEGER scores bit-exact; float32 coordinates: scores against the oracle's rounding of the kernel's own fp64 distances, as that test does)."""
    import os
    import numpy as np
    from oracle import geo_ref as GR
    g = np.load(os.path.join(golden_dir, "score.npz"))
    reps = 1 if take is None or take <= len(g["pred"]) else -(-take // len(g["pred"]))
    pred, true = np.tile(g["pred"], (reps, 1))[:take], np.tile(g["true"], (reps, 1))[:take]
    dist, score = np.tile(g["dist_km"], reps)[:take], np.tile(g["score"], reps)[:take]
    n = len(pred)

    def call(S, L):
        lib, st = L.lib(), L.stream()
        p64, t64 = S.inp("pred64", torch.from_numpy(pred).double().reshape(-1), misalign=16), S.inp("true64", torch.from_numpy(true).double().reshape(-1))
        p32, t32 = S.inp("pred32", torch.from_numpy(pred).float().reshape(-1), misalign=16), S.inp("true32", torch.from_numpy(true).float().reshape(-1))
        o = {"d64": S.out("d64", 1, n, torch.float64), "s64": S.out("s64", 1, n, torch.int32), "d32": S.out("d32", 1, n, torch.float64), "s32": S.out("s32", 1, n, torch.int32)}
        L.check(lib.gg_geoguessr_score_f64(p64.ptr, t64.ptr, n, o["d64"].ptr, o["s64"].ptr, st), "gg_geoguessr_score_f64")
        L.check(lib.gg_geoguessr_score(p32.ptr, t32.ptr, n, o["d32"].ptr, o["s32"].ptr, st), "gg_geoguessr_score")

        def check(v):
            if g["pred"].dtype == np.float64:
                np.testing.assert_allclose(v["d64"].numpy()[0], dist, rtol=1e-8, atol=1e-9); np.testing.assert_array_equal(v["s64"].numpy()[0], score)
            np.testing.assert_array_equal(v["s64"].numpy()[0], GR.geoguessr_score(v["d64"].numpy()[0]))
            np.testing.assert_array_equal(v["s32"].numpy()[0], GR.geoguessr_score(v["d32"].numpy()[0]))
            if g["pred"].dtype != np.float64:
                np.testing.assert_allclose(v["d32"].numpy()[0], dist, rtol=1e-8, atol=1e-9); np.testing.assert_array_equal(v["s32"].numpy()[0], score)
        return o, check
    run_guarded(call)


@case("gg_drop_path_scales")
@pytest.mark.parametrize("slots,batch", [(1, 1), (22, 8), (7, 257)])
def test_drop_path_scales(slots, batch):
    """out[s][b] is 0 or 1 / (1 - rate[s]) (timm DropPath with scale_by_keep), fully determined by (seed, counter): both fills give the same rows."""
    rates = torch.linspace(0.0, 0.5, slots)

    def call(S, L):
        ri = S.inp("rates", rates, misalign=16)
        o = S.out("scales", slots, batch, F32, misalign=16)
        L.check(L.lib().gg_drop_path_scales(ri.ptr, slots, batch, 1234567, 3, o.ptr, L.stream()), "gg_drop_path_scales")

        def check(v):
            keep = (1.0 / (1.0 - rates))[:, None].expand(slots, batch)
            ok = (v["scales"] == 0) | ((v["scales"] - keep).abs() <= 1e-6 * keep)
            assert bool(ok.all()) and bool((v["scales"][0] == 1.0).all())                 # rate 0 keeps everything
        return {"scales": o}, check
    run_guarded(call)


@case("gg_bn_bwd_reduce", "gg_bn_bwd_finalize", "gg_bn_bwd_apply", "gg_bn_bwd_reduce_f32", "gg_bn_bwd_apply_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("M,Cc,act", [(840, 48, 1), (129, 40, 0), (2, 8, 1), (257, 576, 1), (1100, 192, 0)])
def test_batchnorm_backward_three_passes(dt, M, Cc, act):
    """reduce (dz, partial rows) -> finalize (coef [3][C], dgamma, dbeta ACCUMULATED from ones) -> apply (dy = coef0 * dz + coef1 * y + coef2): the chain equals torch's
    BatchNorm backward at test_batchnorm_train's tolerances (dy rtol 2e-2 atol 1e-2, dgamma / dbeta rtol 1e-2 atol 0.5).  partials:
    gg_stat_rows_capacity(gg_bn_bwd_rows(M, C)) rows exactly, as norm.hip documents."""
    y = (rnd(M, Cc, seed=30, scale=2.0) + 0.5).to(BF).float()
    gamma, beta, dout = 1 + 0.2 * rnd(Cc, seed=31), 0.1 * rnd(Cc, seed=32), rnd(M, Cc, seed=34, dtype=dt)
    mean, var = y.double().mean(0), y.double().var(0, unbiased=False)
    stat = torch.cat([mean, torch.rsqrt(var + 1e-5)]).float()
    yr, g_, b_ = y.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    z = F.batch_norm(yr, None, None, g_, b_, True, 0.1, 1e-5)
    (F.gelu(z) if act else z).backward(dout.double())
    f32 = dt == F32

    def call(S, L):
        lib, st = L.lib(), L.stream()
        rows = lib.gg_bn_bwd_rows(M, Cc)
        yi, si, gi, bi = S.inp("y", y.to(dt), misalign=16), S.inp("stat", stat, misalign=16), S.inp("gamma", gamma), S.inp("beta", beta)
        dz = S.out("dz", M, Cc, dt)
        part = S.scratch("partials", 4 * lib.gg_stat_rows_capacity(rows) * 2 * Cc, row_bytes=8 * Cc)
        L.check((lib.gg_bn_bwd_reduce_f32 if f32 else lib.gg_bn_bwd_reduce)(S.inp("dout", dout.to(dt)).ptr, yi.ptr, si.ptr, gi.ptr, bi.ptr, M, Cc, act, None, None, 0,
                                                                            dz.ptr, part.ptr, st), "gg_bn_bwd_reduce")
        coef, dg, db = S.out("coef", 3, Cc, F32), S.out("dgamma", 1, Cc, F32, init=torch.ones(Cc)), S.out("dbeta", 1, Cc, F32, init=torch.ones(Cc))
        L.check(lib.gg_bn_bwd_finalize(part.ptr, rows, Cc, M, si.ptr, gi.ptr, coef.ptr, dg.ptr, db.ptr, 1, st), "gg_bn_bwd_finalize")
        torch.cuda.synchronize()
        dzi, ci = S.inp("dz_in", dz.view.cpu(), misalign=16), S.inp("coef_in", coef.view.cpu().reshape(-1))
        dy = S.out("dy", M, Cc, dt)
        L.check((lib.gg_bn_bwd_apply_f32 if f32 else lib.gg_bn_bwd_apply)(dzi.ptr, yi.ptr, ci.ptr, M, Cc, None, 0, dy.ptr, st), "gg_bn_bwd_apply")

        def check(v):
            close(v["dy"], yr.grad, 2e-2, 1e-2, "bn dy (three passes)")
            close(v["dgamma"][0] - 1.0, g_.grad, 1e-2, 0.5, "bn dgamma"); close(v["dbeta"][0] - 1.0, b_.grad, 1e-2, 0.5, "bn dbeta")
        return {"dz": dz, "coef": coef, "dgamma": dg, "dbeta": db, "dy": dy}, check
    run_guarded(call)


# ------------------------------------------------------------------------------------------- either side of the encoder
@case("gg_segment_mean")
@pytest.mark.parametrize("sizes,D,pad", [((3, 0, 1, 5), 64, 0), ((1,), 8, 8), ((0, 0, 2), 40, 3), ((7, 7, 300), 576, 24)])
def test_segment_mean(sizes, D, pad):
    """out[k] = mean of emb[member[ptr[k] : ptr[k + 1]]] summed in list order in fp32 (the reference's running sum), zeros for empty segments: the same fp32
    additions in the same order, so bit-exact against a sequential fp32 sum (test_build_prototypes_matches_reference_golden asserts equality as well)."""
    rows = max(sum(sizes), 1) + 3
    emb = rnd(rows, D, seed=90)
    g = torch.Generator().manual_seed(91)
    member = torch.cat([torch.randint(0, rows, (s,), generator=g) for s in sizes]).to(I64) if sum(sizes) else torch.zeros(1, dtype=I64)
    ptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=I64)
    ref = torch.zeros(len(sizes), D)
    for k, s in enumerate(sizes):
        acc = torch.zeros(D)
        for i in member[ptr[k]:ptr[k + 1]]:
            acc = acc + emb[i]
        ref[k] = acc / s if s else acc

    def call(S, L):
        ei = S.inp("emb", emb, ld=D + pad + 4, col_off=4, misalign=16)
        o = S.out("out", len(sizes), D, F32)
        L.check(L.lib().gg_segment_mean(ei.ptr, ei.ld, S.inp("ptr", ptr, misalign=16).ptr, S.inp("member", member).ptr, len(sizes), D, o.ptr, L.stream()), "gg_segment_mean")
        return {"out": o}, lambda v: close(v["out"], ref, 0, 2e-7, "segment mean")         # atol 2e-7: that test's bound for the prototype means (x / s vs x * (1 / s))
    run_guarded(call)


@case("gg_preprocess_bilinear")
@pytest.mark.parametrize("N,Hs,Ws,Hd,Wd,u8,norm", [(2, 9, 7, 12, 12, True, True), (1, 16, 16, 16, 16, False, False), (3, 5, 11, 3, 4, False, True), (1, 1, 1, 2, 3, True, False),
                                                   (2, 33, 17, 8, 8, True, True)])
def test_preprocess_bilinear(N, Hs, Ws, Hd, Wd, u8, norm):
    """Bilinear resize (align_corners=False) -> / 255 for uint8 -> (x - mean) / std against oracle.preprocess_ref.prepare_batch at
    test_preprocess_bilinear_matches_reference_golden's atol 1e-5 (fp32, FMA contraction only)."""
    import ctypes
    from oracle import preprocess_ref as P
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    g = torch.Generator().manual_seed(N + Hs)
    src = torch.randint(0, 256, (N, 3, Hs, Ws), dtype=torch.uint8, generator=g) if u8 else torch.rand(N, 3, Hs, Ws, generator=g)
    ref = torch.from_numpy(P.prepare_batch(src.numpy(), (Hd, Wd), mean if norm else None, std if norm else None))

    def call(S, L):
        si = S.inp("src", src.reshape(-1, Ws), misalign=16)
        o = S.out("dst", N * 3 * Hd, Wd, F32, misalign=16)
        m3 = (ctypes.c_float * 3)(*mean) if norm else None
        s3 = (ctypes.c_float * 3)(*std) if norm else None
        L.check(L.lib().gg_preprocess_bilinear(si.ptr, int(u8), N, Hs, Ws, o.ptr, Hd, Wd, m3, s3, L.stream()), "gg_preprocess_bilinear")
        return {"dst": o}, lambda v: close(v["dst"].view(N, 3, Hd, Wd), ref, 0, 1e-5, "preprocess")
    run_guarded(call)


# ------------------------------------------------------------------------------------------- fused convolution forms
def _bn_act(y, mean, rstd, gamma, beta, act):
    """(z, act(z), act'(z)) in fp64 for z = gamma * (y - mean) * rstd + beta."""
    z = ((y.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()).clone().requires_grad_(True)
    a = F.gelu(z) if act else z * 1.0
    a.sum().backward()
    return z.detach(), a.detach(), z.grad


FUSED_DW = [(2, 8, 8, 8, 1, 1), (1, 7, 7, 40, 1, 1), (3, 9, 9, 24, 2, 1), (2, 14, 14, 48, 2, 0), (1, 15, 13, 40, 2, 1), (1, 1, 1, 8, 1, 1), (2, 12, 6, 16, 1, 0), (1, 13, 13, 16, 1, 1),
            (1, 7, 7, 8, 2, 1)]


@case("gg_dwconv3x3_fwd_fused", "gg_dwconv3x3_fwd_fused_f32", "gg_dwconv3x3_bwd_data_fused", "gg_dwconv3x3_bwd_data_fused_f32", "gg_dwconv3x3_s2_bwd_data_fused",
      "gg_dwconv3x3_s2_bwd_data_fused_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("B,H,W,Cc,stride,act", FUSED_DW)
def test_depthwise_conv_fused(dt, B, H, W, Cc, stride, act):
    """The BatchNorm-fused depthwise forms on odd / even maps, W % 4 != 0, C = 8 / 40, strides 1 and 2.  Forward: conv over act(BN(y1)) formed on load + partial statistics
    of the result (rows: gg_dwconv_fwd_fused_stat_rows / gg_dwconv_f32_stat_rows exactly).  Data gradient (stride 1: gg_dwconv3x3_bwd_data_fused, stride 2: _s2_): dy =
    c0 * dz + c1 * y2 + c2 on the loads, * act'(BN(y1)) and the two column sums on the stores (rows: gg_dwconv_fused_stat_rows / gg_dwconv_s2_fused_stat_rows and the f32
    twins); both fusions, and the plain call (no fusion).  Tolerances: test_dwconv_with_batchnorm_gelu_on_load (bf16 1e-2, statistics rtol 2e-3 atol 5e-2),
    test_f32_dwconv_with_batchnorm_gelu_on_load (1e-4, statistics 1e-4 / 1e-2), test_dwconv_stride2_data_gradient_with_batchnorm_fusions (bf16 2e-2, sums 1e-3 / 2e-2 and
    5e-2; the stride-1 bf16 kernel has no parity test of its own and takes the same), its f32 twin and test_f32_dwconv_data_gradient_with_batchnorm_fusions (rtol 2e-4 atol
    2e-5, sums 2e-4 / 2e-3)."""
    f32 = dt == F32
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y1 = rnd(B, H, W, Cc, seed=50, scale=1.5, dtype=dt)
    mean, var = rnd(Cc, seed=51, scale=0.4), rnd(Cc, seed=52).abs() + 0.5
    rstd = (var + 1e-5).rsqrt()
    gamma, beta = rnd(Cc, seed=53) + 1.0, rnd(Cc, seed=54, scale=0.3)
    w = rnd(Cc, 1, 3, 3, seed=55, scale=0.4); taps = w.view(Cc, 9).t().contiguous()
    stat = torch.cat([mean, rstd])
    _, a1, dact = _bn_act(y1, mean, rstd, gamma, beta, act)
    a1q = a1 if f32 else a1.float().to(BF).double()                   # the bf16 kernel rounds the activation it forms, as the unfused path stores it
    fwd_ref = F.conv2d(a1q.permute(0, 3, 1, 2), w.double(), None, stride, 1, 1, Cc)
    dz, y2 = rnd(B, Ho, Wo, Cc, seed=90, dtype=dt), rnd(B, Ho, Wo, Cc, seed=91, dtype=dt)
    coef = torch.stack([1 + 0.2 * rnd(Cc, seed=92), 0.3 * rnd(Cc, seed=93), 0.1 * rnd(Cc, seed=94)])
    dy = coef[0].double() * dz.double() + coef[1].double() * y2.double() + coef[2].double()
    if not f32:
        dy = dy.float().to(BF).double()

    def conv_t(g):
        xr = torch.zeros(B, Cc, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xr, w.double(), None, stride, 1, 1, Cc).backward(g.permute(0, 3, 1, 2))
        return xr.grad.permute(0, 2, 3, 1)
    da = conv_t(dy)
    xh = (y1.double() - mean.double()) * rstd.double()

    def call(S, L):
        lib, st = L.lib(), L.stream()
        yi, si, gi, bi, ti = S.inp("y1", y1.to(dt).reshape(-1, Cc), misalign=16), S.inp("stat", stat), S.inp("gamma", gamma), S.inp("beta", beta, misalign=16), S.inp("taps", taps)
        rows = lib.gg_dwconv_f32_stat_rows(B, Ho, Wo, Cc, stride) if f32 else lib.gg_dwconv_fwd_fused_stat_rows(B, H, W, Cc, stride)
        o = {"y": S.out("y", B * Ho * Wo, Cc, dt), "colstats": S.out("colstats", rows, 2 * Cc, F32)}
        L.check((lib.gg_dwconv3x3_fwd_fused_f32 if f32 else lib.gg_dwconv3x3_fwd_fused)(yi.ptr, si.ptr, gi.ptr, bi.ptr, act, ti.ptr, o["y"].ptr, B, H, W, Cc, stride,
                                                                                        o["colstats"].ptr, st), "dwconv fwd fused")
        dzi, y2i, ci = S.inp("dz", dz.to(dt).reshape(-1, Cc), misalign=16), S.inp("y2", y2.to(dt).reshape(-1, Cc)), S.inp("coef", coef.reshape(-1))
        if stride == 1:
            fn = lib.gg_dwconv3x3_bwd_data_fused_f32 if f32 else lib.gg_dwconv3x3_bwd_data_fused
            prow = lambda fused_in: lib.gg_dwconv_f32_stat_rows(B, H, W, Cc, 1) if f32 else lib.gg_dwconv_fused_stat_rows(B, H, W, Cc, fused_in)
        else:
            fn = lib.gg_dwconv3x3_s2_bwd_data_fused_f32 if f32 else lib.gg_dwconv3x3_s2_bwd_data_fused
            prow = lambda fused_in: (lib.gg_dwconv_f32_s2_fused_stat_rows if f32 else lib.gg_dwconv_s2_fused_stat_rows)(B, H, W, Cc)
        o["dx_both"], o["part_both"] = S.out("dx_both", B * H * W, Cc, dt), S.out("part_both", prow(1), 2 * Cc, F32)
        L.check(fn(dzi.ptr, y2i.ptr, ci.ptr, ti.ptr, o["dx_both"].ptr, B, H, W, Cc, yi.ptr, si.ptr, gi.ptr, bi.ptr, act, o["part_both"].ptr, st), "dgrad fused (both)")
        dyi = S.inp("dy", dy.reshape(-1, Cc).to(dt))
        o["dx_ep"], o["part_ep"] = S.out("dx_ep", B * H * W, Cc, dt), S.out("part_ep", prow(0), 2 * Cc, F32)
        L.check(fn(dyi.ptr, None, None, ti.ptr, o["dx_ep"].ptr, B, H, W, Cc, yi.ptr, si.ptr, gi.ptr, bi.ptr, act, o["part_ep"].ptr, st), "dgrad fused (stores only)")
        o["dx_in"] = S.out("dx_in", B * H * W, Cc, dt)
        L.check(fn(dzi.ptr, y2i.ptr, ci.ptr, ti.ptr, o["dx_in"].ptr, B, H, W, Cc, None, None, None, None, 0, None, st), "dgrad fused (loads only)")
        o["dx_plain"] = S.out("dx_plain", B * H * W, Cc, dt)
        L.check(fn(dyi.ptr, None, None, ti.ptr, o["dx_plain"].ptr, B, H, W, Cc, None, None, None, None, 0, None, st), "dgrad plain")

        def check(v):
            t = 1e-4 if f32 else 1e-2
            close(v["y"].view(B, Ho, Wo, Cc).permute(0, 3, 1, 2), fwd_ref, t, t, "fused dwconv vs conv2d")
            yq = v["y"].double(); s = v["colstats"].double().view(-1, 2, Cc).sum(0)
            close(s[0], yq.sum(0), 1e-4 if f32 else 2e-3, 1e-2 if f32 else 5e-2, "fused dwconv colsum")
            close(s[1], (yq * yq).sum(0), 1e-4 if f32 else 2e-3, 1e-2 if f32 else 5e-2, "fused dwconv colsumsq")
            rt, at = (2e-4, 2e-5) if f32 else (2e-2, 2e-2)
            ref = da * dact
            for k in ("both", "ep"):
                close(v["dx_" + k].view(B, H, W, Cc), ref, rt, at, "fused dgrad " + k)
                oq = v["dx_" + k].double().view(B, H, W, Cc); s = v["part_" + k].double().view(-1, 2, Cc).sum(0)
                close(s[0], oq.sum((0, 1, 2)), 2e-4 if f32 else 1e-3, 2e-3 if f32 else 2e-2, "sum dz " + k)
                close(s[1], (oq * xh).sum((0, 1, 2)), 2e-4 if f32 else 1e-3, 2e-3 if f32 else 5e-2, "sum dz*xhat " + k)
            close(v["dx_in"].view(B, H, W, Cc), da, rt, at, "fused dgrad (loads only)"); close(v["dx_plain"].view(B, H, W, Cc), da, rt, at, "plain dgrad")
        return o, check
    run_guarded(call)


@case("gg_im2col_nhwc_bn_bf16", "gg_im2col_nhwc_f32", "gg_col2im_nhwc_bnbwd_bf16", "gg_col2im_nhwc_bnbwd_f32")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("B,H,W,Cc,act,nparts", [(2, 18, 18, 48, 1, 37), (1, 9, 7, 40, 0, 5), (1, 8, 8, 8, 1, 1), (2, 11, 11, 24, 1, 64), (1, 1, 1, 8, 0, 3), (1, 15, 13, 8, 1, 200)])
def test_im2col_col2im_batchnorm_forms(dt, B, H, W, Cc, act, nparts):
    """Stride-2 im2col over act(BN(y)) of a saved conv output (padding taps stay exactly zero) and col2im fused with BatchNorm backward's reduce (dz = da * act'(BN(y)),
    nparts partial rows; the buffer holds gg_stat_rows_capacity(nparts) rows, what gg_bn_bwd_finalize is given).  Tolerances: test_im2col_fused_batchnorm_gelu (bf16 rtol
    8e-3 atol 1e-3), test_col2im_fused_batchnorm_backward_reduce (dz 8e-3 / 1e-3, sums 2e-3 / 2e-2) and its f32 twin (dz 2e-5 / 2e-6, sums 1e-4 / 1e-3); the f32 gather is
    the f32 BatchNorm-apply's 1e-6 (test_f32_layernorm_with_batchnorm_apply_on_load's stream bound)."""
    f32 = dt == F32
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = rnd(B, H, W, Cc, seed=16, scale=1.5, dtype=dt)
    mean, var = rnd(Cc, seed=17, scale=0.3), rnd(Cc, seed=18).abs() + 0.5
    rstd = (var + 1e-5).rsqrt()
    gamma, beta = rnd(Cc, seed=19) + 1.0, rnd(Cc, seed=20, scale=0.3)
    _, a, dact = _bn_act(y, mean, rstd, gamma, beta, act)
    cols = F.unfold(a.permute(0, 3, 1, 2), 3, padding=1, stride=2).view(B, Cc, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * Cc)
    ones = F.unfold(torch.ones(B, 1, H, W, dtype=torch.float64), 3, padding=1, stride=2).view(B, 1, 9, Ho * Wo).permute(0, 3, 2, 1).expand(B, Ho * Wo, 9, Cc).reshape(B * Ho * Wo, 9 * Cc)
    dcol = rnd(B * Ho * Wo, 9 * Cc, seed=21, scale=0.5, dtype=dt)
    xr = torch.zeros(B, Cc, H, W, dtype=torch.float64, requires_grad=True)
    (F.unfold(xr, 3, padding=1, stride=2).view(B, Cc, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * Cc) * dcol.double()).sum().backward()
    da = xr.grad.permute(0, 2, 3, 1)
    if not f32:
        da = da.float().to(BF).double()                                # bf16-rounded, as the unfused path stores it (the parity test's reference)
    dpre = da * dact
    xh = (y.double() - mean.double()) * rstd.double()

    def call(S, L):
        lib, st = L.lib(), L.stream()
        yi, si, gi, bi = S.inp("y", y.to(dt).reshape(-1, Cc), misalign=16), S.inp("stat", torch.cat([mean, rstd])), S.inp("gamma", gamma, misalign=16), S.inp("beta", beta)
        col = S.out("col", B * Ho * Wo, 9 * Cc, dt)
        if f32:
            L.check(lib.gg_im2col_nhwc_f32(yi.ptr, si.ptr, gi.ptr, bi.ptr, act, col.ptr, B, H, W, Cc, 2, st), "gg_im2col_nhwc_f32 (bn)")
        else:
            L.check(lib.gg_im2col_nhwc_bn_bf16(yi.ptr, si.ptr, gi.ptr, bi.ptr, act, col.ptr, B, H, W, Cc, 2, st), "gg_im2col_nhwc_bn_bf16")
        di = S.inp("dcol", dcol.to(dt), misalign=16)
        dz = S.out("dz", B * H * W, Cc, dt)
        part = S.out("part", lib.gg_stat_rows_capacity(nparts), 2 * Cc, F32, written=False)       # the kernel writes nparts rows; the rest is the finalize's reduction scratch
        L.check((lib.gg_col2im_nhwc_bnbwd_f32 if f32 else lib.gg_col2im_nhwc_bnbwd_bf16)(di.ptr, yi.ptr, si.ptr, gi.ptr, bi.ptr, act, dz.ptr, part.ptr, nparts, B, H, W, Cc, st),
                "gg_col2im_nhwc_bnbwd")

        def check(v):
            got = v["col"].double()
            assert bool((got[ones == 0] == 0).all()), "padding taps must be exactly zero"
            close(got, cols, 1e-6 if f32 else 8e-3, 1e-6 if f32 else 1e-3, "fused im2col")
            close(v["dz"].view(B, H, W, Cc), dpre, 2e-5 if f32 else 8e-3, 2e-6 if f32 else 1e-3, "fused col2im dz")
            p = v["part"][:nparts].double()
            assert not bool(torch.isnan(p).any()), "every one of the nparts rows is written"
            s = p.view(nparts, 2, Cc).sum(0)
            close(s[0], dpre.sum((0, 1, 2)), 1e-4 if f32 else 2e-3, 1e-3 if f32 else 2e-2, "sum dz"); close(s[1], (dpre * xh).sum((0, 1, 2)), 1e-4 if f32 else 2e-3, 1e-3 if f32 else 2e-2, "sum dz*xhat")
        return {"col": col, "dz": dz, "part": part}, check
    run_guarded(call)


@case("gg_gemm_nt", "gg_gemm_nt_f32", "gg_bn_bwd_finalize", "gg_bn_bwd_fold_weights")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("M,Cin,Cmid,Cout", [(300, 64, 128, 72), (129, 8, 64, 8), (17, 64, 64, 64), (1111, 64, 128, 192)])
def test_convnorm_chain_backward_gemm_forms(dt, M, Cin, Cmid, Cout):
    """x -conv1-> y1 -BN(train) + GELU-> a1 -conv3-> y3 backward through the GEMM-side fusions: conv3's data gradient with the BatchNorm-backward epilogue (GgGemmArgs.bn_y:
    dz and the partial sums as colstats), gg_bn_bwd_finalize, then conv1's data gradient from the two sources (dz, y1): bf16 through gg_bn_bwd_fold_weights + A2 / k_split,
    f32 through A2 + a_bn_stat = coef.  test_convnorm_chain_backward_fused_into_gemms (bf16: dy 2e-2 / 2e-2, dgamma / dbeta 2e-2 / 0.5, dx 2e-2 / 3e-2) and
    test_f32_convnorm_chain_backward_fused_into_gemms (dy 2e-4 / 2e-5, dgamma / dbeta 2e-4 / 2e-3, dx 2e-4 / 5e-5).  The smallest batch here is 17 rows, not 2: with two
    rows xhat is +-1 and train-mode BatchNorm's dy is an exact cancellation (its true value is O(eps / var) of its terms), so a tolerance relative to dy says nothing
    about the kernel -- the two-row memory case of this path is test_batchnorm_backward_three_passes[2-8-1]."""
    f32 = dt == F32
    x = rnd(M, Cin, seed=70, dtype=dt)
    W1 = rnd(Cmid, Cin, seed=71) / Cin ** 0.5
    W3 = (rnd(Cout, Cmid, seed=72) / Cmid ** 0.5).to(dt).float()
    gamma, beta = 1 + 0.2 * rnd(Cmid, seed=73), 0.3 * rnd(Cmid, seed=74)
    Gr, skip = rnd(M, Cout, seed=75, dtype=dt), rnd(M, Cin, seed=76, dtype=dt)
    y1 = ((x @ W1.to(dt).float().T) + 1.5).to(dt).float()
    yr, g_, b_ = y1.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    if M > 1:
        a1 = F.gelu(F.batch_norm(yr, None, None, g_, b_, True, 0.1, 1e-5))
        (a1 @ W3.double().T).backward(Gr.double())
    dx_ref = yr.grad @ W1.double() + skip.double()
    mean, var = y1.double().mean(0), y1.double().var(0, unbiased=False)
    stat = torch.cat([mean, torch.rsqrt(var + 1e-5)]).float()

    def call(S, L):
        lib, st = L.lib(), L.stream()
        gemm = lib.gg_gemm_nt_f32 if f32 else lib.gg_gemm_nt
        Gi = S.inp("dY", Gr.to(dt), ld=Cout + 8, misalign=16)
        W3t = S.inp("W3t", W3.T.contiguous().to(dt), ld=Cout + 8)                  # [Cmid, Cout]
        yi, si, gi, bi = S.inp("y1", y1.to(dt), misalign=16), S.inp("stat", stat), S.inp("gamma", gamma), S.inp("beta", beta)
        rows = lib.gg_gemm_colstats_rows(M)
        dz = S.out("dz", M, Cmid, dt)
        part = S.out("partials", lib.gg_stat_rows_capacity(rows), 2 * Cmid, F32, written=False)   # GEMM writes `rows` rows; the finalize's reduction uses the rest
        a = L.GemmArgs()
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N, a.K, a.split_k = Gi.ptr, Gi.ld, W3t.ptr, W3t.ld, dz.ptr, Cmid, M, Cmid, Cout, 1
        a.bn_y, a.bn_stat, a.bn_gamma, a.bn_beta, a.bn_act, a.colstats = yi.ptr, si.ptr, gi.ptr, bi.ptr, 1, part.ptr
        L.check(gemm(C.byref(a), st), "gemm bn_y epilogue")
        coef, dg, db = S.out("coef", 3, Cmid, F32), S.out("dgamma", 1, Cmid, F32), S.out("dbeta", 1, Cmid, F32)
        L.check(lib.gg_bn_bwd_finalize(part.ptr, rows, Cmid, M, si.ptr, gi.ptr, coef.ptr, dg.ptr, db.ptr, 0, st), "gg_bn_bwd_finalize")
        torch.cuda.synchronize()
        dzi, ci = S.inp("dz_in", dz.view.cpu(), misalign=16), S.inp("coef_in", coef.view.cpu().reshape(-1), misalign=16)
        ri = S.inp("residual", skip.to(dt), ld=Cin + 8)
        dx = S.out("dx", M, Cin, dt, ld=Cin + 8)
        b = L.GemmArgs()
        b.A, b.lda, b.A2, b.C, b.ldc, b.M, b.N, b.split_k, b.residual, b.ldr = dzi.ptr, Cmid, yi.ptr, dx.ptr, dx.ld, M, Cin, 1, ri.ptr, ri.ld
        outs = {"dz": dz, "coef": coef, "dgamma": dg, "dbeta": db, "dx": dx}
        if f32:
            Wt = S.inp("W1t", W1.T.contiguous(), ld=Cmid + 4)                       # [Cin, Cmid]
            b.a_bn_stat, b.B, b.ldb, b.K = ci.ptr, Wt.ptr, Wt.ld, Cmid
        else:
            Bf, bias = S.out("Bf", Cin, 2 * Cmid, BF), S.out("fold_bias", 1, Cin, F32)
            L.check(lib.gg_bn_bwd_fold_weights(S.inp("W1", W1).ptr, ci.ptr, si.ptr, Cmid, Cin, Bf.ptr, bias.ptr, st), "gg_bn_bwd_fold_weights")
            torch.cuda.synchronize()
            Bfi, bsi = S.inp("Bf_in", Bf.view.cpu()), S.inp("fold_bias_in", bias.view.cpu())
            b.k_split, b.B, b.ldb, b.K, b.bias = Cmid, Bfi.ptr, 2 * Cmid, 2 * Cmid, bsi.ptr
            outs.update(Bf=Bf, fold_bias=bias)
        L.check(gemm(C.byref(b), st), "gemm two-source")

        def check(v):
            dy = v["coef"][0].double() * v["dz"].double() + v["coef"][1].double() * y1.double() + v["coef"][2].double()
            close(dy, yr.grad, 2e-4 if f32 else 2e-2, 2e-5 if f32 else 2e-2, "dy from gemm-epilogue dz + coef")
            close(v["dgamma"][0], g_.grad, 2e-4 if f32 else 2e-2, 2e-3 if f32 else 0.5, "dgamma"); close(v["dbeta"][0], b_.grad, 2e-4 if f32 else 2e-2, 2e-3 if f32 else 0.5, "dbeta")
            close(v["dx"], dx_ref, 2e-4 if f32 else 2e-2, 5e-5 if f32 else 3e-2, "two-source dgrad")
        return outs, check
    run_guarded(call)


@case("gg_layernorm_bwd_colsum", "gg_bn_bwd_coef_from_x")
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("M,Cc", [(333, 96), (65, 8), (17, 40), (700, 576), (1200, 192)])
def test_batchnorm_coefficients_from_layernorm_column_sums(dt, M, Cc):
    """x = BN_train(y) -> LN(x): gg_layernorm_bwd_colsum's rows (sum dx * x, sum dx) -> gg_bn_bwd_coef_from_x -> dy = c0 * dx + c1 * y + c2 equals torch's dL/dy
    (test_layernorm_bwd_with_batchnorm_column_sums: 2e-5 of the largest magnitude in f32, 3e-2 in bf16).  part: (gg_layernorm_bwd_colsum_rows(M) + 64) rows (header).
    Smallest batch 17 rows: a two-row train-mode BatchNorm backward is an exact cancellation (see test_convnorm_chain_backward_gemm_forms)."""
    f32 = dt == F32
    y = rnd(M, Cc, seed=80, scale=1.7, dtype=dt) + 0.4
    y = y.to(dt).float()
    bg, bb, g, b = rnd(Cc, seed=81) * 0.3 + 1.0, rnd(Cc, seed=82, scale=0.5), rnd(Cc, seed=83) * 0.2 + 1.0, rnd(Cc, seed=84, scale=0.2)
    dout, dres = rnd(M, Cc, seed=85, dtype=dt), rnd(M, Cc, seed=86, dtype=dt)
    yr = y.double().clone().requires_grad_(True)
    x_ref = F.batch_norm(yr, None, None, bg.double(), bb.double(), True, 0.1, 1e-5)
    (F.layer_norm(x_ref, (Cc,), g.double(), b.double(), 1e-5) * dout.double()).sum().backward(retain_graph=True)
    x_ref.backward(dres.double())
    stat = torch.cat([y.double().mean(0), (y.double().var(0, unbiased=False) + 1e-5).rsqrt()]).float()
    x = x_ref.detach().float().to(dt).float()                            # the stored stream (gg_bn_apply's result in the storage type)
    mu = x.double().mean(1); rs = (x.double().var(1, unbiased=False) + 1e-5).rsqrt()

    def call(S, L):
        lib, st = L.lib(), L.stream()
        xi, di, dri = S.inp("x", x.to(dt), misalign=16), S.inp("dout", dout.to(dt)), S.inp("dres", dres.to(dt), misalign=16)
        rows = lib.gg_layernorm_bwd_colsum_rows(M)
        dx = S.out("dx", M, Cc, dt)
        part = S.scratch("part", 4 * (rows + 64) * 2 * Cc, row_bytes=8 * Cc)
        si = S.inp("stat", stat, misalign=16)
        L.check(lib.gg_layernorm_bwd_colsum(di.ptr, xi.ptr, int(f32), S.inp("mean", mu.float()).ptr, S.inp("rstd", rs.float()).ptr, S.inp("gamma", g).ptr, M, Cc, dri.ptr, dx.ptr,
                                            part.ptr, st), "gg_layernorm_bwd_colsum")
        coef = S.out("coef", 3, Cc, F32)
        L.check(lib.gg_bn_bwd_coef_from_x(part.ptr, rows, Cc, M, si.ptr, S.inp("bn_gamma", bg).ptr, S.inp("bn_beta", bb).ptr, coef.ptr, st), "gg_bn_bwd_coef_from_x")

        def check(v):
            dy = v["coef"][0].double() * v["dx"].double() + v["coef"][1].double() * y.double() + v["coef"][2].double()
            err = float((dy - yr.grad).abs().max() / yr.grad.abs().max())
            assert err < (2e-5 if f32 else 3e-2), err
        return {"dx": dx, "coef": coef}, check
    run_guarded(call)


@case("gg_preprocess_pil")
@pytest.mark.parametrize("Hs,Ws,flt,Hr,Wr,top,left,Hc,Wc,mul,norm", [(50, 60, 3, 28, 34, 2, 5, 24, 24, 0, True), (17, 9, 2, 33, 20, 0, 0, 33, 20, 1, True), (8, 8, 2, 8, 8, 0, 0, 8, 8, 0, False),
                                                                     (5, 7, 2, 3, 4, 1, 1, 2, 3, 0, True), (64, 31, 3, 16, 8, 3, 1, 10, 7, 1, False), (40, 90, 3, 20, 45, 0, 11, 20, 23, 0, True)])
def test_preprocess_pil(Hs, Ws, flt, Hr, Wr, top, left, Hc, Wc, mul, norm):
    """Pillow resize of the whole image (bilinear / bicubic; down, up and no-op), crop window, 1 / 255, (x - mean) / std.  Reference: oracle.preprocess_ref.pil_resize (pinned
    bit-exact to Pillow by tests/golden/preprocess_pil.npz); as test_preprocess_pil_matches_pillow_and_transformers_golden the uint8 crop is BIT-IDENTICAL and the float
    result agrees to 1e-6.  The workspace has exactly gg_preprocess_pil_workspace_bytes bytes."""
    import ctypes
    import numpy as np
    from oracle import preprocess_ref as P
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    img = np.random.default_rng(Hs * Ws).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    crop = P.pil_resize(img, Wr, Hr, flt)[top:top + Hc, left:left + Wc]
    x = crop.astype(np.float32) * np.float32(1.0 / 255.0) if mul else crop.astype(np.float32) / np.float32(255.0)
    if norm:
        x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    ref = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))

    def call(S, L):
        lib = L.lib()
        need = lib.gg_preprocess_pil_workspace_bytes(Hs, Ws, flt, Hr, Wr, Wc)
        assert need >= 0
        si = S.inp("src", torch.from_numpy(img).reshape(Hs, Ws * 3), misalign=16)
        o = {"dst": S.out("dst", 3 * Hc, Wc, F32, misalign=16), "u8": S.out("u8", Hc, Wc * 3, torch.uint8)}
        ws = S.scratch("workspace", need, row_bytes=16 * max(Ws, Wr))
        m3 = (ctypes.c_float * 3)(*mean) if norm else None
        s3 = (ctypes.c_float * 3)(*std) if norm else None
        L.check(lib.gg_preprocess_pil(si.ptr, Hs, Ws, flt, Hr, Wr, top, left, Hc, Wc, mul, m3, s3, o["dst"].ptr, o["u8"].ptr, ws.ptr, L.stream()), "gg_preprocess_pil")

        def check(v):
            assert torch.equal(v["u8"].view(Hc, Wc, 3), torch.from_numpy(np.ascontiguousarray(crop))), "uint8 crop differs from Pillow's"
            close(v["dst"].view(3, Hc, Wc), ref, 0, 1e-6, "pixel values")
        return o, check
    run_guarded(call)


@case("gg_proto_refine")
@pytest.mark.parametrize("seed,Kc,D,B,V,members,with_probs", [(11, 40, 64, 33, 4, False, True), (12, 30, 48, 41, 4, True, True), (13, 6, 8, 1, 1, False, False), (14, 12, 40, 7, 1, True, True)])
def test_proto_refine(seed, Kc, D, B, V, members, with_probs):
    """ProtoRefiner.forward against oracle.proto_ref.refine as test_proto_refine_matches_oracle / _within_cluster_matches_oracle do: cells and guess indices identical,
    coordinates at numpy's assert_allclose default (rtol 1e-7).  A cell without prototypes, candidate_probs = NULL, V = 1, the member branch."""
    import numpy as np
    from oracle import proto_ref as P
    rng = np.random.default_rng(seed)
    counts = rng.poisson(2.0, Kc) + (1 if Kc < 10 else 0)
    if Kc >= 10:
        counts[[3, 7]] = 0
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    Pn = int(ptr[-1])
    pemb = rng.standard_normal((Pn, D), dtype=np.float32)
    pll = np.stack([rng.uniform(-180, 180, Pn), rng.uniform(-90, 90, Pn)], 1).astype(np.float32)
    nc = min(5, Kc)
    q = rng.standard_normal((B, V, D), dtype=np.float32)
    cands = np.stack([rng.permutation(Kc)[:nc] for _ in range(B)]).astype(np.int64)
    if Kc >= 10:
        cands[0, 0] = 3
    probs = np.sort(rng.dirichlet(np.ones(nc), B).astype(np.float32), 1)[:, ::-1].copy() if with_probs else None
    init = np.stack([rng.uniform(-180, 180, B), rng.uniform(-90, 90, B)], 1).astype(np.float32)
    kw = dict(topk=nc, max_refinement=30000.0 if members else 1000.0, temperature=1.6)
    if members:
        nmem = rng.integers(0, 5, Pn); nmem[:3] = 0
        mptr = np.concatenate([[0], np.cumsum(nmem)]).astype(np.int64)
        memb = rng.standard_normal((max(int(mptr[-1]), 1), D), dtype=np.float32)
        mll = np.stack([rng.uniform(-180, 180, len(memb)), rng.uniform(-90, 90, len(memb))], 1).astype(np.float32)
        kw.update(member_ptr=mptr, member_emb=memb, member_lnglat=mll)
    o_llh, o_cell, o_idx = P.refine(q, init, cands, probs, ptr, pemb, pll, **kw)
    T = torch.from_numpy

    def call(S, L):
        a = L.ProtoRefineArgs()
        a.embedding, a.B, a.V, a.D = S.inp("embedding", T(q).reshape(B * V, D), misalign=16).ptr, B, V, D
        a.initial_preds, a.candidate_cells = S.inp("initial_preds", T(init)).ptr, S.inp("candidate_cells", T(cands), misalign=16).ptr
        a.candidate_probs = S.inp("candidate_probs", T(probs)).ptr if with_probs else None
        a.num_candidates, a.topk, a.cell_ptr, a.num_cells = nc, nc, S.inp("cell_ptr", T(ptr)).ptr, Kc
        a.proto_emb, a.proto_lnglat, a.max_refinement, a.temperature = S.inp("proto_emb", T(pemb), misalign=16).ptr, S.inp("proto_lnglat", T(pll)).ptr, kw["max_refinement"], 1.6
        o = {"llh": S.out("llh", B, 2, F32), "cell": S.out("cell", 1, B, I64), "idx": S.out("idx", 1, B, I64)}
        a.out_llh, a.out_cell, a.out_idx = o["llh"].ptr, o["cell"].ptr, o["idx"].ptr
        if members:
            a.member_ptr, a.member_emb, a.member_lnglat = S.inp("member_ptr", T(mptr)).ptr, S.inp("member_emb", T(memb), misalign=16).ptr, S.inp("member_lnglat", T(mll)).ptr
        L.check(L.lib().gg_proto_refine(C.byref(a), L.stream()), "gg_proto_refine")

        def check(v):
            np.testing.assert_array_equal(v["cell"].numpy()[0], o_cell); np.testing.assert_array_equal(v["idx"].numpy()[0], o_idx)
            np.testing.assert_allclose(v["llh"].numpy(), o_llh)
        return o, check
    run_guarded(call)
