"""Every site that evaluates GELU, GELU', QuickGELU or QuickGELU' (csrc/common.h), held to fp64 point by point on the probe sets of tests/act_cases.py.

Each site is made a pointwise map by identity operands, so the reference is a function of the one value the site saw:

* GEMM epilogues: A = stacked identity, B = the probe matrix, so C[m, n] = B[n, m mod K].  With a pre-activation copy the reference is the activation of the
  returned copy; without one, of the plain-epilogue result of the same launch (which must be the probe itself, or 0 for a subnormal probe).
* dact and BatchNorm-backward epilogues: B = all ones, so the product is exactly 1 and dact_preact / bn_y are the probes.
* BatchNorm prologues and on-load fusions: stat = (0, 1), gamma = 1, beta = 0, and W = identity or taps = centre 1.
* col2im and depthwise backward epilogues: the upstream is 1 on the centre tap only.

Gates: tests/act_cases.py::gate, per element; the 16-bit forms at bf16 / fp16 sites, the f32 forms at f32 sites.  Every test prints its worst err/gate per form
(`pytest -s`).  All comparisons run on the device in float64.

Left out: the 256 x 256 LDS-DMA tile of gemm.hip (taken from 512 tiles of 256 x 256 on, K >= 4096 or GELU + pre-activation copy at N >= 1536: it shares the epilogue
code of the 192 x 128 tile, gemm_nt_dma_kernel's row phase).

Measured on an MI355X, worst err/gate per form, the same at every site of a form to three digits: bf16 sites GELU 0.962 (z = 2.078), GELU' 0.987, QuickGELU 0.995,
QuickGELU' 0.993 (all four the storage rounding); fp16 sites QuickGELU 0.986, QuickGELU' 0.995; the fp8 site 0.887; f32 sites GELU 0.713 at z = -3.43 (and 1.000 at
z = -2^-149, where z / 2 is a tie between 0 and the smallest subnormal), GELU' 0.341, QuickGELU 0.088, QuickGELU' 0.114.  Prologues with beta = 2 at ragged M and K:
bf16 0.627 of its gate (max err 2.5e-2), f32 rel-L2 2.3e-7 (K = 136) and 3.6e-7 (K = 392), split 3.0e-7.  Before the repairs in csrc/common.h the bf16 GELU' sites
(BatchNorm backward, the x GELU' epilogue of all three tile forms) returned -1.16e-5 for a NaN argument.
"""
import ctypes as C

import pytest
import torch

from tests import act_cases as A

pytestmark = pytest.mark.gpu

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
NAN = float("nan")
ACT = {"gelu": 1, "quick": 2}
PSET = {BF16: "P16", F16: "P16H", F32: "P32"}


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as o
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return o


def _L():
    from geoguessr_ai_amd import _lib
    return _lib


_CACHE = {}


def probes(name, dtype=None):
    """The flat probe set on the device (cached, never written)."""
    key = (name, dtype)
    if key not in _CACHE:
        _CACHE[key] = A.probe_matrix(name, dtype).flatten().cuda()
    return _CACHE[key]


def chunks(flat, n):
    """The probe set in pieces of n values, the last padded with zeros."""
    out = []
    for i in range(0, flat.numel(), n):
        c = flat[i:i + n]
        if c.numel() < n:
            c = torch.cat([c, torch.zeros(n - c.numel(), dtype=flat.dtype, device=flat.device)])
        out.append(c)
    return out


def eye_stack(M, K, dtype):
    a = torch.zeros(M, K, dtype=dtype, device="cuda")
    a[torch.arange(M), torch.arange(M) % K] = 1.0
    return a


def affine(Cc, beta=0.0):
    """stat = (0, 1), gamma = 1, beta: BatchNorm(y) = y + beta exactly."""
    stat = torch.stack([torch.zeros(Cc), torch.ones(Cc)]).cuda()
    return stat, torch.ones(Cc, device="cuda"), torch.full((Cc,), beta, device="cuda")


def assert_seen(seen, want, what):
    """The value the site saw is the probe, bit for bit; a subnormal probe may have been flushed to zero by the matrix pipe."""
    ok = (seen == want) | (torch.isnan(seen) & torch.isnan(want)) | ((want.double().abs() < 2.0 ** -126) & (seen == 0))
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} probes did not reach the site unchanged, first {want.flatten()[int((~ok).flatten().nonzero()[0])].item()!r}"


class Worst:
    """Worst err/gate per form of one site; every violation is kept, and report() prints the figures and raises them together."""

    def __init__(self, what):
        self.what, self.by_form, self.failed = what, {}, []

    def add(self, got, z, kind, store, u=1.0, floor=0.0, where=""):
        form = A.form_for(kind, store)
        w, i, bad = A.check(got, z, form, store, u, floor)
        zi = float(z.double().flatten()[i])
        if bad:
            self.failed.append(f"[{form}{where}] " + "; ".join(bad))
        if not w <= 1.0:
            self.failed.append(f"[{form}{where}] err/gate {w:.3f} at z = {zi!r}: got {float(got.double().flatten()[i])!r}, "
                               f"fp64 {float(A.reference(A.KIND_OF[form], z.double().flatten()[i:i + 1])[0])!r}")
        if w >= self.by_form.get(form, (-1.0, 0.0))[0]:
            self.by_form[form] = (w, zi)

    def report(self):
        print(f"\n[{self.what}] " + "  ".join(f"{f}: worst err/gate {w:.3f} at z = {z!r}" for f, (w, z) in sorted(self.by_form.items())))
        assert not self.failed, f"{self.what}: " + " | ".join(self.failed)


# ---- norm.hip -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual0_rowscale1"])
@pytest.mark.parametrize("pset", ["own", "NONFINITE"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_batchnorm_apply_and_backward(ops, dtype, pset, with_residual):
    """gg_bn_apply / gg_bn_apply_f32 (out = act(z)) and gg_bn_bwd / gg_bn_bwd_f32 (dz = dout act'(z), dout = 1) at M = 512, C = 128: act_t / act_grad_t of norm.hip pick
    the 16-bit forms for 2-byte storage and the f32 forms otherwise.  With residual = 0 and rowscale = 1 the pre-activation is 0 + 1 z."""
    name = PSET[dtype] if pset == "own" else pset
    z = probes(name, dtype).view(A.ROWS, A.COLS)
    stat, gamma, beta = affine(A.COLS)
    kw = dict(residual=torch.zeros_like(z), rowscale=torch.ones(4, device="cuda"), rows_per_scale=128) if with_residual else {}
    w = Worst(f"norm.hip {name} {'residual' if with_residual else 'plain'}")
    ones = torch.ones_like(z)
    for act, code in (("gelu", "gelu"), ("quick", "quick_gelu")):
        w.add(ops.bn_apply(z, stat, gamma, beta, act=code, **kw), z, act, dtype)
        w.add(ops.bn_bwd(ones, z, stat, gamma, beta, act=code, **kw)[0], z, act + "_grad", dtype)
    w.report()


# ---- GEMM epilogues (gemm.hip in both builds, gemm_f32.hip) ---------------------------------------------------------------------------------------------------
def gemm(entry, Am, Bm, M, N, K, *, ldc=None, act=0, preact=False, dact_pre=None, dact=0):
    """One launch through GgGemmArgs; C and the pre-activation copy at pitch ldc (NaN-filled: the pad column must stay unwritten)."""
    L = _L()
    dt = Am.dtype
    ldc = N if ldc is None else ldc
    out = torch.full((M, ldc), NAN, dtype=dt, device="cuda")
    pre = torch.full((M, ldc), NAN, dtype=dt, device="cuda") if preact else None
    a = L.GemmArgs()
    a.A, a.lda, a.B, a.ldb, a.C, a.ldc = Am.data_ptr(), Am.stride(0), Bm.data_ptr(), Bm.stride(0), out.data_ptr(), ldc
    a.M, a.N, a.K, a.act, a.split_k = M, N, K, act, 1
    a.preact = pre.data_ptr() if preact else None
    if dact_pre is not None:
        assert dact_pre.shape == (M, ldc) and dact_pre.is_contiguous()
        a.dact_preact, a.dact = dact_pre.data_ptr(), dact
    L.check(getattr(L.lib(), entry)(C.byref(a), L.stream()), entry)
    if ldc != N:
        assert bool(torch.isnan(out[:, N:]).all()) and (pre is None or bool(torch.isnan(pre[:, N:]).all())), "the pad column was written"
    return out[:, :N], (pre[:, :N] if preact else None)


def gemm_epilogue_site(entry, dtype, M, N, K, what, *, ldc=None, kinds=("gelu", "quick"), nonfinite=True, plain_kinds=None):
    assert M % K == 0
    w = Worst(what)
    eye, ones = eye_stack(M, K, dtype), torch.ones(N, K, dtype=dtype, device="cuda")
    plain_kinds = kinds if plain_kinds is None else plain_kinds
    for c in chunks(probes(PSET[dtype]), N * K):
        Bm = c.view(N, K)
        want = Bm.t().repeat(M // K, 1)
        seen = None
        for kind in kinds:
            out, pre = gemm(entry, eye, Bm, M, N, K, ldc=ldc, act=ACT[kind], preact=True)
            assert_seen(pre, want, f"{what} {kind} + preact")
            w.add(out, pre, kind, dtype)
            if kind in plain_kinds:
                if seen is None:
                    seen = gemm(entry, eye, Bm, M, N, K, ldc=ldc)[0]
                    assert_seen(seen, want, f"{what} plain")
                w.add(gemm(entry, eye, Bm, M, N, K, ldc=ldc, act=ACT[kind])[0], seen, kind, dtype)
    for name in (PSET[dtype], "NONFINITE") if nonfinite else (PSET[dtype],):
        p = probes(name, dtype)
        flat = p.repeat(-(-M * N // p.numel()))[:M * N].view(M, N)
        ld = N if ldc is None else ldc
        dp = torch.zeros(M, ld, dtype=dtype, device="cuda")
        dp[:, :N] = flat
        for kind in kinds:
            out, _ = gemm(entry, eye, ones, M, N, K, ldc=ldc, dact_pre=dp, dact=ACT[kind])
            w.add(out, flat, kind + "_grad", dtype)
    w.report()


@pytest.mark.parametrize("M,N,K,form", [(128, 512, 128, "generic 128-column tile"), (1024, 64, 1024, "generic 64-column tile"), (1024, 256, 256, "LDS-DMA 192 x 128 tile")])
def test_gemm_bf16_epilogues(M, N, K, form):
    """gg_gemm_nt: GELU + preact and QuickGELU + preact (EPI_GELU, on the bf16-rounded tile), QuickGELU on the f32 accumulators (EPI_QGELU), x GELU' and x QuickGELU'
    (EPI_DGELU).  Dispatch (GG_GEMM_NT_NAME): N <= 64 takes the 128 x 64 tile; the LDS-DMA form needs K >= 192, N >= 128, M >= 1024, no f32 output, whole 16-byte chunks;
    everything else the 128 x 128 tile.  GELU without a copy shares EPI_GELU and is run too."""
    gemm_epilogue_site("gg_gemm_nt", BF16, M, N, K, f"gemm.hip bf16 {form} {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K,form", [(128, 512, 128, "generic"), (1024, 256, 256, "LDS-DMA")])
def test_gemm_fp16_epilogues(M, N, K, form):
    """gg_gemm_nt_f16 (gemm_f16.hip: gemm.hip built for fp16) on all finite fp16 values: QuickGELU forward, with the pre-activation copy, and x QuickGELU'; same dispatch
    as the bf16 build."""
    gemm_epilogue_site("gg_gemm_nt_f16", F16, M, N, K, f"gemm.hip fp16 {form} {M}x{N}x{K}", kinds=("quick",), nonfinite=False)


@pytest.mark.parametrize("M,N,K,ldc,form", [(128, 512, 128, None, "64 x 64 small form"), (128 * 257, 128, 128, None, "row-layout epilogue, 128 columns"),
                                            (128 * 257, 64, 128, None, "row-layout epilogue, 64 columns"), (128 * 257, 128, 128, 129, "general epilogue, 128 columns"),
                                            (128 * 257, 64, 128, 65, "general epilogue, 64 columns")])
def test_gemm_f32_epilogues(M, N, K, ldc, form):
    """gg_gemm_nt_f32: GELU, GELU + preact, QuickGELU, QuickGELU + preact, x GELU', x QuickGELU' (the QuickGELU forms are the expf restatements of gemm_f32.hip).
    Dispatch (gg_gemm_nt_f32): at most 256 tiles of 128 rows take the 64 x 64 small form, so M = 128 * 257 does not; the row-layout epilogue needs M % 128 == 0,
    N % tile == 0 and ldc % 4 == 0, so an output pitch of N + 1 takes the general epilogue without its paired stores (ldc % 32 != 0); the small form ends in the general
    epilogue with them (ldc = 512)."""
    gemm_epilogue_site("gg_gemm_nt_f32", F32, M, N, K, f"gemm_f32.hip {form} {M}x{N}x{K}", ldc=ldc)


# ---- BatchNorm-backward epilogues and BatchNorm prologues of the GEMMs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,M,acts", [(BF16, 512, ("gelu",)), (F32, 512, ("gelu", "quick")), (F32, 520, ("gelu", "quick"))], ids=["bf16", "f32_rows", "f32_general"])
def test_gemm_batchnorm_backward_epilogue(ops, dtype, M, acts):
    """ops.conv_dgrad_bn_bwd: dz = (dY Wt^T) act'(BN(y)) with dY = stacked identity, Wt = ones (the product is exactly 1), y = the probes; N = K = 128.  gemm.hip EPI_BNBWD
    (GELU only: the bf16 build has no QuickGELU form here), gemm_f32.hip FE_BNBWD in the row-layout epilogue (M % 128 == 0) and in the general one (M = 520)."""
    N = K = 128
    p = probes(PSET[dtype])
    y = p.repeat(2)[:M * N].view(M, N).contiguous()
    stat, gamma, beta = affine(N)
    w = Worst(f"BatchNorm-backward epilogue {str(dtype)[6:]} M={M}")
    for act in acts:
        dz = ops.conv_dgrad_bn_bwd(eye_stack(M, K, dtype), torch.ones(N, K, dtype=dtype, device="cuda"), y, stat, gamma, beta, act="gelu" if act == "gelu" else "quick_gelu",
                                   want_param_grads=False)[0]
        w.add(dz, y, act + "_grad", dtype)
    w.report()


@pytest.mark.parametrize("dtype,K,acts", [(BF16, 128, ("gelu",)), (F32, 128, ("gelu", "quick")), (F32, 392, ("gelu", "quick"))], ids=["bf16", "f32_ring", "f32_register_staged"])
def test_gemm_batchnorm_prologue(ops, dtype, K, acts):
    """ops.conv_bn_prologue: C = act(BN(y)) W^T with W = identity, so C = act(y) (the other products are act(.) x 0 = 0: every act of a finite probe is finite).
    gemm.hip's prologue (GELU only) at M = 512, K = N = 128; gemm_f32.hip on the LDS-DMA ring (K <= 384) and on the register-staged kernel (K = 392 > 384)."""
    p = probes(PSET[dtype])
    M = -(-p.numel() // K)
    y = chunks(p, M * K)[0].view(M, K)
    stat, gamma, beta = affine(K)
    Wm = torch.eye(K, dtype=dtype, device="cuda")
    w = Worst(f"BatchNorm prologue {str(dtype)[6:]} K={K}")
    for act in acts:
        w.add(ops.conv_bn_prologue(y, stat, gamma, beta, Wm, act="gelu" if act == "gelu" else "quick_gelu"), y, act, dtype)
    w.report()


# ---- gemm_fp8.hip ---------------------------------------------------------------------------------------------------------------------------------------------
def test_gemm_fp8_quick_gelu_epilogue(ops):
    """gg_gemm_nt_e4m3 at 128 x 256 x 128 with act = quick_gelu: A = identity codes (0x38 = 1.0), row n of B holds one half of the 254 finite e4m3 codes and has the scale
    sw[n] = 2^(-10 .. 4), sa = 1: the epilogue sees z = sw[n] code exactly (powers of two) and stores QuickGELU(z) as fp16."""
    codes, vals, scales = A.p8()
    M, N, K = 128, 256, 128
    Bc = torch.zeros(N, K, dtype=torch.uint8)
    z = torch.zeros(N, K, dtype=F64)
    sw = torch.ones(N, dtype=F64)
    for n in range(N):
        half, s = n % 2, (n // 2) % 15
        Bc[n, :127], z[n, :127], sw[n] = codes[half * 127:(half + 1) * 127], vals[half * 127:(half + 1) * 127] * scales[s], scales[s]
    Ac = torch.zeros(M, K, dtype=torch.uint8)
    Ac[torch.arange(M), torch.arange(M)] = 0x38
    sa = torch.ones(M, device="cuda")
    plain = ops.gemm_nt_e4m3(Ac.cuda(), Bc.cuda(), sa, sw.float().cuda())
    want = z.t().contiguous().cuda()
    assert torch.equal(plain.double(), want.to(F16).double())                 # the site saw the probes (the plain result is their fp16 rounding)
    out = ops.gemm_nt_e4m3(Ac.cuda(), Bc.cuda(), sa, sw.float().cuda(), act="quick_gelu")
    w = Worst("gemm_fp8.hip QuickGELU epilogue")
    w.add(out, want.float(), "quick", F16)
    w.report()


# ---- gemm_split3.hip ------------------------------------------------------------------------------------------------------------------------------------------
def planes_of(x):
    L = _L()
    x = x.contiguous()
    out = torch.empty((3,) + tuple(x.shape), dtype=BF16, device="cuda")
    L.check(L.lib().gg_split3_bf16(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), out.data_ptr(), L.stream()), "gg_split3_bf16")
    return out


def split3(Am, Wp, M, N, K, *, act=0, preact=False, dact_pre=None, dact=0, generic=False, plane_fed=False):
    """gg_gemm_nt_split3_af32 (A f32, split in the loader) or, plane_fed, gg_gemm_nt_split3_ex on the planes of A."""
    L = _L()
    a = L.Split3Args()
    out = torch.full((M, N), NAN, device="cuda")
    pre = torch.full((M, N), NAN, device="cuda") if preact else None
    cp = torch.empty((3, M, N), dtype=BF16, device="cuda") if generic else None
    a.b_planes, a.ldb, a.M, a.N, a.K, a.C, a.ldc, a.act = Wp.data_ptr(), K, M, N, K, out.data_ptr(), N, act
    if generic:
        a.c_planes, a.ldp = cp.data_ptr(), N
    a.preact = pre.data_ptr() if preact else None
    if dact_pre is not None:
        a.dact_preact, a.dact = dact_pre.data_ptr(), dact
    if plane_fed:
        Ap = planes_of(Am)
        a.a_planes, a.lda = Ap.data_ptr(), K
        L.check(L.lib().gg_gemm_nt_split3_ex(C.byref(a), L.stream()), "gg_gemm_nt_split3_ex")
    else:
        L.check(L.lib().gg_gemm_nt_split3_af32(C.byref(a), Am.data_ptr(), Am.stride(0), 0, L.stream()), "gg_gemm_nt_split3_af32")
    torch.cuda.synchronize()
    return out, pre


def split3_site(M, N, K, what, **kw):
    w = Worst(what)
    eye = eye_stack(M, K, F32)
    ones_p = planes_of(torch.ones(N, K, device="cuda"))
    for c in chunks(probes("P32"), N * K):
        Wm = c.view(N, K)
        want = Wm.t().repeat(M // K, 1)
        Wp = planes_of(Wm)
        for kind in ("gelu", "quick"):
            out, pre = split3(eye, Wp, M, N, K, act=ACT[kind], preact=True, **kw)
            assert_seen(pre, want, f"{what} {kind} + preact")
            w.add(out, pre, kind, F32)
    for name in ("P32", "NONFINITE"):
        p = probes(name, F32)
        flat = p.repeat(-(-M * N // p.numel()))[:M * N].view(M, N).contiguous()
        for kind in ("gelu", "quick"):
            out, _ = split3(eye, ones_p, M, N, K, dact_pre=flat, dact=ACT[kind], **kw)
            w.add(out, flat, kind + "_grad", F32)
    w.report()


@pytest.mark.parametrize("generic", [False, True], ids=["epilogue_classes", "generic_row_epilogue"])
@pytest.mark.parametrize("N", [128, 192])
@pytest.mark.parametrize("K", [128, 384])
def test_split3_gemm_epilogues(K, N, generic):
    """gg_gemm_nt_split3_af32 with A = f32 identity and W = the planes of the probes: the 128-row form (K < 384) and the 256-row form (K >= 384), 128-column tiles and the
    96-column tiles N = 192 takes (split3_af32_form).  act + preact is class 2 (GELU) / 5 (QuickGELU), dact class 3 / 6 (split3_epilogue_rows_ec, taken for N % 8 == 0 and
    ldc % 4 == 0); a c_planes output forces the generic row epilogue (split3_epilogue_rows)."""
    split3_site(K, N, K, f"gemm_split3.hip {'generic row epilogue' if generic else 'epilogue classes'} N={N} K={K}", generic=generic)


@pytest.mark.parametrize("M,N,K", [(128, 512, 128), (256, 256, 256)])
def test_split3_plane_fed_gemm_epilogue(M, N, K):
    """gg_gemm_nt_split3_ex (gemm_nt_split3_kernel, both operands as planes; M <= 128 takes its 128 x 128 tile, else 256 x 128) ends in the generic row epilogue,
    split3_epilogue_rows, in both tile forms: the ring each leaves holds the f32 tile.  The per-fragment epilogue that kernel once fell back to (split3_epilogue4) was
    reached by no instantiation and is removed."""
    split3_site(M, N, K, f"gemm_split3.hip generic row epilogue of the plane-fed kernel {M}x{N}x{K}", plane_fed=True)


def split3_pro(Am, Wp, M, N, K, stat, gamma, beta, act):
    L = _L()
    out = torch.full((M, N), NAN, device="cuda")
    a = L.Split3Args()
    a.b_planes, a.ldb, a.M, a.N, a.K, a.C, a.ldc = Wp.data_ptr(), K, M, N, K, out.data_ptr(), N
    L.check(L.lib().gg_gemm_nt_split3_af32_pro(C.byref(a), Am.data_ptr(), Am.stride(0), 0, stat.data_ptr(), gamma.data_ptr(), beta.data_ptr(), act, None, L.stream()),
            "gg_gemm_nt_split3_af32_pro")
    torch.cuda.synchronize()
    return out


def test_split3_gemm_batchnorm_prologue():
    """gg_gemm_nt_split3_af32_pro at K = N = 384 with W = the planes of the identity: C = act(y), the three bf16 terms of act(y) summed back exactly -- but for results
    below the smallest normal f32, which the split product flushes to zero (``floor`` of tests/act_cases.py::gate)."""
    K = N = 384
    p = probes("P32")
    M = -(-p.numel() // K)
    y = chunks(p, M * K)[0].view(M, K)
    stat, gamma, beta = affine(K)
    Wp = planes_of(torch.eye(K, device="cuda"))
    w = Worst("gemm_split3.hip BatchNorm prologue K=384")
    for act in ("gelu", "quick"):
        w.add(split3_pro(y, Wp, M, N, K, stat, gamma, beta, ACT[act]), y, act, F32, floor=2.0 ** -126)
    w.report()


# ---- padding that is not zero after the transform -------------------------------------------------------------------------------------------------------------
def _padding_case(M, K, N, act):
    g = torch.Generator().manual_seed(M * 1000 + K + N)
    Am = torch.randn(M, K, generator=g)
    Wm = torch.randn(N, K, generator=g) / K ** 0.5
    return Am, Wm


def _padding_ref(Am, Wm, act, beta):
    z = Am.double() + beta
    return A.reference("gelu" if act == 1 else "quick", z) @ Wm.double().T


def test_bf16_prologue_padding_is_not_transformed(ops):
    """beta = 2: act(BN(0)) = GELU(2) = 1.95, so a K tail or row tail that went through the transform after it was zero-filled moves a result by about 0.17; M = 130,
    K = 136, N = 72 are ragged against every tile.  Gate: rtol = atol = 2e-2 of test_gemm_batchnorm_prologue, against the fp64 product of the fp64-transformed operand."""
    M, K, N = 130, 136, 72
    Am, Wm = _padding_case(M, K, N, 1)
    Am, Wm = Am.to(BF16), Wm.to(BF16)
    stat, gamma, beta = affine(K, 2.0)
    out = ops.conv_bn_prologue(Am.cuda(), stat, gamma, beta, Wm.cuda(), act="gelu").double().cpu()
    ref = _padding_ref(Am, Wm, 1, 2.0)
    err = (out - ref).abs()
    print(f"\n[bf16 prologue padding {M}x{K}x{N}] max err {float(err.max()):.3e}, max err / (2e-2 + 2e-2 |ref|) {float((err / (2e-2 + 2e-2 * ref.abs())).max()):.3f}")
    assert bool((err <= 2e-2 + 2e-2 * ref.abs()).all())


@pytest.mark.parametrize("K", [136, 392])
def test_f32_prologue_padding_is_not_transformed(ops, K):
    """The same on gg_gemm_nt_f32's prologues: the ring (K = 136) and the register-staged kernel (K = 392); gate rel-L2 2e-6 of test_split3_gemm_batchnorm_act_prologue."""
    M, N = 130, 72
    Am, Wm = _padding_case(M, K, N, 1)
    stat, gamma, beta = affine(K, 2.0)
    out = ops.conv_bn_prologue(Am.cuda(), stat, gamma, beta, Wm.cuda(), act="gelu").double().cpu()
    ref = _padding_ref(Am, Wm, 1, 2.0)
    e = float((out - ref).norm() / ref.norm())
    print(f"\n[f32 prologue padding {M}x{K}x{N}] rel-L2 {e:.3e}")
    assert e < 2e-6


@pytest.mark.parametrize("act", [1, 2])
def test_split3_prologue_padding_is_not_transformed(act):
    """gg_gemm_nt_split3_af32_pro at M = 130, N = 72, K = 392, GELU and QuickGELU; gate rel-L2 2e-6."""
    M, N, K = 130, 72, 392
    Am, Wm = _padding_case(M, K, N, act)
    stat, gamma, beta = affine(K, 2.0)
    out = split3_pro(Am.cuda(), planes_of(Wm.cuda()), M, N, K, stat, gamma, beta, act).double().cpu()
    ref = _padding_ref(Am, Wm, act, 2.0)
    e = float((out - ref).norm() / ref.norm())
    print(f"\n[split3 prologue padding {M}x{N}x{K} act {act}] rel-L2 {e:.3e}")
    assert e < 2e-6


# ---- conv.hip and conv_f32.hip --------------------------------------------------------------------------------------------------------------------------------
CONV_C, CONV_H = 64, 32


def conv_probes(dtype):
    """The probe set with |z| <= 2^100 (larger ones set to 0) as one (1, 32, 32, 64) image, and the same on the even pixels of a (1, 64, 64, 64) image of zeros."""
    key = ("conv", dtype)
    if key not in _CACHE:
        p = probes(PSET[dtype]).clone()
        p[p.double().abs() > 2.0 ** 100] = 0
        small = p.view(1, CONV_H, CONV_H, CONV_C).contiguous()
        big = torch.zeros(1, 2 * CONV_H, 2 * CONV_H, CONV_C, dtype=dtype, device="cuda")
        big[:, 0::2, 0::2] = small
        _CACHE[key] = (small, big)
    return _CACHE[key]


def conv_acts(dtype):
    """conv_f32.hip takes every activation code.  conv.hip's im2col refuses all but none / GELU and its depthwise kernels take a GELU flag; only
    gg_col2im_nhwc_bnbwd_bf16 passes the code on to gg_act_grad, so QuickGELU' is probed there too (test_conv_on_store_fusions)."""
    return ("gelu",) if dtype == BF16 else ("gelu", "quick")


def centre_taps():
    t = torch.zeros(9, CONV_C, device="cuda")
    t[4] = 1.0
    return t


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_conv_on_load_fusions(ops, dtype):
    """im2col_nhwc_bn (stride 2: the centre tap of output pixel (i, j) is input pixel (2i, 2j)) and dwconv3x3_fwd_fused at strides 1 and 2 with taps = centre 1: each
    returns act(BN(y)) = act(y) of the probes.  B = 1, C = 64, H = W = 32 (stride 1) or 64 with the probes on the even pixels (stride 2)."""
    small, big = conv_probes(dtype)
    stat, gamma, beta = affine(CONV_C)
    taps = centre_taps()
    w = Worst(f"conv on-load fusions {str(dtype)[6:]}")
    for act in conv_acts(dtype):
        code = "gelu" if act == "gelu" else "quick_gelu"
        col = ops.im2col_nhwc_bn(big, stat, gamma, beta, act=code, stride=2)
        w.add(col.view(CONV_H * CONV_H, 9, CONV_C)[:, 4], small, act, dtype)
        w.add(ops.dwconv3x3_fwd_fused(small, stat, gamma, beta, taps, act=code, stride=1, colstats=True)[0], small, act, dtype)
        w.add(ops.dwconv3x3_fwd_fused(big, stat, gamma, beta, taps, act=code, stride=2, colstats=True)[0], small, act, dtype)
    w.report()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_conv_on_store_fusions(ops, dtype):
    """dwconv3x3_bwd_data_fused (stride 1), dwconv3x3_s2_bwd_data_fused and col2im_nhwc_bnbwd with an upstream of 1 on the centre tap only: each returns
    act'(BN(ep_y)) = act'(y) at the probes (stride 2: on the even pixels; the odd ones get no upstream and must be 0).  gg_col2im_nhwc_bnbwd_bf16 hands its act code to
    gg_act_grad, so it is the one bf16 entry point here that is also run with QuickGELU'."""
    small, big = conv_probes(dtype)
    stat, gamma, beta = affine(CONV_C)
    taps = centre_taps()
    ones = torch.ones_like(small)
    dcol = torch.zeros(CONV_H * CONV_H, 9, CONV_C, dtype=dtype, device="cuda")
    dcol[:, 4] = 1.0
    dcol = dcol.view(CONV_H * CONV_H, 9 * CONV_C)
    w = Worst(f"conv on-store fusions {str(dtype)[6:]}")
    for act in conv_acts(dtype):
        code = "gelu" if act == "gelu" else "quick_gelu"
        ep = dict(ep_stat=stat, ep_gamma=gamma, ep_beta=beta, ep_act=code)
        w.add(ops.dwconv3x3_bwd_data_fused(ones, None, None, taps, ep_y=small, **ep)[0], small, act + "_grad", dtype)
        out = ops.dwconv3x3_s2_bwd_data_fused(ones, None, None, taps, 2 * CONV_H, 2 * CONV_H, ep_y=big, **ep)[0]
        w.add(out[:, 0::2, 0::2], small, act + "_grad", dtype)
        assert float(out[:, 1::2].abs().max()) == 0.0 and float(out[:, :, 1::2].abs().max()) == 0.0
        dz = ops.col2im_nhwc_bnbwd(dcol, big, stat, gamma, beta, act=code, nparts=64)[0]
        w.add(dz[:, 0::2, 0::2], small, act + "_grad", dtype)
        assert float(dz[:, 1::2].abs().max()) == 0.0 and float(dz[:, :, 1::2].abs().max()) == 0.0
    if dtype == BF16:
        dz = ops.col2im_nhwc_bnbwd(dcol, big, stat, gamma, beta, act="quick_gelu", nparts=64)[0]
        w.add(dz[:, 0::2, 0::2], small, "quick_grad", dtype)
    w.report()
