"""Probe sets, fp64 references, per-element gates and restated forms for the activation functions of csrc/common.h (GELU, GELU', QuickGELU, QuickGELU')
and for the sites that evaluate them.  Plain torch on the CPU: no GPU, no libgg.  The pattern is that of tests/contrastive_cases.py.

Probe sets (``probes(name)``), each a flat tensor of exactly 65 536 = 512 x 128 values:

* ``P16``        all 65 280 finite bf16 values (bit patterns in order), padded with zeros
* ``P16H``       all 63 488 finite fp16 values, padded with zeros
* ``P32``        f32: the bf16 values with |z| <= 16; the 257 consecutive f32 values centred on each of 0, +-0.75179 (GELU' = 0), +-4.2426407 (3 sqrt 2, the erf clamp),
                 +-4.75 (the GELU' clamp), +-5.939697 (4.2 sqrt 2, the end of the Phi fit) and +-1/1.702; +-2^k for k = -149 .. 127; the grid of step 2^-9 on
                 [-16, 16] shifted by 2^-9 / pi; padded with zeros
* ``NONFINITE``  multiples of 1/8 in [-8, 8) (exact in bf16, fp16 and f32) with +inf, -inf, NaN in turn at every 7th position from 3: 7 is odd, so the non-finite
                 values fall on even and on odd lanes of a pair and on every position of an 8-chunk, and every one of them has finite neighbours on both sides
* ``P8``         (``p8()``) the 254 finite e4m3 codes and the 15 row scales 2^-10 .. 2^4 of the fp8 site

fp64 references (``reference(kind, z)``): Phi(z) = erfc(-z / sqrt 2) / 2 through torch.special.erfc (never 1 + erf), GELU = z Phi, GELU' = Phi + z phi,
QuickGELU = z sigma(1.702 z), QuickGELU' = sigma + 1.702 z sigma (1 - sigma), sigma(t) = 1 / (1 + exp(-t)).

Gates (``gate(form, store, z, ref)``), per element, never a tensor maximum; u is the upstream factor (1 in every probe), r_T the half-ulp of the storage type
(2^-8 bf16, 2^-11 fp16, 2^-24 f32; bf16 has 8 significand bits, so its half-ulp is 2^-8 of the value at worst -- with 2^-9 the correctly rounded result of an exact
form misses the gate by a factor 1.96):

    |err| <= |u| E(z) + r_T (|u ref| + |u| E(z)) + s_T [|u ref| below the smallest normal of T]

s_T is half the smallest subnormal of T (2^-25 fp16, 2^-134 bf16, 2^-150 f32): below the normal range the storage type rounds absolutely, not relatively (at
z = 2^-149 GELU is z / 2, which f32 cannot hold: the nearest results, 0 and 2^-149, are both 2^-150 away).
``floor`` replaces s_T by 2^-126 at the one site where a split-bf16 product FOLLOWS the activation (gg_gemm_nt_split3_af32_pro): that product flushes f32
subnormals to zero, as the pre-activation copies of the split GEMM's own epilogues show (a subnormal probe arrives as 0), so a result below the smallest normal may be 0.

* ``gelu16``        E = GELU16_BOUND = 4.7e-5, the statement of common.h for gg_gelu / gg_gelu_v2, corrected from 4.4e-5.  The polynomial crosses 1 near u = 3 and where
                    exactly depends on the rounding of each step (fused or not), so the clamp may set in anywhere from the fit edge on: there the error of erf is
                    1 - erf(3) = 2.209e-5 (stated now as 2.3e-5, was 2.1e-5) and that of GELU 3 sqrt 2 / 2 times as much, 4.686e-5.  The restatement reaches 2.15e-5 and
                    4.57e-5 at z = 4.2487 with fused multiply-adds and 2.14e-5 / 4.52e-5 without
* ``gelu_grad16``   E = GELU_GRAD16_BOUND = 1.2e-5, the statement of common.h for gg_gelu_grad_v2
* ``gelu32``        E = (7.3e-8 + 2^-24) |z| (the stated Phi error plus one ulp of v_exp_f32 on h <= 1/2, from the ISA manual's stated accuracy, not measured),
                    and where |ref| > 1e-3 also |err| <= 4e-6 |ref|: the smaller of the two holds
* ``gelu_grad32``   E = gelu_grad32_sup() + 2^-22: common.h states no bound; the supremum of the restatement against fp64 over P32, computed when the gate is first
                    used (1.14e-7 at z = 0.75179; 1.40e-7 without fused multiply-adds; tests/test_act_cases_cpu.py prints and pins it), plus one ulp of each of the two
                    exponentials
* ``quick``, ``quick_grad``   E = 1e-6 (|z| + 1), the term tests/test_gpu_fp8_kernels.py grants the device exponential

Non-finite (``check``): a finite argument must give a finite result.  GELU and QuickGELU: NaN -> NaN, +inf -> +inf, -inf -> NaN (what torch's f32 CPU op gives);
the derivatives: NaN -> NaN, at +-inf either NaN or the limit (1 / 0) within E.

Restated forms (``restated(form, x, defect=None)``): each common.h form in float32 with the fused multiply-add emulated (product and sum in float64, rounded once)
and exp2 / exp / rcp correctly rounded.  They exist to check the stated bounds and the defect list on the CPU; no GPU result is ever compared with them.

* ``erf16``          gg_erf_sqrt2              ``gelu16``       gg_gelu            ``gelu16_v2``     gg_gelu_v2           ``gelu_grad16``   gg_gelu_grad_v2
* ``phi32``          gg_phi_f32(_v2)           ``gelu32``       gg_gelu_f32        ``gelu_grad32``   gg_gelu_grad_f32(_v2)
* ``quick16``        gg_quick_gelu (rcp)       ``quick32``      x / (1 + exp)      ``quick_grad16`` / ``quick_grad32``   s + 1.702 clamp(x) s (1 - s)

``DEFECTS``: a restated form with one fault each, (form, gate, storage type, probe set); tests/test_act_cases_cpu.py shows every one rejected by the gates:

* ``tanh_gelu``      tanh-GELU in place of erf                     * ``no_erf_clamp``    the erf clamp missing
* ``grad_clamp_4``   the GELU' clamp at 4.0                        * ``const_1_7``       1.7 for 1.702
* ``form16_at_f32``  the 16-bit form at an f32 site                * ``one_plus_erf``    0.5 (1 + erf) at an f32 site
* ``pair_lane``      the odd lane of a pair at the even lane's argument
* ``no_zphi``        GELU' without its z phi term                  * ``sign_dropped``    the sign dropped for z < 0

Measured by tests/test_act_cases_cpu.py (`pytest -s`), restatement against fp64 over P16 u P32, fused / unfused: erf 2.15e-5 / 2.14e-5, GELU16 4.57e-5 / 4.52e-5 (gg_gelu_v2
4.57e-5 both ways), GELU'16 1.16e-5 / 1.16e-5, Phi32 6.6e-8 / 6.8e-8, GELU32 relative 3.1e-6 where |GELU| > 1e-3, GELU'32 1.14e-7 / 1.40e-7.  QuickGELU' without the clamp of
its product term (``no_grad_clamp``: 1.702 x overflows for |x| > 2e38 and inf * 0 is NaN) gives NaN at 210 finite values of P16.
"""
import contextlib
import functools
import math

import torch

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
N_PROBES = 65536
ROWS, COLS = 512, 128
ERF16_BOUND = 2.3e-5
GELU16_BOUND = 4.7e-5
GELU_GRAD16_BOUND = 1.2e-5
PHI32_BOUND = 7.3e-8
GELU32_REL, GELU32_REL_FROM = 4e-6, 1e-3
QUICK_C = 1.702
HALF_ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
MIN_NORMAL = {BF16: 2.0 ** -126, F16: 2.0 ** -14, F32: 2.0 ** -126}
HALF_SUBNORMAL = {BF16: 2.0 ** -134, F16: 2.0 ** -25, F32: 2.0 ** -150}
CENTRES = (0.75179, 4.2426407, 4.75, 5.939697, 1.0 / 1.702)
KINDS = ("gelu", "gelu_grad", "quick", "quick_grad")


# ---- probe sets -----------------------------------------------------------------------------------------------------------------------------------------------
def _pad(v, dtype):
    v = v.to(dtype)
    assert v.numel() <= N_PROBES, v.numel()
    out = torch.zeros(N_PROBES, dtype=dtype)
    out[:v.numel()] = v
    return out


def _all_finite_16(dtype):
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    return v[torch.isfinite(v.float())]


def _around(c):
    """The 257 consecutive f32 values centred on c >= 0 (and on 0: -128 .. 128 times the smallest subnormal)."""
    if c == 0.0:
        return (torch.arange(-128, 129, dtype=F64) * 2.0 ** -149).float()
    bits = torch.tensor([c], dtype=F32).view(torch.int32) + torch.arange(-128, 129, dtype=torch.int32)
    return bits.view(F32)


@functools.lru_cache(maxsize=None)
def probes(name):
    if name == "P16":
        return _pad(_all_finite_16(BF16), BF16)
    if name == "P16H":
        return _pad(_all_finite_16(F16), F16)
    if name == "P32":
        b = _all_finite_16(BF16).float()
        parts = [b[b.abs() <= 16.0], _around(0.0)]
        for c in CENTRES:
            parts += [_around(c), -_around(c)]
        p2 = torch.exp2(torch.arange(-149, 128, dtype=F64)).float()
        parts += [p2, -p2]
        parts.append((torch.arange(-16 * 512, 16 * 512 + 1, dtype=F64) * 2.0 ** -9 + 2.0 ** -9 / math.pi).float())
        return _pad(torch.cat(parts), F32)
    if name == "NONFINITE":
        v = ((torch.arange(N_PROBES, dtype=F64) * 37) % 128 - 64) / 8.0
        v = v.float()
        pos = torch.arange(3, N_PROBES, 7)
        v[pos] = torch.tensor([math.inf, -math.inf, math.nan], dtype=F32)[torch.arange(pos.numel()) % 3]
        return v
    raise KeyError(name)


def probe_matrix(name, dtype=None):
    """The probe set as the 512 x 128 matrix the sites take, in its own type or (exactly representable) in ``dtype``."""
    p = probes(name).reshape(ROWS, COLS)
    if dtype is not None and p.dtype != dtype:
        q = p.to(dtype)
        assert torch.equal(q.double().nan_to_num(nan=7.5), p.double().nan_to_num(nan=7.5)), f"{name} is not exact in {dtype}"
        p = q
    return p.clone()


@functools.lru_cache(maxsize=None)
def p8():
    """(codes uint8 [254], values f64 [254], row scales f64 [15]) of the finite OCP e4m3 values."""
    codes = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    c = codes.to(torch.int64)
    s, e, m = (c >> 7) & 1, (c >> 3) & 15, (c & 7).double()
    mag = torch.where(e == 0, m / 8.0 * 2.0 ** -6, (1.0 + m / 8.0) * torch.exp2((e - 7).double()))
    return codes, torch.where(s == 1, -mag, mag), torch.exp2(torch.arange(-10, 5, dtype=F64))


# ---- fp64 references ------------------------------------------------------------------------------------------------------------------------------------------
def phi64(z):
    return 0.5 * torch.special.erfc(-z.double() / math.sqrt(2.0))


def reference(kind, z):
    z = z.double()
    if kind == "gelu":
        return z * phi64(z)
    if kind == "gelu_grad":
        return phi64(z) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    sg = torch.sigmoid(QUICK_C * z)
    if kind == "quick":
        return z * sg
    if kind == "quick_grad":
        return sg + QUICK_C * z * sg * (1.0 - sg)
    raise KeyError(kind)


KIND_OF = {"gelu16": "gelu", "gelu32": "gelu", "gelu_grad16": "gelu_grad", "gelu_grad32": "gelu_grad", "quick": "quick", "quick_grad": "quick_grad"}


def form_for(kind, store):
    """The gate a site of this storage type answers to: the 16-bit forms at bf16 / fp16 sites, the f32 forms at f32 sites."""
    if kind in ("quick", "quick_grad"):
        return kind
    return kind + ("32" if store == F32 else "16")


# ---- gates ----------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gelu_grad32_sup():
    """Supremum over P32 of |restated gg_gelu_grad_f32 - fp64|."""
    z = probes("P32")
    return float((restated("gelu_grad32", z).double() - reference("gelu_grad", z)).abs().max())


def form_bound(form, z):
    z = z.double()
    if form == "gelu16":
        return torch.full_like(z, GELU16_BOUND)
    if form == "gelu_grad16":
        return torch.full_like(z, GELU_GRAD16_BOUND)
    if form == "gelu32":
        return (PHI32_BOUND + 2.0 ** -24) * z.abs()
    if form == "gelu_grad32":
        return torch.full_like(z, gelu_grad32_sup() + 2.0 ** -22)
    if form in ("quick", "quick_grad"):
        return 1e-6 * (z.abs() + 1.0)
    raise KeyError(form)


def gate(form, store, z, ref, u=1.0, floor=0.0):
    u = abs(u)
    E, a = u * form_bound(form, z), u * ref.abs()
    g = E + HALF_ULP[store] * (a + E) + (a < MIN_NORMAL[store]).double() * max(HALF_SUBNORMAL[store], floor)
    if form == "gelu32":
        g = torch.where(ref.abs() > GELU32_REL_FROM, torch.minimum(g, GELU32_REL * a), g)
    return g


def check(got, z, form, store, u=1.0, floor=0.0):
    """(worst err / gate over the finite arguments, index of it, list of violations of the finiteness classes)."""
    z64, got64 = z.double().flatten(), got.double().flatten()
    assert z64.numel() == got64.numel()
    kind = KIND_OF[form]
    fin = torch.isfinite(z64)
    zf = torch.where(fin, z64, torch.zeros_like(z64))
    ref = u * reference(kind, zf)
    g = gate(form, store, zf, ref / u if u else ref, u, floor)
    bad = []
    nf = fin & ~torch.isfinite(got64)
    if nf.any():
        i = int(nf.nonzero()[0])
        bad.append(f"{int(nf.sum())} finite arguments gave a non-finite result, first z = {float(z64[i])!r} at {i} -> {float(got64[i])!r}")
    ratio = torch.where(fin & ~nf, (got64 - ref).abs() / g, torch.zeros_like(g))
    nan_in, pinf, ninf = torch.isnan(z64), z64 == math.inf, z64 == -math.inf
    if (nan_in & ~torch.isnan(got64)).any():
        bad.append("NaN argument gave a number")
    if kind in ("gelu", "quick"):
        if (pinf & (got64 != math.inf)).any():
            bad.append("+inf did not give +inf")
        if (ninf & ~torch.isnan(got64)).any():
            bad.append("-inf did not give NaN")
    else:
        E = float(form_bound(form, torch.ones(1))[0])           # constant in z, but for QuickGELU': there the bound at |z| = 1
        for m, lim in ((pinf, 1.0), (ninf, 0.0)):
            tol = E + HALF_ULP[store] * (lim + E)
            wrong = m & ~torch.isnan(got64) & ~((got64 - lim).abs() <= tol)
            if wrong.any():
                bad.append(f"derivative at {'+' if lim else '-'}inf is neither NaN nor {lim}: {float(got64[int(wrong.nonzero()[0])])!r}")
    w = int(ratio.argmax())
    return float(ratio[w]), w, bad


def assert_inside(got, z, form, store, what, u=1.0):
    worst, w, bad = check(got, z, form, store, u)
    zw = float(z.double().flatten()[w])
    print(f"  {what}: {form} / {str(store).replace('torch.', '')}: worst err/gate {worst:.3f} at z = {zw!r}")
    assert not bad, f"{what}: " + "; ".join(bad)
    assert worst <= 1.0, f"{what}: {form} err/gate {worst:.3f} at z = {zw!r}, got {float(got.double().flatten()[w])!r}, ref {float(reference(KIND_OF[form], z.double().flatten()[w:w + 1])[0])!r}"
    return worst


# ---- restated forms (f32, fused multiply-add emulated) --------------------------------------------------------------------------------------------------------
def _c(v):
    return torch.tensor(v, dtype=F64).float()


_FUSED = [True]


@contextlib.contextmanager
def unfused():
    """Evaluate the restatements with every multiply-add as two rounded operations: what the compiler emits where it does not contract."""
    _FUSED[0] = False
    try:
        yield
    finally:
        _FUSED[0] = True


def _fma(a, b, c):
    a, b, c = (t if torch.is_tensor(t) else _c(t) for t in (a, b, c))
    if not _FUSED[0]:
        return a * b + c
    return (a.double() * b.double() + c.double()).float()


def _horner(coefs, t):
    p = _c(coefs[0]).expand_as(t)
    for c in coefs[1:]:
        p = _fma(p, t, c)
    return p


def _exp2(p):
    return torch.exp2(p.double()).float()


def _exp(p):
    return torch.exp(p.double()).float()


def _rcp(x):
    return (1.0 / x.double()).float()


ERF_COEFS = (3.912539981e-08, -1.883036475e-06, 4.008835822e-05, -5.029218737e-04, 4.196857568e-03, -2.499890141e-02, 1.109308004e-01,
             -3.752196431e-01, 1.128250599e+00)
PHI_COEFS = (1.15539833e-05, -0.000152371736, 0.000845456321, -0.00226795045, 7.51803382e-05, 0.0277323835, -0.1483116, -0.918442011, -1.6279074, -1.0)
GRAD_COEFS = (-1.329242953e-02, 2.763605337e-02, -1.633125265e-02, 2.348791181e-02, -6.481112773e-02, 8.656523583e-02, -8.702833417e-02,
              8.773912323e-02, -8.319626930e-02, 7.598317362e-02, -8.164826059e-02, 1.501617604e-01)


def _erf16(x, clamp=True):
    u = x * _c(0.70710678118654752)
    pu = _horner(ERF_COEFS, u * u) * u
    return pu.clamp(-1.0, 1.0) if clamp else pu


def _phi32(x):
    tu = x.abs() * _c(0.70710678118654752)
    t = tu.clamp(max=float(_c(4.2)))
    p = _fma(tu - t, -12.2, _horner(PHI_COEFS, t))
    h = _exp2(p)
    return torch.where(x < 0, h, 1.0 - h)


def _gelu_grad16(x, clamp=4.75):
    u = x.clamp(-clamp, clamp)
    s = _fma(u * u, 8.864265928e-02, -1.0)
    return _fma(_horner(GRAD_COEFS, s), u, 0.5)


def _sigma(x, c, rcp):
    d = 1.0 + _exp(_c(-c) * x)
    return _rcp(d) if rcp else (1.0 / d.double()).float()


def _quick_grad(x, c, rcp, clamp=True):
    s = _sigma(x, c, rcp)
    xc = x.clamp(-1e30, 1e30) if clamp else x
    return _fma(_c(c) * xc * s, 1.0 - s, s)


def restated(form, x, defect=None):
    x = x.float()
    if defect == "sign_dropped":
        return restated(form, x.abs())
    if defect == "pair_lane":
        y = restated(form, x).clone().reshape(-1, 2)
        y[:, 1] = restated(form, x.reshape(-1, 2)[:, 0])
        return y.reshape(x.shape)
    if form == "erf16":
        return _erf16(x, clamp=defect != "no_erf_clamp")
    if form == "gelu16":
        if defect == "tanh_gelu":
            return _c(0.5) * x * (1.0 + torch.tanh(_c(0.7978845608028654) * _fma(_c(0.044715) * x * x, x, x)))
        return _c(0.5) * x * (1.0 + _erf16(x, clamp=defect != "no_erf_clamp"))
    if form == "gelu16_v2":
        h = x * _c(0.5)
        return _fma(h, _erf16(x, clamp=defect != "no_erf_clamp"), h)
    if form == "gelu_grad16":
        if defect == "no_zphi":
            return _c(0.5) * (1.0 + _erf16(x))
        return _gelu_grad16(x, clamp=4.0 if defect == "grad_clamp_4" else 4.75)
    if form == "phi32":
        return _phi32(x)
    if form == "gelu32":
        if defect == "form16_at_f32":
            return restated("gelu16", x)
        if defect == "one_plus_erf":
            return _c(0.5) * x * (1.0 + torch.special.erf(x.double() * math.sqrt(0.5)).float())
        return x * _phi32(x)
    if form == "gelu_grad32":
        if defect == "form16_at_f32":
            return _gelu_grad16(x)
        if defect == "no_zphi":
            return _phi32(x)
        return _fma(x * _c(0.3989422804014327), _exp2(x * x * _c(-0.72134752044448170)), _phi32(x))
    c = 1.7 if defect == "const_1_7" else QUICK_C
    if form == "quick16":
        return x * _sigma(x, c, True)
    if form == "quick32":
        return (x.double() / (1.0 + _exp(_c(-c) * x)).double()).float()
    if form in ("quick_grad16", "quick_grad32"):
        return _quick_grad(x, c, form == "quick_grad16", clamp=defect != "no_grad_clamp")
    raise KeyError(form)


# (restated form, gate, storage type, probe set): the faithful restatement must be inside its gate at every probe
FAITHFUL = (
    ("gelu16", "gelu16", BF16, "P16"), ("gelu16_v2", "gelu16", BF16, "P16"), ("gelu16", "gelu16", F16, "P16H"), ("gelu16_v2", "gelu16", F16, "P16H"),
    ("gelu16", "gelu16", F32, "P32"), ("gelu16_v2", "gelu16", F32, "P32"),
    ("gelu_grad16", "gelu_grad16", BF16, "P16"), ("gelu_grad16", "gelu_grad16", F16, "P16H"), ("gelu_grad16", "gelu_grad16", F32, "P32"),
    ("gelu32", "gelu32", F32, "P32"), ("gelu32", "gelu32", F32, "P16"), ("gelu_grad32", "gelu_grad32", F32, "P32"), ("gelu_grad32", "gelu_grad32", F32, "P16"),
    ("quick16", "quick", BF16, "P16"), ("quick16", "quick", F16, "P16H"), ("quick32", "quick", F32, "P32"), ("quick32", "quick", F32, "P16"),
    ("quick_grad16", "quick_grad", BF16, "P16"), ("quick_grad16", "quick_grad", F16, "P16H"), ("quick_grad32", "quick_grad", F32, "P32"),
    ("quick_grad32", "quick_grad", F32, "P16"),
)
# defect -> the (restated form, gate, storage type, probe set) it is shown on; every one must be rejected
DEFECTS = {
    "tanh_gelu": (("gelu16", "gelu16", BF16, "P16"),),
    "no_erf_clamp": (("gelu16", "gelu16", BF16, "P16"), ("gelu16_v2", "gelu16", BF16, "P16")),
    "grad_clamp_4": (("gelu_grad16", "gelu_grad16", BF16, "P16"),),
    "const_1_7": (("quick16", "quick", BF16, "P16"), ("quick32", "quick", F32, "P32"), ("quick_grad16", "quick_grad", BF16, "P16"),
                  ("quick_grad32", "quick_grad", F32, "P32")),
    "form16_at_f32": (("gelu32", "gelu32", F32, "P32"), ("gelu_grad32", "gelu_grad32", F32, "P32")),
    "one_plus_erf": (("gelu32", "gelu32", F32, "P32"),),
    "pair_lane": (("gelu16_v2", "gelu16", BF16, "P16"), ("gelu_grad16", "gelu_grad16", BF16, "P16"), ("gelu32", "gelu32", F32, "P32"),
                  ("gelu_grad32", "gelu_grad32", F32, "P32"), ("quick16", "quick", BF16, "P16"), ("quick_grad32", "quick_grad", F32, "P32")),
    "no_zphi": (("gelu_grad16", "gelu_grad16", BF16, "P16"), ("gelu_grad32", "gelu_grad32", F32, "P32")),
    "sign_dropped": (("gelu16", "gelu16", BF16, "P16"), ("gelu_grad16", "gelu_grad16", BF16, "P16"), ("gelu32", "gelu32", F32, "P32"),
                     ("gelu_grad32", "gelu_grad32", F32, "P32"), ("quick16", "quick", BF16, "P16"), ("quick_grad32", "quick_grad", F32, "P32")),
}


def stored(y, store):
    """The f32 result as the site stores it."""
    return y.to(store)
