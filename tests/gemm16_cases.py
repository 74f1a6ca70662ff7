"""Case table, exact operand family and exact references for the 16-bit NT GEMM (csrc/gemm.hip: gg_gemm_nt, gg_gemm_nt_f16) on every tile walk and k-loop form of its
two kernels.  Plain torch on the CPU: no GPU, no libgg.  The pattern is that of tests/act_cases.py.

Exact family.  A is ternary ({-1, 0, 1}, half of the entries nonzero), B integer in [-2, 2] (at K = 4096 with 15 of 16 entries zero, so that the product stays
within +-256: dense, its standard deviation would be 64), bias and residual integer in [-8, 8], row scales in {0, 1, 2} with
rows_per_scale = 77 (divides no tile height).  Every partial sum of A B^T is an integer far below 2^24, so a float32 matmul is the exact product in any summation
order, and every expected output is an integer of magnitude <= 256: exact in bf16 (8 significand bits) and in fp16.  The comparison with a kernel is therefore
torch.equal, with no tolerance.  ``expected()`` asserts these properties per case: f32 product == f64 product, |value| <= 256 for the plain result and for BOTH
roundings of the linear epilogue (rowscale * (z + bias) is rounded to the 16-bit type before + residual is added and rounded again).

Buffers (``padded`` / ``nan_out``).  Operands sit in buffers whose row pitch is 8 elements wider than the matrix (lda = K + 8, ldb = K + 8, ldr = ldc = N + 8); the
pad columns of A, B and the residual hold NaN, C and the pre-activation copy are pre-filled with NaN.  A k-chunk beyond K that leaks into the product, or a store
that is skipped or strays into the pad, shows as a NaN and not as a small error.

Case table (``CASES``).  Each case records the route gg_gemm_nt_route must report -- (kernel, tilesM, tilesN, group_m) -- without switches (``route``; per epilogue
where the dispatch depends on it, ``route_by_epi``) and, for the cases run under GG_DEV_SWITCHES=1 GG_GEMM_DMA_TILE=256, under that switch (``route256``), and its
k-form class (``kform``): nk = ceil(K / 64) stages, the steady pairs the LDS-DMA loop runs while s + 3 < nk, the tail of 2 or 3 stages behind them, and the
16-byte chunks of the K tail, (K % 64) / 8.

Epilogues (``EPIS``): ``plain`` and ``linear`` (bias, row scale, residual) run on every case, bit for bit.  ``gelu_pre`` (bias + GELU + pre-activation copy) and
``quick_pre`` return the pre-activation bit for bit and the activation inside the gate of tests/act_cases.py for a 16-bit site; ``quick`` (QuickGELU on the f32
accumulators) and ``dgelu`` / ``dquick`` (x GELU' / x QuickGELU' of a second tensor, multiples of 1/8 in [-8, 8)) answer to the same gate with the exact product as
the upstream factor.  No tolerance is defined here.
"""
import collections
import functools
import math

import torch

from tests import act_cases as A

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
NAN = float("nan")
PAD = 8                        # extra elements of every row pitch
ROWS_PER_SCALE = 77            # divides none of 16, 96, 128, 192, 256
MAX_EXACT = 256                # integers up to here are exact in bf16 and fp16
SK = 64                        # contraction depth of a k-stage (both kernels)
LONG_K = 512                   # beyond this K the B operand is thinned (operands())

# route codes of include/gg.h (GG_GEMM_ROUTE_*)
R128, R64, DMA192, DMA256 = 0, 1, 2, 3
ROUTE_NAME = {R128: "register-staged 128 x 128", R64: "register-staged 128 x 64", DMA192: "LDS-DMA 192 x 128", DMA256: "LDS-DMA 256 x 256"}
TILE = {R128: (128, 128), R64: (128, 64), DMA192: (192, 128), DMA256: (256, 256)}
WAVE = {R128: (64, 64), R64: (32, 64), DMA192: (96, 64), DMA256: (128, 64)}          # a wave's sub-tile (rows, columns)
ACT_CODE = {"gelu": 1, "quick": 2}
EPIS = ("plain", "linear", "gelu_pre", "quick_pre", "quick", "dgelu", "dquick")
EXACT_EPIS = ("plain", "linear")

KForm = collections.namedtuple("KForm", "nk pairs tail tail_chunks")
Case = collections.namedtuple("Case", "name M N K epis route route_by_epi route256 kform")


def kform(K):
    """(stages, steady pairs, tail stages, chunks of the K tail) of the LDS-DMA k-loop: `for (s = 0; s + 3 < nk; s += 2)` runs the pairs, the rest is the tail."""
    nk = -(-K // SK)
    pairs = len(range(0, max(nk - 3, 0), 2))
    return KForm(nk, pairs, nk - 2 * pairs, (K % SK) // 8)


def _case(name, M, N, K, route, *, extra=(), route_by_epi=None, route256=None):
    return Case(name, M, N, K, EXACT_EPIS + tuple(extra), route, route_by_epi or {}, route256, kform(K))


K_SWEEP = (192, 200, 224, 232, 248, 256, 320, 384, 448, 456)          # nk 3 .. 8; tails of 1, 4, 5 and 7 chunks; a 1-chunk tail behind three steady pairs
K_SWEEP_256 = (192, 200, 232, 320, 384, 4096)
ACT_EXTRA = ("gelu_pre", "quick_pre", "quick", "dgelu", "dquick")


def _table():
    t = []
    # LDS-DMA 192 x 128 at M = 1030, N = 200: 6 x 2 tiles, the last M tile has 70 rows (its second wave row is empty), the last N tile 72 columns
    for K in K_SWEEP:
        t.append(_case(f"dma192_1030x200x{K}", 1030, 200, K, (DMA192, 6, 2, 0), extra=("gelu_pre",) if K == 232 else ()))
    t.append(_case("dma192_1030x256x4096", 1030, 256, 4096, (DMA192, 6, 2, 0)))                          # 64 stages
    # tile walks of the 192 x 128 form: 10 x 10 tiles in groups of 8 M-tiles, a last group of 2, 100 tiles (no multiple of the 8 XCDs), ragged N; 9 exact N tiles + K tail
    t.append(_case("dma192_walk_1736x1224x192", 1736, 1224, 192, (DMA192, 10, 10, 8)))
    t.append(_case("dma192_walk_1736x1152x264", 1736, 1152, 264, (DMA192, 10, 9, 8)))
    # register-staged siblings below the DMA gate (M < 1024): 128 x 128 tiles, ragged second tile in M and N; one 128 x 64 case
    for K in K_SWEEP:
        t.append(_case(f"reg128_130x200x{K}", 130, 200, K, (R128, 2, 2, 0)))
    t.append(_case("reg128_130x256x4096", 130, 256, 4096, (R128, 2, 2, 0)))
    t.append(_case("reg64_130x64x200", 130, 64, 200, (R64, 2, 1, 0)))
    # LDS-DMA 256 x 256 by the dispatch's own rule (GELU + pre-activation copy, N >= 1536, 86 x 6 = 516 >= 512 tiles); the other epilogues of this shape take 192 x 128
    t.append(_case("dma256_natural_22016x1536x192", 22016, 1536, 192, (DMA192, 115, 12, 8), extra=("gelu_pre",), route_by_epi={"gelu_pre": (DMA256, 86, 6, 4)}))
    # LDS-DMA 256 x 256 under GG_GEMM_DMA_TILE=256: 5 x 2 tiles, the last M tile has 6 rows; group_m = 4 with a last group of 2
    for K in K_SWEEP_256:
        t.append(_case(f"dma256_1030x512x{K}", 1030, 512, K, (DMA192, 6, 4, 0), route256=(DMA256, 5, 2, 0), extra=ACT_EXTRA if K == 200 else ()))
    t.append(_case("dma256_walk_1290x1280x256", 1290, 1280, 256, (DMA192, 7, 10, 8), route256=(DMA256, 6, 5, 4)))
    return tuple(t)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FORCED_256 = tuple(c for c in CASES if c.route256 is not None)
NATURAL = tuple(c for c in CASES if c.route256 is None)
M1030 = tuple(c for c in CASES if c.M == 1030)                        # rerun on the register-staged kernel under GG_GEMM_DMA=0


def natural_route(case, epi):
    return case.route_by_epi.get(epi, case.route)


def grid_of(kernel, M, N):
    """(tilesM, tilesN, group_m) of a kernel's tile grid: ceil division by its tile, groups of 8 (192 x 128) / 4 (256 x 256) M-tiles beyond that many N tiles."""
    bm, bn = TILE[kernel]
    tm, tn = -(-M // bm), -(-N // bn)
    g = {DMA192: 8, DMA256: 4}.get(kernel, 0)
    return tm, tn, (g if g and tn > g else 0)


def reg_route(case):
    """The route of a case with the LDS-DMA form switched off (GG_GEMM_DMA=0)."""
    rem = case.N % 128
    k = R64 if case.N <= 64 or (rem != 0 and rem <= 64) else R128
    return (k,) + grid_of(k, case.M, case.N)


def coverage(kernel, under_switch):
    """The classes of k-form and tile walk that the table runs on one LDS-DMA geometry: a set of strings."""
    got = set()
    for c in CASES:
        routes = [c.route256] if under_switch else [natural_route(c, e) for e in c.epis]
        for r in routes:
            if r is None or r[0] != kernel:
                continue
            kf = c.kform
            got.add("pairs:" + ("0" if kf.pairs == 0 else "1" if kf.pairs == 1 else "2+"))
            got.add(f"tail:{kf.tail}")
            got.add("chunks:" + ("0" if kf.tail_chunks == 0 else "1-4" if kf.tail_chunks <= 4 else "5-7"))
            tm, tn, g = r[1:]
            got.add("group_m:off" if g == 0 else "group_m:partial" if tm % g else "group_m:whole")
    return got


REQUIRED_COVERAGE = {"pairs:0", "pairs:1", "pairs:2+", "tail:2", "tail:3", "chunks:0", "chunks:1-4", "chunks:5-7", "group_m:off", "group_m:partial"}


# ---- operands -------------------------------------------------------------------------------------------------------------------------------------------------
def _seed(case):
    return (case.M * 1000003 + case.N * 1009 + case.K) % (2 ** 31)


@functools.lru_cache(maxsize=4)
def operands(name):
    """The exact family for one case, f32 on the CPU: A [M, K], B [N, K], bias [N], residual [M, N], rowscale [ceil(M / 77)], second [M, N] (dact_preact)."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(c))
    Am = ((torch.rand(c.M, c.K, generator=g) < 0.5).float() * (torch.randint(0, 2, (c.M, c.K), generator=g).float() * 2 - 1))
    Bm = torch.randint(-2, 3, (c.N, c.K), generator=g).float()
    if c.K > LONG_K:                              # 64 stages: keep one entry of B in 16, or the product (sigma 64 at K = 4096) leaves the integers bf16 holds
        Bm = Bm * (torch.rand(c.N, c.K, generator=g) < 1.0 / 16).float()
    bias = torch.randint(-8, 9, (c.N,), generator=g).float()
    res = torch.randint(-8, 9, (c.M, c.N), generator=g).float()
    rs = torch.randint(0, 3, (-(-c.M // ROWS_PER_SCALE),), generator=g).float()
    second = (torch.randint(-64, 64, (c.M, c.N), generator=g).float() / 8.0) if any(e in ("dgelu", "dquick") for e in c.epis) else None
    return dict(A=Am, B=Bm, bias=bias, residual=res, rowscale=rs, second=second)


def _assert_exact(x, what):
    m = float(x.abs().max())
    assert m <= MAX_EXACT and bool((x == x.round()).all()), f"{what}: not an integer of magnitude <= {MAX_EXACT} (max {m})"
    for dt in (BF16, F16):
        assert torch.equal(x.to(dt).float(), x), f"{what}: not exact in {dt}"


@functools.lru_cache(maxsize=4)
def expected(name):
    """Exact results of one case (f32): z = A B^T, plain = z, pre = z + bias, scaled = rowscale (z + bias), linear = scaled + residual.  Asserts the exactness
    properties the bit-for-bit comparison rests on."""
    c = BY_NAME[name]
    o = operands(name)
    z = o["A"] @ o["B"].t()
    assert torch.equal(z.double(), o["A"].double() @ o["B"].double().t()), f"{name}: the f32 product is not the f64 product"
    assert c.K * 2 < 2 ** 24                     # |a b| <= 2 per term: no partial sum, in any order, leaves the integers f32 holds exactly
    pre = z + o["bias"]
    scaled = o["rowscale"].repeat_interleave(ROWS_PER_SCALE)[:c.M, None] * pre
    linear = scaled + o["residual"]
    _assert_exact(z, f"{name} plain")
    _assert_exact(pre, f"{name} pre-activation")
    _assert_exact(scaled, f"{name} linear epilogue, first rounding: rowscale (z + bias)")
    _assert_exact(linear, f"{name} linear epilogue, second rounding: + residual")
    return dict(z=z, pre=pre, linear=linear)


TN_SHAPES = ((4099, 200, 136), (9000, 96, 432))          # gg_gemm_tn: several row splits with a ragged last one (gg_gemm_tn_splits), N and K ragged against 128


def tn_case(M, N, K):
    """dW[N, K] = dY[M, N]^T X[M, K] on the exact family (dY ternary, X integer in [-2, 2]): the f32 result is exact in any order and any split of the rows."""
    g = torch.Generator().manual_seed((M * 1000003 + N * 1009 + K) % (2 ** 31))
    dY = ((torch.rand(M, N, generator=g) < 0.5).float() * (torch.randint(0, 2, (M, N), generator=g).float() * 2 - 1))
    X = torch.randint(-2, 3, (M, K), generator=g).float()
    want = dY.t() @ X
    assert torch.equal(want.double(), dY.double().t() @ X.double()) and M * 2 < 2 ** 24
    assert torch.equal(dY.to(BF16).float(), dY) and torch.equal(X.to(BF16).float(), X)
    return dY, X, want


# ---- buffers --------------------------------------------------------------------------------------------------------------------------------------------------
def padded(x, dtype, device="cpu"):
    """x [R, C] in a buffer [R, C + PAD] whose pad columns hold NaN; returns the buffer (the matrix is buf[:, :C], row pitch C + PAD)."""
    buf = torch.full((x.shape[0], x.shape[1] + PAD), NAN, dtype=dtype, device=device)
    buf[:, :x.shape[1]] = x.to(device=device, dtype=dtype)
    return buf


def nan_out(M, N, dtype, device="cpu"):
    return torch.full((M, N + PAD), NAN, dtype=dtype, device=device)


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------------------------
def locate(idx, N, kernel):
    """Where a flat index of an M x N result sits in the kernel's tiling: a description for failure messages."""
    m, n = idx // N, idx % N
    (bm, bn), (wr, wc) = TILE[kernel], WAVE[kernel]
    return f"element ({m}, {n}): tile (tm {m // bm}, tn {n // bn}), wave row {(m % bm) // wr}, wave column {(n % bn) // wc}, tile-local ({m % bm}, {n % bn})"


def assert_bits(got, want, kernel, what):
    """got [M, N] (16-bit, any device) equals want (f32, exact) bit for bit; the message names the first bad element's tile, wave row / column and whether it is NaN."""
    if torch.equal(got.float(), want.to(got.device)):
        return
    g, want = got.float().cpu(), want.cpu()
    bad = ~(g == want)                                                 # (a NaN is never equal)
    i = int(bad.flatten().nonzero()[0])
    nn = int(torch.isnan(g).sum())
    raise AssertionError(f"{what} [{ROUTE_NAME[kernel]}]: {int(bad.sum())} of {g.numel()} elements differ ({nn} NaN); first at {locate(i, g.shape[1], kernel)}: "
                         f"got {float(g.flatten()[i])!r}{' (NaN)' if math.isnan(float(g.flatten()[i])) else ''}, exact {float(want.flatten()[i])!r}")


def assert_pad_nan(buf, N, what):
    assert bool(torch.isnan(buf[:, N:]).all()), f"{what}: the pad columns of the output were written"


def assert_act_gate(got, z, kind, store, what, upstream=None):
    """got = u act(z) inside the per-element gate of tests/act_cases.py for a 16-bit site (u: the exact upstream factor, 1 when None); z finite."""
    form = A.form_for(kind, store)
    z64, got64 = z.double().to(got.device).flatten(), got.double().flatten()              # (on the device the result is on)
    u = torch.ones_like(z64) if upstream is None else upstream.double().to(got.device).flatten()
    ref = A.reference(A.KIND_OF[form], z64)
    gate = A.gate(form, store, z64, ref, u)
    ratio = (got64 - u * ref).abs() / gate
    ratio = torch.where(torch.isfinite(got64), ratio, torch.full_like(ratio, math.inf))
    w = int(ratio.argmax())
    worst = float(ratio[w])
    print(f"  {what}: {form} worst err/gate {worst:.3f} at z = {float(z64[w])!r}, u = {float(u[w])!r}")
    assert worst <= 1.0, f"{what}: {form} err/gate {worst:.3f} at flat index {w}: z = {float(z64[w])!r}, u = {float(u[w])!r}, got {float(got64[w])!r}, fp64 {float(u[w] * ref[w])!r}"
    return worst
