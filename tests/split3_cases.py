"""Case table, exact operand families and exact references for the split-bf16 GEMMs (csrc/gemm_split3.hip: gg_gemm_nt_split3_ex, gg_gemm_nt_split3_af32 / _stats /
_pro, gg_gemm_tn_split3, gg_split3_bf16) on every tile form, k-loop form and plane product of their four kernels.  Plain torch on the CPU: no GPU, no libgg.  The
pattern is that of tests/gemm16_cases.py.

The split.  ``split3`` restates gg_split3_rne (csrc/common.h): a = bf16(clamp(x, +-BF16_MAX)), b = bf16(x - a), c = bf16(x - a - b), all round-to-nearest-even (the
clamp passes over a NaN, which then lives in b and c).  A split GEMM adds the six products a1 b1, a1 b2, a2 b1, a1 b3, a2 b2, a3 b1 in f32.

Exact families.  Integers sit entirely in the first plane, so the operands carry wide significands; the sums stay exact because ONE operand is sparse: in every block
of 16 rows every 8-element chunk of the contraction holds exactly one non-zero (row r of the block owns the chunks c = r mod 16, at a random place inside the chunk), so
every 16 x 8 operand fragment of every MFMA carries a term, and a row of K = 1544 holds 13 terms.
  w3s1   wide +-m 2^-18, m uniform in [2^18, 2^19) (19-bit significands, |x| in [1, 2): three planes) times sparse +-1: products a1 b1, a2 b1, a3 b1
  s1w3   the mirror image (sparse +-1 on the A side, wide on the B side): a1 b1, a1 b2, a1 b3
  w2w2   dense +-m 2^-8, m < 2^10 times sparse +-j 2^-8, 2^8 <= j < 2^9 (two planes each, third plane zero): a1 b1, a1 b2, a2 b1, a2 b2
  int    ternary times sparse +-1: the plain integer family (one plane), for the column statistics
``expected`` asserts per case, as conditions and not as measurements: (1) sum_k (|a1| + |a2| + |a3|)(|b1| + |b2| + |b3|) / granule < 2^23 (granule 2^-18, 2^-18,
2^-16, 1; this bounds sum_k |a_k| |b_k| of the operands from above) -- every plane is a multiple of the granule, so every partial sum of every plane product, in any
order, is a multiple of the granule below 2^23 granules: exact in f32; (2) the f32 product equals the f64 product; (3) the planes sum to the operand exactly; (4) at
least 0.4 of the wide operand's elements have a non-zero third plane (w2w2: second plane, 0.4 dense, 0.2 among the sparse non-zeros); (5) every 16 x 8 block of the
sparse operand holds a non-zero.  Bias and residual are integers in [-8, 8], row scales in {0, 1, 2} with rows_per_scale = 77; the "linear" epilogue
(acc + bias) * scale + residual must satisfy (1) again, (sum_k |a_k| |b_k| + |bias|) * scale + |residual| < 2^23 granules, which is why it runs at K <= 256 on the wide
families and on w2w2 beyond; acc + bias alone only has to be an f32 (asserted as such).

Buffers.  Every row pitch is PAD = 8 elements wider than the matrix (dY: 4); pad columns of operands hold NaN, outputs are pre-filled with NaN.  For the TN kernel the
allocation continues with 8 NaN rows behind row M - 1, the row-scale array with NaN entries behind index (M - 1) / rows_per_scale.

No tolerance is defined here: every comparison is bit for bit, the activations answer to the f32-site gate of tests/act_cases.py.
"""
import collections
import functools
import math

import torch

from tests import act_cases as A

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NAN = float("nan")
PAD = 8
ROWS_PER_SCALE = 77                      # divides none of 32, 64, 128, 256
BF16_MAX = 3.3895313892515355e38         # GG_BF16_MAX_F: the clamp of the first plane
SK = 32                                  # contraction depth of a k-stage (all four kernels)
GRANULE = {"w3s1": 2.0 ** -18, "s1w3": 2.0 ** -18, "w2w2": 2.0 ** -16, "int": 1.0}
FAMS = ("w3s1", "s1w3", "w2w2")

# route codes of include/gg.h (GG_SPLIT3_ROUTE_*)
PL256, PL128, A256, A128 = 0, 1, 2, 3
ROUTE_NAME = {PL256: "plane-fed 256 x 128, two-stage ring", PL128: "plane-fed 128 x 128, three-stage ring", A256: "af32 256-row", A128: "af32 128-row"}
TILE_M = {PL256: 256, PL128: 128, A256: 256, A128: 128}
ACT_CODE = {"gelu": 1, "quick": 2}
EPI_CLASS = {"plain": 1, "bias": 1, "gelu_pre": 2, "dgelu": 3, "linear": 4, "quick_pre": 5, "dquick": 6, "planes": 0, "stats": 0}
ACT_EPIS = ("gelu_pre", "dgelu", "quick_pre", "dquick")

Route = collections.namedtuple("Route", "kernel tile_n epilogue mapped tilesM tilesN lds_bytes")
Case = collections.namedtuple("Case", "name entry M N K fams epis natural group switched")      # natural / switched: (kernel, tile_n); group: (variable, value) or None


# ---- the split ------------------------------------------------------------------------------------------------------------------------------------------------
def split3(x):
    """gg_split3_rne on the CPU: three bf16 planes of an f32 tensor.  The clamp is the median of (x, -BF16_MAX, BF16_MAX) with the minNum / maxNum rule (fminf(fmaxf(..)),
    which is what v_med3_f32 computes): a NaN is passed over, so the first plane of a NaN is -BF16_MAX and the NaN itself sits in the second and third plane -- every
    product with it is still NaN (assert_planes_equal's callers check that the planes of a NaN sum to NaN)."""
    x = x.to(F32)
    a = torch.fmin(torch.fmax(x, torch.tensor(-BF16_MAX)), torch.tensor(BF16_MAX)).to(BF16)
    r1 = x - a.float()
    b = r1.to(BF16)
    c = (r1 - b.float()).to(BF16)
    return a, b, c


# ---- routes ---------------------------------------------------------------------------------------------------------------------------------------------------
def kform(K):
    """(stages, chunks of the K tail) of a k-loop: nk = ceil(K / 32), (K % 32) / 8."""
    return -(-K // SK), (K % SK) // 8


def lds_bytes(kernel, tile_n, K=0, pro=False):
    if kernel in (PL256, PL128):
        return 147456                                                   # 2 x 3 x (256 + 128) x 64 B = 3 x 6 x 128 x 64 B
    ring = 2 * 3 * (256 + tile_n) * 64 if kernel == A256 else 3 * (128 + 2 * tile_n) * 64
    return ring + (2 * (((K + 31) & ~31) + 3 * SK) * 4 if pro else 0)


def route_for(case, epi, kernel_width=None, no_ec=False):
    """The GgSplit3Route a (case, epilogue) must report on a kernel and tile width (default: the case's natural ones)."""
    kernel, tile_n = kernel_width or case.natural
    ec = 0
    if case.entry == "af32" and not no_ec and case.N % 8 == 0:
        ec = EPI_CLASS[epi]
    return Route(kernel, tile_n, ec, 0, -(-case.M // TILE_M[kernel]), -(-case.N // tile_n), lds_bytes(kernel, tile_n, case.K, case.entry == "pro"))


def natural_af32(N, K):
    """The dispatch rule of the A-as-f32 forms, restated: 256-row tiles from K = 384 on, 96-column tiles where they save a fifth of the columns."""
    w128, w96 = 1.0 - N / (-(-N // 128) * 128), 1.0 - N / (-(-N // 96) * 96)
    return (A256 if K >= 384 else A128, 96 if w128 - w96 >= 0.2 else 128)


def _case(name, entry, M, N, K, natural, *, fams=("w3s1",), epis=None, group=None, switched=None):
    if epis is None:
        epis = ("plain",) if entry in ("planes", "pro") else ("bias",)
    assert (group is None) == (switched is None)
    return Case(name, entry, M, N, K, tuple(fams), tuple(epis), natural, group, switched)


G_TILE256, G_TILE128 = ("GG_SPLIT3A_TILE", "256"), ("GG_SPLIT3A_TILE", "128")
G_BN96, G_BN128, G_NOEC = ("GG_SPLIT3A_BN", "96"), ("GG_SPLIT3A_BN", "128"), ("GG_SPLIT3_NO_EC", "1")
GROUPS = (G_TILE256, G_TILE128, G_BN96, G_BN128, G_NOEC)


def _table():
    t = []
    # plane-fed, two-stage ring (M > 128): nk 1, 2, 3, 4 with tails of 1, 2, 3, 0 chunks; 2 x 2 tiles, a last M tile of 4 rows, a last N tile of 8 columns
    for K, fams in ((8, FAMS + ("int",)), (48, ("s1w3",)), (88, ("w2w2",)), (128, ("w3s1",))):
        t.append(_case(f"pl256_260x136x{K}", "planes", 260, 136, K, (PL256, 128), fams=fams, epis=("plain", "linear") if K == 48 else ("plain",)))
    # 49 stages, 5 x 2 tiles (ragged: 6 rows, 80 columns); at K = 1544 the sparse operand's extent is a multiple of 16, or the folded last block doubles a row's terms
    t.append(_case("pl256_1030x208x1544", "planes", 1030, 208, 1544, (PL256, 128), fams=("w3s1", "w2w2")))
    t.append(_case("pl256_784x200x1544", "planes", 784, 200, 1544, (PL256, 128), fams=("s1w3",)))                       # 4 x 2 tiles, a last M tile of 16 rows
    t.append(_case("pl256_260x130x40", "planes", 260, 130, 40, (PL256, 128), epis=("plain", "planes")))                # N % 8 != 0: the scalar stores
    t.append(_case("pl256_260x200x40_act", "planes", 260, 200, 40, (PL256, 128), epis=ACT_EPIS))
    # plane-fed, three-stage ring (M <= 128): nk 1, 2, 3, 7 (the ring wraps twice), every tail
    for K, fams in ((8, ("w3s1",)), (48, ("w2w2",)), (88, ("s1w3",)), (224, FAMS + ("int",)), (232, ("w3s1",))):
        t.append(_case(f"pl128_70x136x{K}", "planes", 70, 136, K, (PL128, 128), fams=fams, epis=("plain", "planes") if K == 88 else ("plain",)))
    t.append(_case("pl128_6x72x40", "planes", 6, 72, 40, (PL128, 128)))                                             # a single partial tile
    # af32 256-row kernel, K >= 384: nk 12 / 13 with tails 0, 1, 3, 0; widths 128 (N = 200: last tile 72 columns) and 96 (N = 168: 72 columns); K = 1544
    for K in (384, 392, 408, 416):
        t.append(_case(f"a256_1030x200x{K}", "af32", 1030, 200, K, (A256, 128), fams=FAMS + ("int",) if K == 392 else ("w3s1",),
                       epis=("bias", "planes") if K == 408 else ("bias",)))
    t.append(_case("a256_1030x168x384", "af32", 1030, 168, 384, (A256, 96), fams=("s1w3",)))
    t.append(_case("a256_1030x168x392", "af32", 1030, 168, 392, (A256, 96), fams=("w3s1",)))
    t.append(_case("a256_1030x208x1544", "af32", 1030, 208, 1544, (A256, 128), fams=("w3s1", "w2w2")))
    t.append(_case("a256_784x200x1544", "af32", 784, 200, 1544, (A256, 128), fams=("s1w3",)))
    t.append(_case("a256_272x192x1544", "af32", 272, 192, 1544, (A256, 96), fams=("w3s1", "s1w3")))
    t.append(_case("a256_260x136x400", "af32", 260, 136, 400, (A256, 128), fams=("w2w2",), epis=("bias", "linear")))      # last N tile 8 columns; tail 2; class 4
    t.append(_case("a256_260x168x416_lin", "af32", 260, 168, 416, (A256, 96), fams=("w2w2",), epis=("linear",)))
    t.append(_case("a256_260x130x384", "af32", 260, 130, 384, (A256, 128), fams=("s1w3",), epis=("bias", "planes")))      # N % 8 != 0: generic epilogue, scalar stores
    t.append(_case("a256_300x200x384_act", "af32", 300, 200, 384, (A256, 128), epis=ACT_EPIS))
    t.append(_case("a256_520x1024x384", "af32", 520, 1024, 384, (A256, 128)))                                          # 3 x 8 = 24 tiles: a multiple of 8
    # ... under GG_SPLIT3A_TILE=256: nk 1, 2, 3 -- every look-ahead load is masked
    for K in (8, 40, 72):
        t.append(_case(f"a256s_260x200x{K}", "af32", 260, 200, K, (A128, 128), fams=FAMS if K == 40 else ("w3s1",), epis=("bias", "linear") if K == 40 else ("bias",),
                       group=G_TILE256, switched=(A256, 128)))
    t.append(_case("a256s_260x168x40", "af32", 260, 168, 40, (A128, 96), fams=("s1w3",), group=G_TILE256, switched=(A256, 96)))
    # af32 128-row kernel, K < 384: K = 8, 40, 96, 200, 376; widths 128 and 96; M = 130: a last M tile of 2 rows
    for K in (8, 40, 96, 200, 376):
        t.append(_case(f"a128_130x200x{K}", "af32", 130, 200, K, (A128, 128), fams=FAMS + ("int",) if K == 200 else ("w3s1",),
                       epis=("bias", "linear") if K == 40 else ("bias",)))
    t.append(_case("a128_130x168x40", "af32", 130, 168, 40, (A128, 96), fams=("w3s1", "s1w3"), epis=("bias", "linear")))
    t.append(_case("a128_130x168x200", "af32", 130, 168, 200, (A128, 96), fams=("w2w2",), epis=("bias", "linear", "planes")))
    t.append(_case("a128_6x72x40", "af32", 6, 72, 40, (A128, 128)))                                                    # a single partial tile
    t.append(_case("a128_130x130x40", "af32", 130, 130, 40, (A128, 128), epis=("bias", "linear", "planes")))             # N % 8 != 0
    t.append(_case("a128_130x136x376", "af32", 130, 136, 376, (A128, 128)))                              # a last N tile of 8 columns
    t.append(_case("a128_500x200x40", "af32", 500, 200, 40, (A128, 128)))                                              # 4 x 2 = 8 tiles
    t.append(_case("a128_1030x200x200", "af32", 1030, 200, 200, (A128, 128), fams=("w2w2",)))                            # 9 x 2 = 18 tiles; last M tile 6 rows
    t.append(_case("a128_130x200x200_act", "af32", 130, 200, 200, (A128, 128), epis=ACT_EPIS))
    # ... under GG_SPLIT3A_TILE=128: K = 1544
    t.append(_case("a128s_130x208x1544", "af32", 130, 208, 1544, (A256, 128), fams=("w3s1", "w2w2"), group=G_TILE128, switched=(A128, 128)))
    t.append(_case("a128s_144x200x1544", "af32", 144, 200, 1544, (A256, 128), fams=("s1w3",), group=G_TILE128, switched=(A128, 128)))
    t.append(_case("a128s_130x176x1544", "af32", 130, 176, 1544, (A256, 96), group=G_TILE128, switched=(A128, 96)))
    # the other width, forced: N = 576 on 96 columns, N = 192 on 128, N = 200 on 96 (a last tile of 8 columns), each af32 kernel
    t.append(_case("bn96_260x576x384", "af32", 260, 576, 384, (A256, 128), fams=("w3s1", "s1w3"), group=G_BN96, switched=(A256, 96)))
    t.append(_case("bn96_130x576x40", "af32", 130, 576, 40, (A128, 128), fams=("w3s1", "w2w2"), epis=("bias", "linear"), group=G_BN96, switched=(A128, 96)))
    t.append(_case("bn96_260x200x392", "af32", 260, 200, 392, (A256, 128), group=G_BN96, switched=(A256, 96)))
    t.append(_case("bn96_130x200x200", "af32", 130, 200, 200, (A128, 128), group=G_BN96, switched=(A128, 96)))
    t.append(_case("bn128_260x192x384", "af32", 260, 192, 384, (A256, 96), fams=("w3s1", "s1w3"), group=G_BN128, switched=(A256, 128)))
    t.append(_case("bn128_130x192x40", "af32", 130, 192, 40, (A128, 96), fams=("w3s1", "w2w2"), epis=("bias", "linear"), group=G_BN128, switched=(A128, 128)))
    # the generic epilogue in place of the classes: GG_SPLIT3_NO_EC=1
    t.append(_case("noec_260x200x384", "af32", 260, 200, 384, (A256, 128), fams=("w2w2",), epis=("bias", "linear") + ACT_EPIS, group=G_NOEC, switched=(A256, 128)))
    t.append(_case("noec_130x168x40", "af32", 130, 168, 40, (A128, 96), epis=("bias", "linear") + ACT_EPIS, group=G_NOEC, switched=(A128, 96)))
    # column statistics on the integer family: both af32 kernels, both widths
    for name, M, N, K, nat in (("stats_a256_1030x200x384", 1030, 200, 384, (A256, 128)), ("stats_a256_1030x168x392", 1030, 168, 392, (A256, 96)),
                               ("stats_a128_1030x200x40", 1030, 200, 40, (A128, 128)), ("stats_a128_300x168x200", 300, 168, 200, (A128, 96))):
        t.append(_case(name, "af32", M, N, K, nat, fams=("int",), epis=("stats",)))
    # BatchNorm prologue without activation (always the 256-row kernel): K = 384, 416, 1024; widths 96 and 128
    for M, N, K, w in ((260, 200, 384, 128), (260, 168, 416, 96), (300, 208, 1024, 128), (260, 96, 1024, 96), (1030, 168, 384, 96)):
        t.append(_case(f"pro_{M}x{N}x{K}", "pro", M, N, K, (A256, w)))
    return tuple(t)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
UNSWITCHED = tuple(c for c in CASES if c.group is None)


def in_group(group):
    return tuple(c for c in CASES if c.group == group)


def run_route(case, epi):
    """The route of a case where it is run: under its group's switch, or naturally."""
    return route_for(case, epi, case.switched, no_ec=case.group == G_NOEC)


def coverage():
    """The form classes the table runs: a set of strings (tests/test_split3_cases_cpu.py names the required ones)."""
    got = set()
    for c in CASES:
        kernel, tile_n = c.switched or c.natural
        nk, tail = kform(c.K)
        k = {PL256: "pl256", PL128: "pl128", A256: "a256", A128: "a128"}[kernel]
        sw = "/switched" if c.group in (G_TILE256, G_TILE128) else ""
        got.add(f"{k}:nk={nk if nk <= 3 else 'odd' if nk % 2 else 'even'}{sw}")
        if kernel == PL128 and nk >= 7:
            got.add("pl128:nk>=7")
        got.add(f"{k}:tail={tail}")
        got.add(f"{k}:w{tile_n}")
        if c.group in (G_BN96, G_BN128):
            got.add(f"{k}:w{tile_n}/forced")
        got.add(f"{k}:K={c.K}{sw}")
        tm, tn = -(-c.M // TILE_M[kernel]), -(-c.N // tile_n)
        last_m, last_n = c.M - (tm - 1) * TILE_M[kernel], c.N - (tn - 1) * tile_n
        if last_m < 64:
            got.add(f"{k}:last_m<64" + ("/single" if tm == 1 else ""))
        got.add(f"last_n={last_n}")
        tiles = tm * tn
        got.add("tiles<8" if tiles < 8 else "tiles%8==0" if tiles % 8 == 0 else "tiles>8,rem")
        for e in c.epis:
            if c.entry == "af32":
                r = run_route(c, e)
                got.add(f"{k}:{e}/class{r.epilogue}" + ("/noec" if c.group == G_NOEC else "/n%8" if c.N % 8 else ""))
            else:
                got.add(f"{k}:{c.entry}/{e}")
        for f in c.fams:
            got.add(f"{k}:{f}")
    return got


# ---- operands -------------------------------------------------------------------------------------------------------------------------------------------------
def sparse_mask(rows, L, g):
    """[rows, L] bool: in every block of 16 rows, every 8-element chunk of L holds exactly one True -- row (c mod 16) of the block (folded into a shorter last block)
    owns chunk c, at a random place inside the chunk."""
    nb, nc = -(-rows // 16), -(-L // 8)
    b, c = torch.meshgrid(torch.arange(nb), torch.arange(nc), indexing="ij")
    rb = torch.clamp(rows - 16 * b, max=16)
    r = 16 * b + (c % 16) % rb
    width = torch.clamp(L - 8 * c, max=8)
    col = 8 * c + torch.randint(0, 8, (nb, nc), generator=g) % width
    m = torch.zeros(rows, L, dtype=torch.bool)
    m[r.flatten(), col.flatten()] = True
    return m


def _sign(shape, g):
    return torch.randint(0, 2, shape, generator=g).float() * 2 - 1


def wide3(shape, g):
    return _sign(shape, g) * torch.randint(2 ** 18, 2 ** 19, shape, generator=g).float() * 2.0 ** -18


def family(fam, rows_d, rows_s, L, g, dense_first=True):
    """(dense [rows_d, L], sparse [rows_s, L]) of a family; for s1w3 the roles are the mirror image: the caller puts `sparse` on the A side."""
    if fam in ("w3s1", "s1w3"):
        dense = wide3((rows_d, L), g)
        sparse = _sign((rows_s, L), g)
    elif fam == "w2w2":
        dense = _sign((rows_d, L), g) * torch.randint(0, 2 ** 10, (rows_d, L), generator=g).float() * 2.0 ** -8
        sparse = _sign((rows_s, L), g) * torch.randint(2 ** 8, 2 ** 9, (rows_s, L), generator=g).float() * 2.0 ** -8
    else:
        assert fam == "int", fam
        dense = torch.randint(-1, 2, (rows_d, L), generator=g).float()
        sparse = _sign((rows_s, L), g)
    return dense, sparse * sparse_mask(rows_s, L, g).float()


def _seed(*v):
    s = 0
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31)
    return s


@functools.lru_cache(maxsize=3)
def operands(name, fam):
    """One (case, family), f32 on the CPU: A [M, K], B [N, K], bias [N], residual [M, N], rowscale [ceil(M / 77)], second [M, N] (dact_preact: multiples of 1 / 8),
    and for the prologue cases mean, rstd, gamma, beta [K] and A_fed = A - shift."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(c.M, c.N, c.K, FAMS.index(fam) if fam in FAMS else 7))
    if fam == "s1w3":
        Bm, Am = family(fam, c.N, c.M, c.K, g)
    else:
        Am, Bm = family(fam, c.M, c.N, c.K, g)
    o = dict(A=Am, B=Bm, bias=torch.randint(-8, 9, (c.N,), generator=g).float(), residual=torch.randint(-8, 9, (c.M, c.N), generator=g).float(),
             rowscale=torch.randint(0, 3, (-(-c.M // ROWS_PER_SCALE),), generator=g).float(),
             second=torch.randint(-64, 64, (c.M, c.N), generator=g).float() / 8.0)
    if c.entry == "pro":
        mean, beta = torch.randint(-2, 3, (c.K,), generator=g).float(), torch.randint(-2, 3, (c.K,), generator=g).float()
        gamma, rstd = torch.full((c.K,), 2.0), torch.full((c.K,), 0.5)
        scale = gamma * rstd
        shift = beta - mean * scale                                     # the loader's table: act(fmaf(v, scale, shift)) with scale = 1
        fed = Am - shift
        assert bool((scale == 1.0).all()) and torch.equal(fed.double(), Am.double() - shift.double()), f"{name}: A - shift is not representable"
        assert torch.equal(torch.addcmul(shift.expand_as(fed), fed, scale.expand_as(fed)), Am)
        o.update(mean=mean, rstd=rstd, gamma=gamma, beta=beta, A_fed=fed)
    return o


def _abs_planes(x):
    return sum(p.double().abs() for p in split3(x))


def assert_family(fam, dense, sparse, what):
    """Conditions (3), (4), (5) on one (dense, sparse) pair; (1) and (2) need the product and are asserted by the caller."""
    for x in (dense, sparse):
        p = split3(x)
        assert torch.equal(p[0].double() + p[1].double() + p[2].double(), x.double()), f"{what}: the planes do not sum to the operand"
    pd, ps = split3(dense), split3(sparse)
    nz = sparse != 0
    if fam in ("w3s1", "s1w3"):
        share = float((pd[2] != 0).float().mean())
        assert share >= 0.4, f"{what}: only {share:.3f} of the wide operand has a non-zero third plane"
        assert bool((ps[1] == 0).all()) and bool((sparse.abs()[nz] == 1).all())
    elif fam == "w2w2":
        sd, ss = float((pd[1] != 0).float().mean()), float((ps[1][nz] != 0).float().mean())
        assert sd >= 0.4 and ss >= 0.2, f"{what}: second-plane shares {sd:.3f} (dense), {ss:.3f} (sparse non-zeros)"
        assert bool((pd[2] == 0).all()) and bool((ps[2] == 0).all())
    else:
        assert bool((pd[1] == 0).all()) and bool((ps[1] == 0).all())
    rows, L = sparse.shape
    blk = torch.zeros(-(-rows // 16) * 16, -(-L // 8) * 8, dtype=torch.bool)
    blk[:rows, :L] = nz
    per = blk.view(blk.shape[0] // 16, 16, blk.shape[1] // 8, 8).sum((1, 3))
    assert bool((per == 1).all()), f"{what}: a 16 x 8 block of the sparse operand holds {int(per.min())} .. {int(per.max())} non-zeros"


def _is_f32(x64):
    return torch.equal(x64.float().double(), x64)


@functools.lru_cache(maxsize=3)
def expected(name, fam):
    """Exact results of one (case, family), f32: z = A B^T, pre = z + bias, linear = (z + bias) * rowscale + residual, planes = split3 of z, colstats.  Asserts the
    conditions the bit-for-bit comparison rests on (module docstring)."""
    c, o = BY_NAME[name], operands(name, fam)
    what, gr = f"{name}/{fam}", GRANULE[fam]
    dense, sparse = (o["B"], o["A"]) if fam == "s1w3" else (o["A"], o["B"])
    assert_family(fam, dense, sparse, what)
    z64 = o["A"].double() @ o["B"].double().t()
    z = o["A"] @ o["B"].t()
    assert torch.equal(z.double(), z64), f"{what}: the f32 product is not the f64 product"
    span = _abs_planes(o["A"]) @ _abs_planes(o["B"]).t()
    assert bool((span >= o["A"].double().abs() @ o["B"].double().abs().t()).all())
    worst = float(span.max()) / gr
    assert worst < 2 ** 23, f"{what}: condition 1 fails, sum |planes| / granule = 2^{math.log2(worst):.2f}"
    e = dict(z=z, span_log2=math.log2(max(worst, 1.0)))
    pre64 = z64 + o["bias"].double()
    assert _is_f32(pre64), f"{what}: acc + bias is not an f32"
    e["pre"] = pre64.float()
    if "linear" in c.epis:
        sc = o["rowscale"].double().repeat_interleave(ROWS_PER_SCALE)[:c.M, None]
        bound = (o["A"].double().abs() @ o["B"].double().abs().t() + o["bias"].double().abs()) * sc + o["residual"].double().abs()
        assert float(bound.max()) / gr < 2 ** 23, f"{what}: the linear epilogue leaves condition 1: 2^{math.log2(float(bound.max()) / gr):.2f} granules"
        lin64 = pre64 * sc + o["residual"].double()
        assert _is_f32(pre64 * sc) and _is_f32(lin64)
        e["linear"] = lin64.float()
    if "planes" in c.epis:
        e["pre_planes"] = split3(e["pre"])
    if "stats" in c.epis:
        assert fam == "int" and bool((z == z.round()).all())
        nb = -(-c.M // 128)
        zp = torch.zeros(nb * 128, c.N, dtype=F64)
        zp[:c.M] = z64
        s, q = zp.view(nb, 128, c.N).sum(1), (zp * zp).view(nb, 128, c.N).sum(1)
        assert float((zp * zp).view(nb, 128, c.N).abs().sum(1).max()) < 2 ** 24          # integers: any order of the 128 rows is exact
        e["colstats"] = torch.stack((s, q), 1).float()                                     # [nb][2][N]
    return e


# ---- gg_split3_bf16 edges -------------------------------------------------------------------------------------------------------------------------------------
def split_edge_values():
    """f32 [rows, 64]: the three families, +-0, the f32 denormal range, 3.39e38 ... FLT_MAX (the clamp of the first plane), +-inf, NaN."""
    g = torch.Generator().manual_seed(3)
    n = 64
    flt_max = torch.finfo(F32).max
    rows = [wide3((n,), g), _sign((n,), g) * torch.randint(0, 2 ** 10, (n,), generator=g).float() * 2.0 ** -8, _sign((n,), g),
            torch.tensor([0.0, -0.0] * (n // 2)),
            _sign((n,), g) * torch.randint(1, 2 ** 23, (n,), generator=g).float() * 2.0 ** -149,                    # denormals
            _sign((n,), g) * (2.0 ** -126) * (1.0 + torch.rand(n, generator=g)),                                      # the smallest normals
            _sign((n,), g) * torch.linspace(3.39e38, flt_max, n),
            torch.tensor([BF16_MAX, -BF16_MAX, flt_max, -flt_max, math.inf, -math.inf, NAN, -NAN] * (n // 8)),
            torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-20, torch.randn(n, generator=g) * 1e20]
    return torch.stack([r.to(F32) for r in rows])


def assert_planes_equal(got, want, what):
    """bf16 planes bit for bit, NaN by class."""
    for i, (p, q) in enumerate(zip(got, want)):
        p, q = p.cpu(), q.cpu()
        same = (p.view(torch.int16) == q.view(torch.int16)) | (torch.isnan(p) & torch.isnan(q))
        if not bool(same.all()):
            j = int((~same).flatten().nonzero()[0])
            raise AssertionError(f"{what}: plane {i + 1}: {int((~same).sum())} of {same.numel()} elements differ, first at flat index {j}: got {float(p.flatten()[j])!r}, "
                                 f"restatement {float(q.flatten()[j])!r}")


# ---- TN weight gradient ---------------------------------------------------------------------------------------------------------------------------------------
TnCase = collections.namedtuple("TnCase", "name M N K splits scaled fam")
TnGeom = collections.namedtuple("TnGeom", "tilesN tilesK rows_per_split stages last_rows last_stages grid")


def tn_geometry(M, N, K, splits):
    """gg_gemm_tn_split3's geometry, a pure function of what the caller passes: tile 256 (n) x 128 (k), slabs of whole 32-row stages."""
    rps = -(-(-(-M // splits)) // 32) * 32
    assert rps * (splits - 1) < M, "more splits than 32-row stages"
    last = M - rps * (splits - 1)
    tn, tk = -(-N // 256), -(-K // 128)
    return TnGeom(tn, tk, rps, rps // 32, last, -(-last // 32), tn * tk * splits)


TN_CASES = (
    TnCase("tn_70x260x132_s3", 70, 260, 132, 3, True, "w3s1"),          # one stage per slab, a last slab of 6 rows; 2 x 2 tiles x 3 slabs = 12 workgroups
    TnCase("tn_150x260x132_s3", 150, 260, 132, 3, True, "s1w3"),       # two stages; last slab 22 rows
    TnCase("tn_230x260x132_s3", 230, 260, 132, 3, True, "w2w2"),        # three stages; last slab 38 rows: two stages, the last of 6 rows
    TnCase("tn_300x260x132_s3", 300, 260, 132, 3, False, "s1w3"),        # four stages; last slab 44 rows
    TnCase("tn_200x64x32_s1", 200, 64, 32, 1, False, "w3s1"),           # one slab of seven stages, the last of 8 rows; one workgroup
    TnCase("tn_100x260x132_s2", 100, 260, 132, 2, True, "w3s1"),        # 2 x 2 x 2 = 8 workgroups
    TnCase("tn_420x512x256_s3", 420, 512, 256, 3, False, "w2w2"),       # five stages per slab (odd >= 3), whole tiles
)
TN_BY_NAME = {c.name: c for c in TN_CASES}


@functools.lru_cache(maxsize=2)
def tn_operands(name):
    """dY [M, N], X [M, K], rowscale [ceil(M / 77)] or None; the sparse operand is laid out along the contraction (the rows), per 16 columns."""
    c = TN_BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(c.M, c.N, c.K, c.splits))
    if c.fam == "s1w3":
        x, dy = family(c.fam, c.K, c.N, c.M, g)
    else:
        dy, x = family(c.fam, c.N, c.K, c.M, g)
    rs = torch.randint(0, 3, (-(-c.M // ROWS_PER_SCALE),), generator=g).float() if c.scaled else None
    return dy.t().contiguous(), x.t().contiguous(), rs


@functools.lru_cache(maxsize=2)
def tn_expected(name):
    """(slabs [splits, N, K], reduced [N, K]), exact; asserts the conditions on the contraction over the rows."""
    c = TN_BY_NAME[name]
    dY, X, rs = tn_operands(name)
    geo, gr = tn_geometry(c.M, c.N, c.K, c.splits), GRANULE[c.fam]
    dense, sparse = (X, dY) if c.fam == "s1w3" else (dY, X)
    assert_family(c.fam, dense.t().contiguous(), sparse.t().contiguous(), name)
    s = rs.repeat_interleave(ROWS_PER_SCALE)[:c.M, None] if rs is not None else torch.ones(c.M, 1)
    span = (_abs_planes(dY) * (2.0 if c.scaled else 1.0)).t() @ _abs_planes(X)          # (any row scale of {0, 1, 2})
    assert float(span.max()) / gr < 2 ** 23, f"{name}: condition 1 fails"
    assert torch.equal((dY * s).double(), dY.double() * s.double())
    slabs = []
    for i in range(c.splits):
        r = slice(i * geo.rows_per_split, min(c.M, (i + 1) * geo.rows_per_split))
        p64 = (dY[r] * s[r]).double().t() @ X[r].double()
        assert torch.equal(((dY[r] * s[r]).t() @ X[r]).double(), p64), f"{name}: slab {i}: the f32 product is not the f64 product"
        slabs.append(p64.float())
    slabs = torch.stack(slabs)
    total = slabs.double().sum(0)
    assert _is_f32(total)
    return slabs, total.float()


# ---- buffers --------------------------------------------------------------------------------------------------------------------------------------------------
def padded(x, dtype=F32, device="cpu", tail_rows=0, pad=PAD):
    """x [R, C] in a buffer [R + tail_rows, C + pad] whose pad columns and tail rows hold NaN."""
    buf = torch.full((x.shape[0] + tail_rows, x.shape[1] + pad), NAN, dtype=dtype, device=device)
    buf[:x.shape[0], :x.shape[1]] = x.to(device=device, dtype=dtype)
    return buf


def padded_planes(planes, device="cpu"):
    """Three bf16 planes [R, C] as one buffer [3, R, C + PAD] with NaN pad columns."""
    R, Cc = planes[0].shape
    buf = torch.full((3, R, Cc + PAD), NAN, dtype=BF16, device=device)
    for i, p in enumerate(planes):
        buf[i, :, :Cc] = p.to(device)
    return buf


def nan_out(M, N, dtype=F32, device="cpu"):
    return torch.full((M, N + PAD), NAN, dtype=dtype, device=device)


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------------------------
def assert_bits(got, want, what, granule=None, tile=None):
    """got [M, N] (f32, any device) equals want (f32, exact) bit for bit (a NaN is never equal; -0 equals +0 only where the exact value is a zero)."""
    want = want.to(got.device)
    if torch.equal(got, want):
        return
    g, w = got.cpu(), want.cpu()
    bad = ~(g == w)
    i = int(bad.flatten().nonzero()[0])
    m, n = i // g.shape[1], i % g.shape[1]
    err = (g.double() - w.double())[bad]
    fin = err[torch.isfinite(err)]
    gran = f"; |error| {float(fin.abs().min()) / granule:.3g} .. {float(fin.abs().max()) / granule:.3g} granules" if granule and fin.numel() else ""
    where = f", tile ({m // tile[0]}, {n // tile[1]}) local ({m % tile[0]}, {n % tile[1]})" if tile else ""
    raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ ({int(torch.isnan(g).sum())} NaN){gran}; first at ({m}, {n}){where}: "
                         f"got {float(g[m, n])!r}, exact {float(w[m, n])!r}")


def assert_pad_nan(buf, N, what):
    assert bool(torch.isnan(buf[..., N:]).all()), f"{what}: the pad columns of the output were written"


def assert_act_gate(got, z, kind, what, upstream=None):
    """got = u act(z) inside the per-element gate of tests/act_cases.py for an f32 site (u: the exact upstream factor, 1 when None); z finite."""
    form = A.form_for(kind, F32)
    z64, got64 = z.double().to(got.device).flatten(), got.double().flatten()
    u = torch.ones_like(z64) if upstream is None else upstream.double().to(got.device).flatten()
    ref = A.reference(A.KIND_OF[form], z64)
    gate = A.gate(form, F32, z64, ref, u)
    ratio = (got64 - u * ref).abs() / gate
    ratio = torch.where(torch.isfinite(got64), ratio, torch.full_like(ratio, math.inf))
    w = int(ratio.argmax())
    worst = float(ratio[w])
    print(f"  {what}: {form} worst err/gate {worst:.3f} at z = {float(z64[w])!r}, u = {float(u[w])!r}")
    assert worst <= 1.0, f"{what}: {form} err/gate {worst:.3f} at flat index {w}: z = {float(z64[w])!r}, u = {float(u[w])!r}, got {float(got64[w])!r}, fp64 {float(u[w] * ref[w])!r}"
    return worst
