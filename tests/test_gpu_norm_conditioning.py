"""Conditioning of the normalisation statistics: BatchNorm's one-pass variance under a channel offset, constant channels, LayerNorm under row
offsets, and the backward forms that cancel against the raw input.  Every reference is fp64 torch on the CPU.

BatchNorm: bn_finalize forms var = q / count - mean^2 from f32 partial sums (sum y, sum y*y) folded in double.  The formula's condition number is
1 + r^2 with r = |mean| / std of the channel, so the gate on rstd and on the variance part of running_var is 8 * (1 + r^2) * 2^-24 and on the mean
4 * 2^-24 * (|mean| + std).  A CPU emulation of the chain (f32 partials in the producers' order -- at most 4 rows per lane, then a tree, 128 rows per
partial for the GEMMs, at most 32 sequential values per partial for the depthwise maps -- folded in double; 512 channels, r in {0, 4, 16}, M from 75
to 4099) stayed at or under 0.43 of the rstd gate and 0.58 of the mean gate at the depthwise sizes (M = 75 .. 192), 0.46 at the GEMM sizes; a purely
sequential 128-row partial reaches 1.0 - 1.2 x the rstd gate and 1.9 x the mean gate, so a producer that falls back to one long sequential sum fails.
The constants are the derived ones, not widened.

bf16 producers: the statistics are those of the STORED (bf16-rounded) tensor (gemm.hip / conv.hip take them from the rounded values).  The storage
rounding alone moves a channel mean by 7e-5 (r = 0, M = 4099) to 2e-3 (r = 4, M = 130; worst of 256 channels on the CPU, medians 2e-5 to 4e-4) -- above
test_batchnorm_train's mean gate of 1e-5 -- so the reference is
formed in two steps that together pin the chain to the fp64 product of the bf16-rounded operands: the stored tensor against that product within one
bf16 rounding, and the statistics against the fp64 statistics of the stored tensor at test_batchnorm_train's gates.

LayerNorm is two-pass: no r^2 term.  torch's own f32 layer_norm stayed within 0.69 (mean), 0.21 (rstd) and 0.16 (output) of the gates below on the
same rows on the CPU."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
EPS = 1e-5
RSTD_MAX = (1.0 / math.sqrt(EPS)) * (1 + 2.0 ** -20)


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as o
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def close(got, ref, rtol, atol, what=""):
    got = got.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert torch.isfinite(got).all(), what + ": not finite"
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.4g} (ref max {float(ref.abs().max()):.4g})"


# ------------------------------------------------------------------------------------------- A: statistics through the producers
R_F32, R_BF16 = (0.0, 4.0, 16.0), (0.0, 4.0)


def channel_offsets(N, rs):
    """r classes interleaved over the channels of one launch, signs mixed"""
    n = torch.arange(N)
    r = torch.tensor(rs, dtype=F64)[n % len(rs)]
    return r * torch.where((n // len(rs)) % 2 == 0, 1.0, -1.0).double(), n % len(rs)


def gemm_operands(M, N, K, rs, seed, dtype):
    """A = [randn | 1], B = [randn / sqrt(K - 1) | mu_n]: channel n of A . B^T has std ~ 1 and mean mu_n"""
    mu, cls = channel_offsets(N, rs)
    A = torch.cat([rnd(M, K - 1, seed=seed), torch.ones(M, 1, dtype=F64)], 1)
    B = torch.cat([rnd(N, K - 1, seed=seed + 1) / math.sqrt(K - 1), mu[:, None]], 1)
    return A.to(dtype), B.to(dtype), cls


def run_gemm(ops, kind, A, B):
    """-> (stored product on the GPU, partial rows [rows][2][N])"""
    from geoguessr_ai_amd import _lib as L
    M, K = A.shape
    N = B.shape[0]
    if kind in ("gemm_f32", "gemm_bf16"):
        return ops.gemm_nt(A.cuda(), B.cuda(), colstats=True)
    assert kind == "split3"
    Bd = B.cuda()
    Bp = torch.empty(3, N, K, dtype=BF, device="cuda")
    L.check(L.lib().gg_split3_bf16(Bd.data_ptr(), N, K, K, Bp.data_ptr(), L.stream()), "gg_split3_bf16")
    rows = L.lib().gg_gemm_colstats_rows(M)
    out = torch.empty(M, N, device="cuda")
    stats = torch.full((L.lib().gg_stat_rows_capacity(rows), 2, N), float("nan"), device="cuda")
    Ad = A.cuda()
    a = L.Split3Args()
    a.b_planes, a.ldb, a.M, a.N, a.K, a.C, a.ldc = Bp.data_ptr(), K, M, N, K, out.data_ptr(), N
    L.check(L.lib().gg_gemm_nt_split3_af32_stats(C.byref(a), Ad.data_ptr(), K, 0, stats.data_ptr(), L.stream()), "gg_gemm_nt_split3_af32_stats")
    torch.cuda.synchronize()
    return out, stats[:rows]


def finalize(ops, parts, count):
    """gg_bn_finalize with running statistics that start at zero and momentum 0.1: running_var = 0.1f * (float)unbiased, so the variance part is
    recovered by one division and carries two more f32 roundings (2 * 2^-24, added to its gate)"""
    Cn = parts.shape[-1]
    rm, rv = torch.zeros(Cn, device="cuda"), torch.zeros(Cn, device="cuda")
    stat = ops.bn_finalize(parts, count, EPS, 0.1, rm, rv)
    return stat.cpu().double(), rm.cpu().double(), rv.cpu().double()


MOM = float(torch.tensor(0.1, dtype=F32))


def check_stats(what, y, stat, rm, rv, cls, rs, bf16, skip=None):
    """y: the stored tensor [M, C] (fp64 copy); prints the worst error per r class next to its gate, then asserts"""
    M = y.shape[0]
    mean, var = y.mean(0), y.var(0, unbiased=False)
    unb = var * M / (M - 1)
    std = var.sqrt()
    r = mean.abs() / std.clamp_min(1e-300)
    rstd_ref = (var + EPS).rsqrt()
    e_mean = (stat[0] - mean).abs()
    e_rstd = (stat[1] / rstd_ref - 1).abs()
    e_rm = (rm / MOM - mean).abs()
    e_rv = ((rv / MOM) / unb.clamp_min(1e-300) - 1).abs()
    if bf16:       # test_batchnorm_train's gates: mean rtol = atol = 1e-5 scaled by max(1, |mean|), rstd / running_var rtol 1e-4
        g_mean = (1e-5 + 1e-5 * mean.abs()) * mean.abs().clamp_min(1.0)
        g_rstd = torch.full_like(r, 1e-4)
        g_rv = g_rstd
    else:
        g_mean = 4 * U * (mean.abs() + std)
        g_rstd = 8 * (1 + r * r) * U
        g_rv = g_rstd + 2 * U
    keep = torch.ones_like(r, dtype=torch.bool) if skip is None else ~skip
    assert torch.isfinite(stat).all() and torch.isfinite(rm).all() and torch.isfinite(rv).all(), what
    ok = True
    for k, rk in enumerate(rs):
        m = (cls == k) & keep
        if not m.any():
            continue
        line = (f"[{what}] r~{rk:g} (measured {float(r[m].min()):.2f}..{float(r[m].max()):.2f}): mean err/gate {float((e_mean[m] / g_mean[m]).max()):.3f}, "
                f"rstd rel err {float(e_rstd[m].max()):.2e} (gate {float(g_rstd[m].min()):.2e}, worst err/gate {float((e_rstd[m] / g_rstd[m]).max()):.3f}), "
                f"running_var err/gate {float((e_rv[m] / g_rv[m]).max()):.3f}")
        print(line)
        ok = ok and bool((e_mean[m] <= g_mean[m]).all() and (e_rstd[m] <= g_rstd[m]).all() and (e_rv[m] <= g_rv[m]).all() and (e_rm[m] <= g_mean[m] + 2 * U * mean[m].abs()).all())
    assert ok, what + ": statistics outside their gate (figures printed above)"


GEMM_SHAPES = [(130, 48, 32), (517, 200, 96), (4099, 48, 96), (4099, 200, 32), (130, 200, 96), (517, 48, 32)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("kind", ["gemm_f32", "split3"])
def test_batchnorm_statistics_f32_gemm_producers(ops, kind, M, N, K):
    """gg_gemm_nt_f32 with colstats / gg_gemm_nt_split3_af32_stats -> gg_bn_finalize against the fp64 statistics of the tensor the kernel stored (the sums
    are taken from the stored accumulators: gemm_f32.hip `cs += v; cq += v * v`, gemm_split3.hip likewise), r in {0, 4, 16} on the channels of one launch."""
    A, B, cls = gemm_operands(M, N, K, R_F32, seed=M + N + K, dtype=F32)
    y, parts = run_gemm(ops, kind, A, B)
    ref = A.double() @ B.double().t()
    assert float((y.cpu().double() - ref).norm() / ref.norm()) < 1e-6
    stat, rm, rv = finalize(ops, parts, M)
    check_stats(f"{kind} {M}x{N}x{K}", y.cpu().double(), stat, rm, rv, cls, R_F32, bf16=False)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_batchnorm_statistics_bf16_gemm_producer(ops, M, N, K):
    """gg_gemm_nt (bf16) with colstats, r in {0, 4}: stored tensor == fp64 product of the bf16-rounded operands within one bf16 rounding (2^-8 relative plus
    the f32 accumulation, 1e-5 of sum|terms|), statistics == fp64 statistics of the stored tensor at test_batchnorm_train's gates (module docstring)."""
    A, B, cls = gemm_operands(M, N, K, R_BF16, seed=M + N + K, dtype=BF)
    y, parts = run_gemm(ops, "gemm_bf16", A, B)
    assert y.dtype == BF
    ref = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    err = (y.cpu().double() - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag).all()), float((err / (2.0 ** -8 * ref.abs() + 1e-5 * mag)).max())
    stat, rm, rv = finalize(ops, parts, M)
    check_stats(f"gemm_bf16 {M}x{N}x{K}", y.cpu().double(), stat, rm, rv, cls, R_BF16, bf16=True)


def dw_inputs(Cn, H, rs, seed, dtype, amp):
    """input = per-channel constant + noise, taps = a centre tap near 1 plus small neighbours (their sum is not zero): the channel offset survives the
    convolution; the zero padding adds spread at the border, so r is measured on the stored result"""
    mu, cls = channel_offsets(Cn, rs)
    x = (rnd(3, H, H, Cn, seed=seed) + amp * mu).to(dtype)
    taps = 0.05 * rnd(9, Cn, seed=seed + 1)
    taps[4] += 1.0
    return x, taps.float(), mu, cls


DW_SHAPES = [(40, 1, 7), (24, 2, 9), (64, 2, 15)]


@pytest.mark.parametrize("Cn,stride,H", DW_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("fused", [False, True])
def test_batchnorm_statistics_depthwise_producers(ops, fused, dtype, Cn, stride, H):
    """gg_dwconv3x3_fwd[_f32] with colstats and gg_dwconv3x3_fwd_fused[_f32] (the offset then comes from the BatchNorm beta applied on load; GELU at stride 2
    with positive offsets, none at stride 1 with mixed signs) -> gg_bn_finalize, on test_dwconv's odd maps with batch 3.  Partial-row counts come from
    gg_dwconv_stat_rows / gg_dwconv_f32_stat_rows / gg_dwconv_fwd_fused_stat_rows inside the ops wrappers."""
    bf16 = dtype == BF
    rs = R_BF16 if bf16 else R_F32
    x, taps, mu, cls = dw_inputs(Cn, H, rs, seed=Cn + H, dtype=dtype, amp=2.0)
    if fused:
        act = "gelu" if stride == 2 else None
        noise = rnd(3, H, H, Cn, seed=Cn + H + 7).to(dtype)
        beta = (2.0 * mu.abs() if act else 2.0 * mu).float()
        stat_in = torch.stack([0.1 * rnd(Cn, seed=3), 1 + 0.1 * rnd(Cn, seed=4).abs()]).float()
        gamma = (1 + 0.1 * rnd(Cn, seed=5)).float()
        y, parts = ops.dwconv3x3_fwd_fused(noise.cuda(), stat_in.cuda(), gamma.cuda(), beta.cuda(), taps.cuda(), act=act, stride=stride, colstats=True)
    else:
        y, parts = ops.dwconv3x3_fwd(x.cuda(), taps.cuda(), stride=stride, colstats=True)
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), taps.double().t().reshape(Cn, 1, 3, 3), None, stride, 1, 1, Cn).permute(0, 2, 3, 1)
        mag = F.conv2d(x.double().abs().permute(0, 3, 1, 2), taps.double().abs().t().reshape(Cn, 1, 3, 3), None, stride, 1, 1, Cn).permute(0, 2, 3, 1)
        err = (y.cpu().double() - ref).abs()
        assert bool((err <= (2.0 ** -8 * ref.abs() if bf16 else 0) + 1e-5 * mag).all()), "depthwise result"
    assert parts.shape[0] >= 1
    yv = y.reshape(-1, Cn)
    stat, rm, rv = finalize(ops, parts, yv.shape[0])
    name = f"dwconv{'_fused' if fused else ''}_{'bf16' if bf16 else 'f32'} C{Cn} s{stride} H{H} ({parts.shape[0]} partial rows)"
    check_stats(name, yv.cpu().double(), stat, rm, rv, cls, rs, bf16=bf16)


# ------------------------------------------------------------------------------------------- B: constant and near-constant channels
# channel -> value; channel 3 is constant (3.3) except for one row.  The further values give q / count - mean^2 more chances to come out negative (the clamp)
CONST = {0: 0.0, 2: 3.3, 9: 3.3, 12: 0.0, 17: -5.1, 20: 100.3, 26: 1.7, 33: 0.7}
SPIKE, SPIKE_ROW = 3, 77


def const_gemm_operands(M, N, K, rs, seed, dtype):
    A, B, cls = gemm_operands(M, N, K, rs, seed, dtype)
    A, B = A.double(), B.double()
    A[:, 0] = 0.0
    A[SPIKE_ROW, 0] = 1.0                      # column 0 of A is the indicator of one row
    for c, v in list(CONST.items()) + [(SPIKE, 3.3)]:
        B[c] = 0.0
        B[c, K - 1] = v
    B[SPIKE, 0] = 1.0
    return A.to(dtype), B.to(dtype), cls


def bn_ref(y, gamma, beta, act, res, dout):
    """fp64 train-mode BatchNorm (+ residual, activation) of the stored tensor with autograd"""
    yd = y.clone().requires_grad_(True)
    g_, b_ = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    z = (yd - mean) * torch.rsqrt(var + EPS) * g_ + b_
    if res is not None:
        z = res.double() + z
    out = F.gelu(z) if act else z
    out.backward(dout.double())
    return out.detach(), yd.grad, g_.grad, b_.grad


@pytest.mark.parametrize("kind", ["gemm_f32", "split3", "gemm_bf16"])
def test_constant_channels_through_batchnorm(ops, kind):
    """Channels that are exactly constant (0 and 3.3) and one that is constant but for a single row, inside the 8-channel vectors of ordinary channels with
    r in {0, 4}: q / count - mean^2 is rounding noise there (up to ~ 8 v^2 2^-24, the size of eps).  The clamp keeps rstd <= 1 / sqrt(eps); the apply
    returns beta on the constant channels within |v gamma| / sqrt(eps) * 2^-21 + 1e-6 (the f32 rounding of v*sc - mean*sc; bf16 storage adds its own
    rounding of the result, 2^-8 relative); the backward stays finite and the ordinary channels keep test_f32_batchnorm_forward_backward's (bf16:
    test_batchnorm_train's) dy tolerance."""
    bf16 = kind == "gemm_bf16"
    dt = BF if bf16 else F32
    rs = R_BF16          # at r = 16 the rstd gate itself (1.2e-4) is wider than the dy rtol (1e-4) asserted below: the two cannot hold together by derivation
    M, N, K = 517, 48, 32
    A, B, cls = const_gemm_operands(M, N, K, rs, seed=11, dtype=dt)
    y, parts = run_gemm(ops, kind, A, B)
    yd = y.cpu().double()
    const = torch.zeros(N, dtype=torch.bool)
    vals = torch.zeros(N, dtype=F64)
    for c in CONST:
        assert bool((yd[:, c] == yd[0, c]).all()), f"channel {c} of the product is not constant: the test's operands are wrong"
        const[c] = True
        vals[c] = yd[0, c]
    special = const.clone()
    special[SPIKE] = True
    stat, rm, rv = finalize(ops, parts, M)
    assert torch.isfinite(stat).all() and torch.isfinite(rm).all() and torch.isfinite(rv).all()
    print(f"[{kind}] constant channels: rstd {[round(float(v), 2) for v in stat[1][const]]} (limit {RSTD_MAX:.3f}), spike channel rstd {float(stat[1][SPIKE]):.3f}")
    assert bool((stat[1] <= RSTD_MAX).all()) and bool((stat[1] > 0).all())
    assert bool((rv >= 0).all())
    check_stats(f"{kind} beside constant channels", yd, stat, rm, rv, cls, rs, bf16=bf16, skip=special)

    gamma, beta = (1 + 0.2 * rnd(N, seed=12)).float(), (0.1 * rnd(N, seed=13)).float()
    res, dout = rnd(M, N, seed=14).to(dt), rnd(M, N, seed=15).to(dt)
    statd = stat.float().cuda()
    for act in (None, "gelu"):
        for with_res in (False, True):
            r_ = res if with_res else None
            out_ref, dy_ref, dg_ref, db_ref = bn_ref(yd, gamma, beta, act, r_, dout)
            out = ops.bn_apply(y, statd, gamma.cuda(), beta.cuda(), act=act, residual=r_.cuda() if with_res else None).cpu().double()
            assert torch.isfinite(out).all()
            tol = (vals * gamma.double()).abs() / math.sqrt(EPS) * 2.0 ** -21 + 1e-6
            err = (out - out_ref).abs()[:, const]
            # bf16 storage: one rounding of the result, and the bf16 path's polynomial erf (common.h: |GELU error| <= 4.4e-5 absolute)
            gate = tol[const] + (2.0 ** -8 * out_ref.abs()[:, const] + (4.4e-5 if act else 0) if bf16 else 0)
            print(f"[{kind}] bn_apply act={act} residual={with_res}: constant channels worst err/gate {float((err / gate).max()):.3f}")
            assert bool((err <= gate).all()), (kind, act, with_res, float((err / gate).max()))
            close(out[:, ~special], out_ref[:, ~special], 1e-2 if bf16 else 1e-4, 1e-2 if bf16 else 1e-4, "apply on the ordinary channels")
            dz, dy, dg, db = ops.bn_bwd(dout.cuda(), y, statd, gamma.cuda(), beta.cuda(), act=act, residual=r_.cuda() if with_res else None)
            for t in (dz, dy, dg, db):
                assert torch.isfinite(t.float()).all(), "BatchNorm backward on a constant channel"
            if bf16:
                close(dy[:, ~special], dy_ref[:, ~special], 2e-2, 1e-2, "bn dy beside constant channels (bf16)")
            else:
                close(dy[:, ~special], dy_ref[:, ~special], 1e-4, 1e-5, "bn dy beside constant channels")
                close(dg[~special], dg_ref[~special], 1e-4, 1e-4, "bn dgamma beside constant channels")
                close(db[~special], db_ref[~special], 1e-4, 1e-4, "bn dbeta beside constant channels")


@pytest.mark.parametrize("dtype", [F32, BF])
def test_constant_channels_through_depthwise_batchnorm(ops, dtype):
    """the same through gg_dwconv3x3_fwd[_f32] (a centre-only tap keeps a constant input channel constant through the zero padding)"""
    bf16 = dtype == BF
    rs = R_BF16 if bf16 else R_F32
    Cn, H = 40, 7
    x, taps, mu, cls = dw_inputs(Cn, H, rs, seed=5, dtype=F64, amp=2.0)
    taps = taps.double()
    for c, v in CONST.items():
        x[..., c] = v
        taps[:, c] = 0.0
        taps[4, c] = 1.0
    x = x.to(dtype)
    y, parts = ops.dwconv3x3_fwd(x.cuda(), taps.float().cuda(), stride=1, colstats=True)
    yd = y.reshape(-1, Cn).cpu().double()
    const = torch.zeros(Cn, dtype=torch.bool)
    for c in CONST:
        assert bool((yd[:, c] == yd[0, c]).all())
        const[c] = True
    stat, rm, rv = finalize(ops, parts, yd.shape[0])
    print(f"[dwconv {'bf16' if bf16 else 'f32'}] constant channels: rstd {[round(float(v), 2) for v in stat[1][const]]}")
    assert torch.isfinite(stat).all() and bool((stat[1] <= RSTD_MAX).all())
    check_stats("dwconv beside constant channels", yd, stat, rm, rv, cls, rs, bf16=bf16, skip=const)
    gamma, beta = (1 + 0.2 * rnd(Cn, seed=12)).float(), (0.1 * rnd(Cn, seed=13)).float()
    out = ops.bn_apply(y.reshape(-1, Cn), stat.float().cuda(), gamma.cuda(), beta.cuda()).cpu().double()
    tol = (yd[0] * gamma.double()).abs() / math.sqrt(EPS) * 2.0 ** -21 + 1e-6 + (2.0 ** -8 * beta.double().abs() if bf16 else 0)
    assert bool(((out - beta.double()).abs()[:, const] <= tol[const]).all())


# ------------------------------------------------------------------------------------------- C: LayerNorm under row offsets
LN_M = 67
CONST_ROWS = {5: 0.0, 30: 3.3, 66: -1000.0}


def ln_rows(Cn, seed):
    """row m = mu_m + randn with mu alternating 0, +256, -64, 16 on adjacent rows; three rows exactly constant (the last one is the wave kernel's unpaired row)"""
    mu = torch.tensor([0.0, 256.0, -64.0, 16.0], dtype=F64).repeat(LN_M // 4 + 1)[:LN_M]
    x = mu[:, None] + rnd(LN_M, Cn, seed=seed)
    for m, v in CONST_ROWS.items():
        x[m] = v
    return x


def ln_ref(x, gamma, beta):
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    rstd = (var + EPS).rsqrt()
    return (x - mu[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mu, rstd, var


def check_ln(what, x, gamma, beta, out, mean, rstd, rtol, atol, store=0.0, nconst=3):
    """x: fp64 copy of what the kernel normalised; mean / rstd may be None (forms that do not store them); store: one rounding of the output's storage type.
    Rows whose variance is below 1e-7 (exactly constant, or constant up to the f32 rounding of a BatchNorm applied on load) take the constant-row gate
    |v gamma| / sqrt(eps) * 2^-21 + 1e-6 around the reference, which is beta itself on an exactly constant row."""
    ref, mu, rs, var = ln_ref(x, gamma, beta)
    const = var < 1e-7
    out = out.double().cpu()
    assert torch.isfinite(out).all(), what
    line = f"[{what}]"
    if mean is not None:
        mean, rstd = mean.double().cpu(), rstd.double().cpu()
        assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
        fm = (mean - mu).abs() / (4 * U * (mu.abs() + 1))
        fr = ((rstd / rs - 1).abs() / (8 * U * (1 + mu.abs())))[~const]
        line += f" mean err/gate {float(fm.max()):.3f}, rstd err/gate {float(fr.max()):.3f},"
        assert bool((fm <= 1).all()), (what, "mean", float(fm.max()))
        assert bool((fr <= 1).all()), (what, "rstd", float(fr.max()))
        assert bool((rstd <= RSTD_MAX).all())
    tol = atol + rtol * ref.abs() + (8 * mu.abs()[:, None] * U * float(gamma.abs().max()) if rtol < 1e-3 else 0)
    fo = ((out - ref).abs() / tol)[~const]
    line += f" output err/gate {float(fo.max()):.3f}"
    assert int(const.sum()) >= nconst, (what, "the test's rows are wrong", int(const.sum()))
    if not bool(const.any()):
        print(line)
        assert bool((fo <= 1).all()), (what, "output", float(fo.max()))
        return
    v = x[const].abs().max(1, keepdim=True).values
    gate = (v * gamma.double()).abs() / math.sqrt(EPS) * 2.0 ** -21 + 1e-6 + store * ref[const].abs()
    fc = (out[const] - ref[const]).abs() / gate
    exact = var[const] == 0
    if bool(exact.any()):
        assert bool(((ref[const][exact] - beta.double()).abs() < 1e-12).all())
    line += f", constant rows err/gate {float(fc.max()):.3f}"
    print(line)
    assert bool((fc <= 1).all()), (what, "constant rows", float(fc.max()))
    assert bool((fo <= 1).all()), (what, "output", float(fo.max()))


LN_PARAMS = lambda Cn: ((1 + 0.2 * rnd(Cn, seed=41)).float(), (0.1 * rnd(Cn, seed=42)).float())


@pytest.mark.parametrize("Cn", [40, 160, 192, 576, 768, 1024])
def test_layernorm_forward_under_row_offsets(ops, Cn):
    """gg_layernorm_fwd: f32 and bf16 storage (16-lane kernel up to C = 640, one-wave-per-row kernel above), the mixed-storage forms (always the wave kernel,
    two rows in flight per wave) and gg_layernorm_fwd_f16.  Tolerances: test_layernorm's (f32 1e-4 + the offset term, bf16 1e-2), fp16 2e-3."""
    from geoguessr_ai_amd import _lib as L
    x = ln_rows(Cn, seed=Cn)
    gamma, beta = LN_PARAMS(Cn)
    g, b = gamma.cuda(), beta.cuda()
    out, mean, rstd = ops.layernorm_fwd(x.float().cuda(), g, b)
    check_ln(f"ln f32 C{Cn}", x.float().double(), gamma, beta, out, mean, rstd, 1e-4, 1e-4)
    xb = x.to(BF)
    out, mean, rstd = ops.layernorm_fwd(xb.cuda(), g, b)
    check_ln(f"ln bf16 C{Cn}", xb.double(), gamma, beta, out, mean, rstd, 1e-2, 1e-2, store=2.0 ** -8)
    out, mean, rstd = ops.layernorm_fwd(x.float().cuda(), g, b, out_f32=False)          # wave kernel at every C
    check_ln(f"ln f32->bf16 C{Cn}", x.float().double(), gamma, beta, out, mean, rstd, 1e-2, 1e-2, store=2.0 ** -8)
    out, mean, rstd = ops.layernorm_fwd(xb.cuda(), g, b, out_f32=True)
    check_ln(f"ln bf16->f32 C{Cn}", xb.double(), gamma, beta, out, mean, rstd, 1e-4, 1e-4)
    xh = x.to(F16).cuda()
    oh = torch.empty_like(xh)
    L.check(L.lib().gg_layernorm_fwd_f16(xh.data_ptr(), g.data_ptr(), b.data_ptr(), LN_M, Cn, L.f32(EPS), oh.data_ptr(), L.stream()), "gg_layernorm_fwd_f16")
    check_ln(f"ln f16 C{Cn}", xh.cpu().double(), gamma, beta, oh, None, None, 2e-3, 2e-3, store=2.0 ** -10)


@pytest.mark.parametrize("Cn", [40, 160, 192, 576])
def test_layernorm_split_and_batchnorm_on_load_under_row_offsets(ops, Cn):
    """gg_layernorm_fwd_split3 (the three planes summed), gg_layernorm_fwd_bn, gg_layernorm_fwd_bn_f32 and gg_layernorm_fwd_bn_split3.  In the BatchNorm forms
    the input is y = (x - shift) / scale per channel, so the BatchNorm applied on the way in (beta ~ 16) restores the shifted rows; the reference normalises
    the stream the kernel itself wrote.  (There a constant row is constant only up to the rounding of the applied BatchNorm: check_ln's near-constant gate in f32; in bf16 the rounding of y
    leaves no constant row and every row is an ordinary one.)"""
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    x = ln_rows(Cn, seed=Cn)
    gamma, beta = LN_PARAMS(Cn)
    g, b = gamma.cuda(), beta.cuda()
    xf = x.float().cuda()
    planes = torch.empty(3, LN_M, Cn, dtype=BF, device="cuda")
    mean, rstd = torch.empty(LN_M, device="cuda"), torch.empty(LN_M, device="cuda")
    L.check(lib.gg_layernorm_fwd_split3(xf.data_ptr(), g.data_ptr(), b.data_ptr(), LN_M, Cn, L.f32(EPS), planes.data_ptr(), mean.data_ptr(), rstd.data_ptr(), L.stream()), "ln_split3")
    check_ln(f"ln split3 C{Cn}", x.float().double(), gamma, beta, planes.double().sum(0), mean, rstd, 1e-4, 1e-4)
    # BatchNorm on load
    bn_mean, bn_rstd = 0.2 * rnd(Cn, seed=71), 1 + 0.1 * rnd(Cn, seed=72).abs()
    bg, bb = 1 + 0.1 * rnd(Cn, seed=73), 16 + 0.3 * rnd(Cn, seed=74)
    y = (x - bb) / (bg * bn_rstd) + bn_mean
    stat = torch.stack([bn_mean, bn_rstd]).float().cuda()
    bgd, bbd = bg.float().cuda(), bb.float().cuda()
    for dt in (F32, BF):
        xo, out, mean, rstd = ops.layernorm_fwd_bn(y.to(dt).cuda(), stat, bgd, bbd, g, b)
        xs = xo.cpu().double()
        assert float((xs - x).abs().max()) < (2.0 ** -7 if dt == BF else 2e-5) * 1100, "BatchNorm-applied stream"
        check_ln(f"ln bn {'f32' if dt == F32 else 'bf16'} C{Cn}", xs, gamma, beta, out, mean, rstd, 1e-4 if dt == F32 else 1e-2, 1e-4 if dt == F32 else 1e-2,
                 store=0.0 if dt == F32 else 2.0 ** -8, nconst=3 if dt == F32 else 0)
    xo = torch.empty(LN_M, Cn, device="cuda")
    yf = y.float().cuda()
    L.check(lib.gg_layernorm_fwd_bn_split3(yf.data_ptr(), stat.data_ptr(), bgd.data_ptr(), bbd.data_ptr(), xo.data_ptr(), g.data_ptr(), b.data_ptr(), LN_M, Cn, L.f32(EPS),
                                           planes.data_ptr(), mean.data_ptr(), rstd.data_ptr(), L.stream()), "ln_bn_split3")
    check_ln(f"ln bn split3 C{Cn}", xo.cpu().double(), gamma, beta, planes.double().sum(0), mean, rstd, 1e-4, 1e-4)


@pytest.mark.parametrize("Cn,f32", [(40, True), (192, True), (576, True), (1024, True), (192, False), (1024, False)])
def test_layernorm_backward_under_row_offsets(ops, Cn, f32):
    """gg_layernorm_bwd on the shifted rows with the statistics the forward saved, against fp64 autograd at test_layernorm's tolerances (both kernels: C = 1024
    takes the one-wave-per-row form)."""
    dt = F32 if f32 else BF
    x = ln_rows(Cn, seed=Cn).to(dt)
    gamma, beta = LN_PARAMS(Cn)
    dout, dres = rnd(LN_M, Cn, seed=43).to(dt), rnd(LN_M, Cn, seed=44).to(dt)
    xr, g_, b_ = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(xr, (Cn,), g_, b_, EPS).backward(dout.double())
    _, mean, rstd = ops.layernorm_fwd(x.cuda(), gamma.cuda(), beta.cuda())
    dx, dg, db = ops.layernorm_bwd(dout.cuda(), x.cuda(), mean, rstd, gamma.cuda(), dres=dres.cuda())
    t = (1e-4, 1e-4) if f32 else (2e-2, 2e-2)
    ref = xr.grad + dres.double()
    print(f"[ln bwd {'f32' if f32 else 'bf16'} C{Cn}] dx worst err/gate {float(((dx.cpu().double() - ref).abs() / (t[1] + t[0] * ref.abs())).max()):.3f}")
    close(dx, ref, t[0], t[1], "ln dx under row offsets")
    close(dg, g_.grad, 1e-2, 0.3, "ln dgamma")
    close(db, b_.grad, 1e-2, 0.3, "ln dbeta")


@pytest.mark.parametrize("Cn,f32", [(40, True), (192, True), (576, True), (192, False)])
def test_batchnorm_backward_from_column_sums_under_channel_offsets(ops, Cn, f32):
    """y -> x = BN_train(y) with beta = r * gamma, r in {0, 4, 16} over the channels (bf16: {0, 4}) -> LayerNorm.  gg_layernorm_bwd_colsum leaves (sum dx*x,
    sum dx) against the RAW shifted x; gg_bn_bwd_coef_from_x forms gamma * mean(dx * xhat) = (t - beta * s1) / M, which cancels.  Gates: dy against fp64
    autograd at test_layernorm_bwd_with_batchnorm_column_sums' 2e-5 / 3e-2 of the largest |dy|, plus the cancellation term 8 * r * 2^-24 relative to
    sum|dx * x| of the channel, carried through dy = c0*dx + c1*y + c2 (a CPU f32 emulation of the sums, 512 sequential rows per partial, stayed under
    0.3 of that term at r = 0 and under 0.08 at r >= 4)."""
    dt = F32 if f32 else BF
    rs = R_F32 if f32 else R_BF16
    M = 333
    mu, cls = channel_offsets(Cn, rs)
    y = (rnd(M, Cn, seed=80, scale=1.7) + 0.4).to(dt).double()
    bg = (rnd(Cn, seed=81) * 0.2 + 1.0).float()
    bb = (mu * bg.double()).float()
    g, b = (rnd(Cn, seed=83) * 0.2 + 1.0).float(), rnd(Cn, seed=84, scale=0.2).float()
    dout, dres = rnd(M, Cn, seed=85).to(dt), rnd(M, Cn, seed=86).to(dt)
    yr = y.clone().requires_grad_(True)
    x_ref = F.batch_norm(yr, None, None, bg.double(), bb.double(), True, 0.1, EPS)
    (F.layer_norm(x_ref, (Cn,), g.double(), b.double(), EPS) * dout.double()).sum().backward(retain_graph=True)
    x_ref.backward(dres.double())
    rstd_bn = (y.var(0, unbiased=False) + EPS).rsqrt()
    stat = torch.stack([y.mean(0), rstd_bn]).float().cuda()
    x = ops.bn_apply(y.to(dt).cuda(), stat, bg.cuda(), bb.cuda())
    _, mean, rstd = ops.layernorm_fwd(x, g.cuda(), b.cuda())
    dx0, _, _ = ops.layernorm_bwd(dout.cuda(), x, mean, rstd, g.cuda(), dres=dres.cuda(), want_param_grads=False)
    dx, part, rows = ops.layernorm_bwd_colsum(dout.cuda(), x, mean, rstd, g.cuda(), dres=dres.cuda())
    close(dx, dx0, 1e-6 if f32 else 8e-3, 1e-6 if f32 else 1e-3, "dx of the colsum form")
    coef = ops.bn_bwd_coef_from_x(part, rows, M, stat, bg.cuda(), bb.cuda()).cpu().double()
    dxd = dx.double().cpu()
    dy = coef[0] * dxd + coef[1] * y + coef[2]
    ref = yr.grad
    # cancellation term: an error e in u = (t - beta s1) / M moves dy by rstd^2 * |y - mean| * e
    xs = x.double().cpu()
    e_u = 8 * mu.abs() * U * (dxd * xs).abs().sum(0) / M
    extra = rstd_bn ** 2 * (y - y.mean(0)).abs() * e_u
    tol = (2e-5 if f32 else 3e-2) * ref.abs().max() + extra
    f = (dy - ref).abs() / tol
    for k, rk in enumerate(rs):
        print(f"[coef_from_x {'f32' if f32 else 'bf16'} C{Cn}] r={rk:g}: dy worst err/gate {float(f[:, cls == k].max()):.3f}")
    assert bool((f <= 1).all()), float(f.max())


# ------------------------------------------------------------------------------------------- D: weight-gradient GEMMs with BatchNorm applied on load
@pytest.mark.parametrize("M,N,K", [(517, 52, 36), (3000, 200, 96)])
@pytest.mark.parametrize("f32", [True, False])
def test_gemm_tn_with_batchnorm_apply_on_load_under_channel_offsets(ops, f32, M, N, K):
    """dW = (c0*dz + c1*y + c2)^T X with y shifted by r in {0, 4, 16} on different columns and (c1, c2) the BatchNorm-backward pair, so c1*y + c2 cancels
    (c2 = -c1 * mean + small).  Tolerances of test_f32_gemm_tn_with_batchnorm_apply_on_load (2e-5) and test_gemm_tn_with_batchnorm_apply_on_load (rtol 2e-3 against the
    bf16-rounded dy), each scaled by sum_m |dy[m][n] X[m][k]| of the output element instead of the largest output; no absolute term."""
    dt = F32 if f32 else BF
    mu, cls = channel_offsets(N, R_F32)
    y = (rnd(M, N, seed=91) + mu).to(dt).double()
    dz, X = rnd(M, N, seed=90, scale=0.1).to(dt).double(), rnd(M, K, seed=92).to(dt).double()
    c0, c1 = 1.0 + 0.1 * rnd(N, seed=93), 0.05 * rnd(N, seed=94)
    coef = torch.stack([c0, c1, -c1 * mu + 0.02 * rnd(N, seed=95)]).float()
    cd = coef.double()
    if not f32 and (N % 8 or K % 8):          # the bf16 form takes N, K in multiples of 8 only: it must refuse, not compute something
        from geoguessr_ai_amd import _lib as L
        with pytest.raises(L.GgError):
            ops.gemm_tn_bn(dz.to(dt).cuda(), y.to(dt).cuda(), coef.cuda(), X.to(dt).cuda())
        N, K = 56, 40
        return test_gemm_tn_with_batchnorm_apply_on_load_under_channel_offsets(ops, f32, M, N, K)
    got = ops.gemm_tn_bn(dz.to(dt).cuda(), y.to(dt).cuda(), coef.cuda(), X.to(dt).cuda()).cpu().double()
    dy = cd[0] * dz + (cd[1] * y + cd[2])
    if f32:
        ref = dy.t() @ X
        tol = 2e-5 * (dy.abs().t() @ X.abs())
    else:
        dyq = dy.float().to(BF).double()            # the bf16 kernel rounds the formed dy to bf16 for the MFMA (as the existing test's reference does)
        ref = dyq.t() @ X
        tol = 2e-3 * (dyq.abs().t() @ X.abs())
    f = (got - ref).abs() / tol
    for k, rk in enumerate(R_F32):
        print(f"[gemm_tn_bn {'f32' if f32 else 'bf16'} {M}x{N}x{K}] r={rk:g}: worst err/gate {float(f[cls == k].max()):.3f}")
    assert bool((f <= 1).all()), float(f.max())
