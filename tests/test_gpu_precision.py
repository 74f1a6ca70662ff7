"""Reference-precision (fp32) mode and the tightened parity of round 2 -- all through libgg.so on the GPU.

* f32 kernels (gg_*_f32: f32 MFMA GEMMs, depthwise / im2col, BatchNorm, pooling) against plain torch fp32 math on the CPU;
* online-softmax attention (gg_attention_flash_*) for 49 / 196 / 577 / 1024-token shapes, bf16 and f32 storage, forward and backward
  incl. the relative-position-bias gradient, against torch autograd;
* whole-model parity at the tolerances SURVEY.md 8(c) states: fp32 mode vs the fp32 oracle (rtol 1e-4 class), bf16 mode vs the
  bf16-storage-emulating oracle (embedding rel <= 2e-2, top-1 geocell agreement >= 99 %, top-5 overlap >= 4.9), with PER-STAGE
  activation taps (gg_tinyvit_activation_info <-> oracle taps) so an error is localised instead of averaged into a cosine, and
  per-tensor gradient relative errors.  Measured values are printed (pytest -s) and tabulated in DESIGN.md section 4."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as o
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, ref, rtol, atol, what=""):
    got = got.detach().float().cpu(); ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.4g} (ref max {float(ref.abs().max()):.4g})"


def relerr(got, ref):
    got = got.detach().double().cpu().flatten(); ref = ref.detach().double().cpu().flatten()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


# ------------------------------------------------------------------------------------------- f32 GEMMs
def test_f32_mfma_fragment_layout(ops):
    M = N = K = 128
    A = torch.zeros(M, K)
    A[torch.arange(M), (torch.arange(M) * 7 + 3) % K] = 1.0
    B = torch.arange(N)[:, None] * 0.5 + torch.arange(K)[None, :] * 0.03125
    got = ops.gemm_nt(A.cuda(), B.cuda())
    assert got.dtype == F32
    close(got, A @ B.t(), 0, 0, "f32 mfma layout (exact)")


@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (300, 200, 100), (1000, 48, 32), (4099, 384, 96), (96, 576, 2304), (64, 12647, 576),
                                   (257, 96, 432), (130, 72, 20), (515, 192, 64), (300, 576, 192), (129, 288, 48), (1000, 100, 36)])
def test_f32_gemm_plain_and_stats(ops, M, N, K):
    A, B = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1)
    ref = A.double() @ B.double().t()
    got, stats = ops.gemm_nt(A.cuda(), B.cuda(), colstats=True)
    close(got, ref, 2e-6, 2e-6 * float(ref.abs().max()), f"f32 gemm {M}x{N}x{K}")
    s = stats.cpu().double().sum(0)
    close(s[0], ref.sum(0), 1e-5, 1e-4 * float(ref.abs().sum(0).max()), "colstats sum")
    close(s[1], (ref * ref).sum(0), 1e-5, 1e-5 * float((ref * ref).sum(0).max()), "colstats sumsq")


def test_f32_gemm_epilogues(ops):
    M, N, K, T = 520, 200, 96, 130
    A, B = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=0.2)
    bias, res = rnd(N, seed=5), rnd(M, N, seed=6)
    rs = torch.tensor([0.0, 1.25, 1.25, 0.0])
    z = (A.double() @ B.double().t() + bias.double())
    out, pre = ops.gemm_nt(A.cuda(), B.cuda(), bias=bias.cuda(), act="gelu", preact=True)
    close(pre, z, 1e-5, 1e-5, "f32 preact")
    close(out, F.gelu(z), 1e-5, 1e-5, "f32 gelu (exact erf)")
    out = ops.gemm_nt(A.cuda(), B.cuda(), bias=bias.cuda(), rowscale=rs.cuda(), rows_per_scale=T, residual=res.cuda())
    close(out, res.double() + rs.double().repeat_interleave(T)[:, None] * z, 1e-5, 1e-5, "f32 rowscale+residual")
    hp = rnd(M, N, seed=7)
    zz = hp.double().clone().requires_grad_(True)
    F.gelu(zz).sum().backward()
    out = ops.gemm_nt(A.cuda(), B.cuda(), dact_preact=hp.cuda(), dact="gelu", rowscale=rs.cuda(), rows_per_scale=T)
    close(out, (A.double() @ B.double().t()) * zz.grad * rs.double().repeat_interleave(T)[:, None], 1e-5, 1e-5, "f32 dgelu")
    out = ops.gemm_nt(A.cuda(), B.cuda(), bias=bias.cuda(), act="quick_gelu")
    close(out, z * torch.sigmoid(1.702 * z), 1e-5, 1e-5, "f32 quick_gelu")


@pytest.mark.parametrize("M,N,K,T", [(777, 96, 432, 0), (4100, 576, 576, 1025), (300, 12648, 576, 300), (50, 48, 32, 0), (100003, 48, 32, 0), (20001, 64, 64, 77),
                                     (9999, 40, 20, 0)])
def test_f32_gemm_tn_weight_gradient(ops, M, N, K, T):
    dY, X = rnd(M, N, seed=8, scale=0.1), rnd(M, K, seed=9)
    rs = None
    ref = dY.double()
    if T:
        rs = torch.linspace(0.5, 1.5, (M + T - 1) // T)
        ref = ref * rs.double().repeat_interleave(T)[:M, None]
    ref = ref.t() @ X.double()
    got = ops.gemm_tn(dY.cuda(), X.cuda(), rowscale=None if rs is None else rs.cuda(), rows_per_scale=T)
    close(got, ref, 1e-5, 1e-5 * float(ref.abs().max()), f"f32 gemm_tn {M}x{N}x{K}")
    close(ops.colsum_bf16(dY.cuda()), dY.double().sum(0), 1e-5, 1e-5, "colsum f32")


# ------------------------------------------------------------------------------------------- f32 spatial kernels
@pytest.mark.parametrize("B,H,C,stride", [(2, 14, 384, 1), (3, 9, 64, 1), (2, 28, 192, 2), (2, 7, 576, 1), (1, 13, 40, 2), (2, 56, 24, 1),
                                          (1, 5, 1024, 1), (1, 6, 1024, 2)])      # the widest C the depthwise family takes, once per route
def test_f32_dwconv_forward_backward(ops, B, H, C, stride):
    x = rnd(B, H, H, C, seed=10)
    w = rnd(C, 1, 3, 3, seed=11, scale=0.4)
    taps = w.view(C, 9).t().contiguous()
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, stride, 1, 1, C)
    y, stats = ops.dwconv3x3_fwd(x.cuda(), taps.cuda(), stride=stride, colstats=True)
    close(y, yr.permute(0, 2, 3, 1), 1e-5, 1e-5, "dw f32 fwd")
    s = stats.cpu().double().sum(0)
    close(s[0], yr.sum((0, 2, 3)), 1e-4, 1e-3, "dw f32 stat sum")
    close(s[1], (yr * yr).sum((0, 2, 3)), 1e-4, 1e-3, "dw f32 stat sumsq")
    dy = rnd(*yr.shape, seed=12).permute(0, 2, 3, 1).contiguous()
    yr.backward(dy.permute(0, 3, 1, 2).double())
    dx = ops.dwconv3x3_bwd_data(dy.cuda(), taps.cuda(), B, H, H, C, stride=stride)
    close(dx, xr.grad.permute(0, 2, 3, 1), 1e-5, 1e-5, "dw f32 bwd data")
    dw = ops.dwconv3x3_bwd_weight(x.cuda(), dy.cuda(), stride=stride)
    close(dw, wr.grad, 1e-4, 1e-4 * float(wr.grad.abs().max()), "dw f32 bwd weight")


def test_f32_im2col_col2im(ops):
    B, H, C = 2, 12, 48
    x = rnd(B, H, H, C, seed=13)
    col = ops.im2col_nhwc(x.cuda(), stride=2)
    ref = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1, stride=2)           # (B, C*9, L), k = c*9 + tap
    ref = ref.view(B, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)      # -> k = tap*C + c
    close(col, ref, 0, 0, "im2col f32 (exact)")
    d = rnd(*col.shape, seed=14)
    dx = ops.col2im_nhwc(d.cuda(), B, H, H, C, stride=2)
    lhs = float((col.cpu().double() * d.double()).sum()); rhs = float((x.double() * dx.cpu().double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs), "col2im is the adjoint of im2col"
    img = rnd(2, 3, 16, 16, seed=15)
    c1 = ops.im2col_nchw3(img.cuda(), stride=2, out_dtype=F32).cpu()
    r1 = F.unfold(img, 3, padding=1, stride=2).view(2, 3, 9, -1).permute(0, 3, 2, 1).reshape(-1, 27)
    close(c1[:, :27], r1, 0, 0, "im2col nchw f32")
    assert float(c1[:, 27:].abs().max()) == 0
    stat = torch.stack([rnd(C, seed=16, scale=0.1), 1 + 0.1 * rnd(C, seed=17).abs()])
    gam, bet = 1 + 0.2 * rnd(C, seed=18), 0.1 * rnd(C, seed=19)
    cb = ops.im2col_nhwc_bn(x.cuda(), stat.cuda(), gam.cuda(), bet.cuda(), act="gelu", stride=2)
    act = F.gelu((x.double() - stat[0].double()) * (stat[1] * gam).double() + bet.double())
    rb = F.unfold(act.permute(0, 3, 1, 2), 3, padding=1, stride=2).view(B, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)
    close(cb, rb, 1e-5, 1e-5, "im2col+BN+GELU f32")


@pytest.mark.parametrize("act", [None, "gelu"])
def test_f32_batchnorm_forward_backward(ops, act):
    M, C, T = 1030, 96, 515
    y = rnd(M, C, seed=20) * 2 + 0.3
    gamma, beta = 1 + 0.2 * rnd(C, seed=21), 0.2 * rnd(C, seed=22)
    res = rnd(M, C, seed=23)
    rs = torch.tensor([1.25, 0.0])
    yd = y.double().requires_grad_(True)
    g_, b_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    z = (yd - mean) * torch.rsqrt(var + 1e-5) * g_ + b_
    pre = res.double() + rs.double().repeat_interleave(T)[:, None] * z
    out_ref = F.gelu(pre) if act else pre
    stat = torch.stack([mean.detach(), torch.rsqrt(var.detach() + 1e-5)]).float()
    out = ops.bn_apply(y.cuda(), stat.cuda(), gamma.cuda(), beta.cuda(), act=act, residual=res.cuda(), rowscale=rs.cuda(), rows_per_scale=T)
    close(out, out_ref, 1e-5, 1e-5, "bn_apply f32")
    dout = rnd(M, C, seed=24)
    out_ref.backward(dout.double())
    dz, dy, dg, db = ops.bn_bwd(dout.cuda(), y.cuda(), stat.cuda(), gamma.cuda(), beta.cuda(), act=act, residual=res.cuda(), rowscale=rs.cuda(),
                                rows_per_scale=T)
    close(dy, yd.grad, 1e-4, 1e-5, "bn_bwd f32 dy")
    close(dg, g_.grad, 1e-4, 1e-4, "bn_bwd f32 dgamma")
    close(db, b_.grad, 1e-4, 1e-4, "bn_bwd f32 dbeta")


# ------------------------------------------------------------------------------------------- online-softmax attention
def _attn_ref(qkv, nh, D, N, nw, ws, map_hw, table, q_off, k_off, v_off, hs, dout=None):
    """torch reference on the same token layout; returns out (tokens, nh*D) [and dqkv, dtable]."""
    qkv = qkv.double().clone().requires_grad_(True)
    tab = None if table is None else table.double().clone().requires_grad_(True)
    tokens = qkv.shape[0]
    if ws:
        Hh = Ww = map_hw
        per = (Hh // ws) * (Ww // ws)
        b = nw // per
        idx = torch.arange(tokens).view(b, Hh // ws, ws, Ww // ws, ws).permute(0, 1, 3, 2, 4).reshape(nw, N)
        yy, xx = torch.arange(N) // ws, torch.arange(N) % ws
        bidx = (yy[:, None] - yy[None, :]).abs() * ws + (xx[:, None] - xx[None, :]).abs()
    else:
        idx = torch.arange(tokens).view(nw, N)
    out = torch.zeros(tokens, nh * D, dtype=torch.float64)
    outs = []
    for h in range(nh):
        q = qkv[:, q_off + h * hs:q_off + h * hs + D][idx]
        k = qkv[:, k_off + h * hs:k_off + h * hs + D][idx]
        v = qkv[:, v_off + h * hs:v_off + h * hs + D][idx]
        s = q @ k.transpose(1, 2) * D ** -0.5
        if tab is not None:
            s = s + tab[h][bidx]
        outs.append(torch.softmax(s, -1) @ v)
    o = torch.stack(outs, 2).reshape(nw * N, nh * D)
    out = torch.zeros(tokens, nh * D, dtype=torch.float64).index_copy(0, idx.reshape(-1), o)
    if dout is None:
        return out.detach()
    out.backward(dout.double())
    return out.detach(), qkv.grad, None if tab is None else tab.grad


# ------------------------------------------------------------------------------------------- f32 BatchNorm fusions
@pytest.mark.parametrize("C,H,act,stride", [(192, 28, "gelu", 2), (48, 15, "gelu", 2), (384, 14, "gelu", 1), (16, 13, "gelu", 1), (40, 7, None, 1),
                                            (256, 56, "gelu", 1)])
def test_f32_dwconv_with_batchnorm_gelu_on_load(ops, C, H, act, stride):
    """gg_dwconv3x3_fwd_fused_f32 == gg_bn_apply_f32 then gg_dwconv3x3_fwd_f32 (MBConv.conv2 / PatchMerging.conv2 in fp32 mode), incl. the
    BatchNorm partial statistics of the result, and == torch conv2d over fp32 BatchNorm + exact GELU."""
    B = 3
    y1 = rnd(B, H, H, C, seed=50, scale=1.5)
    mean, var = rnd(C, seed=51, scale=0.4), rnd(C, seed=52).abs() + 0.5
    stat = torch.stack([mean, (var + 1e-5).rsqrt()])
    gamma, beta = rnd(C, seed=53) + 1.0, rnd(C, seed=54, scale=0.3)
    taps = rnd(9, C, seed=55, scale=0.4)
    a1 = ops.bn_apply(y1.cuda().view(-1, C), stat.cuda(), gamma.cuda(), beta.cuda(), act=act).view(B, H, H, C)
    want, wstats = ops.dwconv3x3_fwd(a1, taps.cuda(), stride=stride, colstats=True)
    got, gstats = ops.dwconv3x3_fwd_fused(y1.cuda(), stat.cuda(), gamma.cuda(), beta.cuda(), taps.cuda(), act=act, stride=stride, colstats=True)
    assert got.dtype == F32
    close(got, want, 1e-5, 1e-5, "fused f32 dwconv vs apply + conv")
    close(gstats.sum(0), wstats.sum(0), 1e-4, 1e-2, "fused f32 dwconv statistics")
    z = (y1 - mean) * stat[1] * gamma + beta
    ref = F.conv2d((F.gelu(z) if act else z).permute(0, 3, 1, 2), taps.t().reshape(C, 1, 3, 3), None, stride, 1, 1, C)
    close(got.permute(0, 3, 1, 2), ref, 1e-4, 1e-4, "fused f32 dwconv vs conv2d")


@pytest.mark.parametrize("C,H", [(384, 14), (40, 7), (256, 56), (16, 13)])
def test_f32_dwconv_data_gradient_with_batchnorm_fusions(ops, C, H):
    """gg_dwconv3x3_bwd_data_fused_f32: BatchNorm-backward apply on the loads (dy2 = c0*dz2 + c1*y2 + c2), stride-1 data gradient,
    * GELU'(BN1(y1)) and BatchNorm backward's two column sums on the stores -- each fusion alone and both together, vs fp32 torch."""
    B = 2
    dz = rnd(B, H, H, C, seed=90); y2 = rnd(B, H, H, C, seed=91)
    coef = torch.stack([1 + 0.2 * rnd(C, seed=92), 0.3 * rnd(C, seed=93), 0.1 * rnd(C, seed=94)])
    w = rnd(C, 1, 3, 3, seed=95, scale=0.4); taps = w.view(C, 9).t().contiguous()
    y1 = rnd(B, H, H, C, seed=96) + 0.3
    gamma, beta = 1 + 0.2 * rnd(C, seed=97), 0.2 * rnd(C, seed=98)
    mean, var = y1.mean((0, 1, 2)), y1.var((0, 1, 2), unbiased=False)
    rstd = torch.rsqrt(var + 1e-5)
    dy = coef[0] * dz + coef[1] * y2 + coef[2]
    xr = torch.zeros(B, C, H, H, requires_grad=True)
    F.conv2d(xr, w, None, 1, 1, 1, C).backward(dy.permute(0, 3, 1, 2))
    da = xr.grad.permute(0, 2, 3, 1)
    z = ((y1 - mean) * rstd * gamma + beta).requires_grad_(True)
    F.gelu(z).sum().backward()
    ref = da * z.grad
    c = lambda t: t.cuda()
    ep = dict(ep_y=c(y1), ep_stat=c(torch.stack([mean, rstd])), ep_gamma=c(gamma), ep_beta=c(beta), ep_act="gelu")
    out, part = ops.dwconv3x3_bwd_data_fused(c(dz), c(y2), c(coef), c(taps), **ep)
    close(out, ref, 1e-4, 1e-5, "f32 fused dgrad (both)")
    s = part.cpu().sum(0)
    close(s[0], ref.sum((0, 1, 2)), 1e-4, 1e-3, "f32 fused sum dz")
    close(s[1], (ref * ((y1 - mean) * rstd)).sum((0, 1, 2)), 1e-4, 2e-3, "f32 fused sum dz*xhat")
    out, part = ops.dwconv3x3_bwd_data_fused(c(dy), None, None, c(taps), **ep)
    close(out, ref, 1e-4, 1e-5, "f32 fused dgrad (epilogue only)")
    close(part.cpu().sum(0)[0], ref.sum((0, 1, 2)), 1e-4, 1e-3, "f32 fused sum dz (epilogue only)")
    out, part = ops.dwconv3x3_bwd_data_fused(c(dz), c(y2), c(coef), c(taps))
    assert part is None
    close(out, da, 1e-4, 1e-5, "f32 fused dgrad (load only)")


@pytest.mark.parametrize("act", [None, "gelu"])
@pytest.mark.parametrize("M,K,N", [(3000, 256, 64), (1111, 384, 96), (130, 128, 128)])
def test_f32_gemm_batchnorm_prologue(ops, M, K, N, act):
    """MBConv.conv3 in fp32 mode: C = act(BN(y_prev)) @ W^T with the BatchNorm + exact GELU formed while the GEMM stages its A tile."""
    y = rnd(M, K, seed=80) + 0.5
    W = rnd(N, K, seed=81) / K ** 0.5
    gamma, beta = 1 + 0.2 * rnd(K, seed=82), 0.3 * rnd(K, seed=83)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    stat = torch.stack([mean, torch.rsqrt(var + 1e-5)])
    z = F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5)
    ref = (F.gelu(z) if act else z) @ W.T
    out, stats = ops.conv_bn_prologue(y.cuda(), stat.cuda(), gamma.cuda(), beta.cuda(), W.cuda(), act=act, colstats=True)
    assert out.dtype == F32
    close(out, ref, 1e-4, 1e-4, "f32 prologue gemm")
    s = stats.cpu().sum(0)
    close(s[0], ref.sum(0), 1e-4, 2e-3, "f32 prologue colsum")
    close(s[1], (ref * ref).sum(0), 1e-4, 2e-3, "f32 prologue colsumsq")


@pytest.mark.parametrize("M,Cin,Cmid,Cout", [(3000, 64, 256, 64), (1111, 64, 128, 192), (200, 96, 384, 96)])
def test_f32_convnorm_chain_backward_fused_into_gemms(ops, M, Cin, Cmid, Cout):
    """x -conv1-> y1 -BN(train)+GELU-> a1 -conv3-> y3 in f32: conv3's dgrad carries BatchNorm backward's reduce in its epilogue, conv1's
    dgrad forms dy1 = c0*dz1 + c1*y1 + c2 from the two sources while staging A (+ residual).  Checked against fp32 autograd."""
    x = rnd(M, Cin, seed=70)
    W1 = rnd(Cmid, Cin, seed=71) / Cin ** 0.5
    W3 = rnd(Cout, Cmid, seed=72) / Cmid ** 0.5
    gamma, beta = 1 + 0.2 * rnd(Cmid, seed=73), 0.3 * rnd(Cmid, seed=74)
    G = rnd(M, Cout, seed=75)
    skip = rnd(M, Cin, seed=76)
    y1 = x @ W1.T + 1.5
    yr = y1.clone().requires_grad_(True)
    g_, b_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a1 = F.gelu(F.batch_norm(yr, None, None, g_, b_, True, 0.1, 1e-5))
    (a1 @ W3.T).backward(G)
    dx_ref = yr.grad @ W1 + skip
    mean, var = y1.mean(0), y1.var(0, unbiased=False)
    stat = torch.stack([mean, torch.rsqrt(var + 1e-5)]).cuda()
    dz, coef, dg, db = ops.conv_dgrad_bn_bwd(G.cuda(), W3.T.contiguous().cuda(), y1.cuda(), stat, gamma.cuda(), beta.cuda(), act="gelu")
    assert dz.dtype == F32
    dy = coef[0] * dz + coef[1] * y1.cuda() + coef[2]
    close(dy, yr.grad, 2e-4, 2e-5, "f32 dy from gemm-epilogue dz + coef")
    close(dg, g_.grad, 2e-4, 2e-3, "f32 dgamma")
    close(db, b_.grad, 2e-4, 2e-3, "f32 dbeta")
    dx = ops.folded_dgrad(dz, y1.cuda(), W1.cuda(), coef, stat, residual=skip.cuda())
    close(dx, dx_ref, 2e-4, 5e-5, "f32 two-source dgrad")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("nh,D,ws,map_hw,batch,linearN", [(3, 32, 7, 14, 2, 0), (2, 32, 14, 14, 2, 0), (2, 32, 32, 32, 1, 0), (2, 32, 24, 24, 1, 0),
                                                          (2, 64, 0, 0, 2, 577), (3, 64, 0, 0, 3, 50),
                                                          # edges of the single-pass backward / balanced forward dispatch: a 256-token window with bias (16 tiles: the
                                                          # LDS budget decides), one tile, one token, 17 tokens (2 tiles, 1 live row), 256 tokens at head dim 64 (two-pass),
                                                          # 80 tokens = 5 tiles (the smallest 4 n + 1 strip count: cooperative tail with 4 owner waves)
                                                          (2, 32, 16, 16, 1, 0), (2, 32, 0, 0, 3, 16), (2, 32, 0, 0, 3, 1), (1, 32, 0, 0, 2, 17), (1, 64, 0, 0, 2, 256),
                                                          (2, 64, 0, 0, 2, 80), (2, 32, 9, 18, 1, 0)])
def test_flash_attention_forward_backward(ops, dtype, nh, D, ws, map_hw, batch, linearN):
    if ws:
        N, nw = ws * ws, batch * (map_hw // ws) ** 2
        hs, q_off, k_off, v_off = 3 * D, 0, D, 2 * D            # TinyViT per-head interleaved [q|k|v]
        table = rnd(nh, ws * ws, seed=30, scale=0.5)
    else:
        N, nw = linearN, batch
        hs, q_off, k_off, v_off = D, 0, nh * D, 2 * nh * D       # CLIP [q|k|v] blocks
        table = None
    tokens = nw * N
    qkv = rnd(tokens, 3 * nh * D, seed=31)
    dout = rnd(tokens, nh * D, seed=32)
    if dtype == BF:
        qkv, dout = qkv.to(BF).float(), dout.to(BF).float()
    kw = dict(num_windows=nw, tokens_per_window=N, num_heads=nh, head_dim=D, q_off=q_off, k_off=k_off, v_off=v_off, head_stride=hs,
              window_size=ws, map_h=map_hw, map_w=map_hw, bias_table=None if table is None else table.cuda())
    out, lse = ops.attention_flash(qkv.cuda().to(dtype), want_lse=True, **kw)
    ref, dq_ref, dt_ref = _attn_ref(qkv, nh, D, N, nw, ws, map_hw, table, q_off, k_off, v_off, hs, dout)
    tol = 2e-5 if dtype == F32 else 1.5e-2
    close(out, ref, tol, tol, f"flash fwd {dtype}")
    # backward consumes the forward's stored out / lse
    dqkv, dtab = ops.attention_flash(qkv.cuda().to(dtype), dout=dout.cuda().to(dtype), out=out, lse=lse, want_dbias=table is not None, **kw)
    e = relerr(dqkv, dq_ref)
    assert e < (2e-5 if dtype == F32 else 1.5e-2), f"flash dqkv rel err {e}"
    if table is not None:
        e = relerr(dtab, dt_ref)
        assert e < (5e-5 if dtype == F32 else 2e-2), f"flash dbias rel err {e}"
    # dS hand-off (GgAttnArgs.ds_scratch): dK/dV pass first, dQ as one product of the stored dS -- same dk / dv bit for bit, dq to rounding
    dqkv2, dtab2 = ops.attention_flash(qkv.cuda().to(dtype), dout=dout.cuda().to(dtype), out=out, lse=lse, want_dbias=table is not None, ds_handoff=True, **kw)
    e = relerr(dqkv2, dq_ref)
    assert e < (2e-5 if dtype == F32 else 1.5e-2), f"flash dqkv (dS hand-off) rel err {e}"
    assert float((dqkv2.float() - dqkv.float()).abs().max()) <= (1e-5 if dtype == F32 else 2e-2) * float(dqkv.float().abs().max())
    if table is not None:          # (LDS float atomics inside a workgroup: equal to rounding, not bit for bit)
        assert relerr(dtab2, dt_ref) < (5e-5 if dtype == F32 else 2e-2)


def test_flash_online_softmax_rescale_branch(ops):
    """A key in the LAST tile dominates one query's row: the running max jumps after earlier tiles were accumulated (the rescale path)."""
    nh, D, N = 1, 32, 200
    qkv = rnd(N, 3 * D, seed=33) * 0.2
    qkv[5, :D] = 3.0                          # query 5
    qkv[190, D:2 * D] = 3.0                   # key 190 (4th tile) aligned with it: score ~ 32*9/5.6 = 51
    kw = dict(num_windows=1, tokens_per_window=N, num_heads=nh, head_dim=D, q_off=0, k_off=D, v_off=2 * D, head_stride=3 * D)
    out = ops.attention_flash(qkv.cuda(), **kw)
    ref = _attn_ref(qkv, nh, D, N, 1, 0, 0, None, 0, D, 2 * D, 3 * D)
    close(out, ref, 2e-5, 2e-5, "flash rescale")


# ------------------------------------------------------------------------------------------- whole-model parity with stage taps
def _randomize(bb, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in bb.named_parameters():
            if name.endswith(("bn.weight", "norm.weight")):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias") and p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("attention_biases"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif name.endswith(".weight") and p.dim() == 2:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))


def _tap_names(cfg):
    names = [("patch_embed", "patch_embed.out", True)]
    for i in range(cfg.depths[0]):
        names.append((f"stages.0.blocks.{i}.out", f"stages.0.blocks.{i}.out", True))
    for s in range(1, 4):
        names.append((f"stages.{s}.downsample.out", f"stages.{s}.downsample.out", True))
        for i in range(cfg.depths[s]):
            for leaf in ("attn.out", "x1", "x2", "out"):
                names.append((f"stages.{s}.blocks.{i}.{leaf}", f"stages.{s}.blocks.{i}.{leaf if leaf != 'attn.out' else 'attn.out'}", False))
    return names


def _compare_taps(bb, cfg, taps, batch, dtype, tol, label):
    """Relative L2 error of every saved activation against the oracle's tap of the same name; returns the table."""
    rows = []
    for oname, hname, nchw in _tap_names(cfg):
        ref = taps[oname]
        if ref.dim() == 4 and nchw:
            ref = ref.permute(0, 2, 3, 1)
        try:
            raw = bb.activation(hname, batch)
        except Exception as exc:             # x1 of a frozen block is a temporary under the freeze policy's workspace plan (checked in the unfrozen cases)
            if "not retained" in str(exc):
                continue
            raise
        got = raw.view(dtype)[:ref.numel()].view(ref.shape if ref.dim() != 4 or nchw else ref.shape).float().cpu()
        if oname.endswith("attn.out"):          # oracle taps windows (B', N, C); the runtime keeps map order
            C = ref.shape[-1]
            s = int(oname.split(".")[1])
            ws, res = cfg.window_sizes[s], cfg.img_size // (4 * 2 ** s)
            B = batch
            if res != ws:
                ref = ref.view(B, res // ws, res // ws, ws, ws, C).transpose(2, 3).reshape(B, res * res, C)
            got = raw.view(dtype)[:ref.numel()].view(ref.shape).float().cpu()
        rows.append((oname, relerr(got, ref)))
    worst = max(rows, key=lambda r: r[1])
    print(f"\n[{label}] per-stage activation rel-L2 error (worst: {worst[0]} {worst[1]:.3e})")
    for n, e in rows:
        if n.endswith(".out") or n == "patch_embed":
            print(f"    {n:34s} {e:.3e}")
    bad = [(n, e) for n, e in rows if e > tol]
    assert not bad, (label, bad[:6])
    return rows


def _train_step_case(model_name, precision, N, centroids, unfrozen, seed=0, drop_path_rate=None, extra_trainable=()):
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from oracle import tinyvit_ref as R
    from oracle import step_ref as S
    torch.manual_seed(seed)
    kw = {} if drop_path_rate is None else dict(drop_path_rate=drop_path_rate)
    base = TinyViTAdapter(model_name, pretrained=False, precision=precision, **kw)
    _randomize(base.backbone, seed + 1)
    base = base.cuda()
    cfg = R.config_for(model_name, **kw)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True).cuda().train()
    assert model.precision == ("fp32" if precision == "fp32_split" else precision) and base.backbone.split == (precision == "fp32_split")
    if unfrozen:
        base.unfreeze_all()
    bb = base.backbone
    for n in extra_trainable:
        bb._params[n].requires_grad_(True)
    trainable = [n for n, p in bb.named_parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.randn(N, 4, 3, cfg.img_size, cfg.img_size, generator=g)
    labels = torch.stack([torch.rand(N, generator=g) * 360 - 180, torch.rand(N, generator=g) * 180 - 90], 1)
    keep = (torch.rand(bb.num_drop_slots, 4 * N, generator=g) > 0.3)
    rates = torch.tensor(bb.drop_rates).unsqueeze(1)
    scales = (keep.float() / (1 - rates)).contiguous().cuda()
    has_dp = max(bb.drop_rates) > 0
    bb.make_drop_scales = lambda batch, generator=None: (scales if has_dp else None)
    st = {k: v.detach().cpu().clone() for k, v in bb.state_dict().items()}
    W, b = model.cell_layer.weight.detach().cpu().clone(), model.cell_layer.bias.detach().cpu().clone()
    with gemm_launches() as launches:
        out = model(pixel_values=x.cuda(), labels=labels.cuda(), labels_clf=None)
        out.loss.backward()
        torch.cuda.synchronize()
    masks = [keep[s] for s in range(bb.num_drop_slots)] if has_dp else None
    emu = precision == "bf16"
    taps = {}
    # the oracle of the matching arithmetic: fp32 for the fp32 mode, bf16-storage-emulating for the bf16 mode
    st_o = {k: (t.clone().requires_grad_(True) if (t.is_floating_point() and "running" not in k and k in trainable) else t.clone()) for k, t in st.items()}
    Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    emb_o = R.forward(cfg, st_o, x.reshape(4 * N, 3, cfg.img_size, cfg.img_size), training=True, emulate_bf16=emu, drop_masks=masks, taps=taps)
    emb_o = emb_o.view(N, 4, -1)
    loss_o, logits_o = S.head_loss(emb_o, Wg, bg, torch.from_numpy(centroids), labels, emulate_bf16=emu)
    loss_o.backward()
    grads = {k: t.grad for k, t in st_o.items() if t.requires_grad and t.grad is not None}
    grads["cell_layer.weight"], grads["cell_layer.bias"] = Wg.grad, bg.grad
    taps = {k: v.detach() for k, v in taps.items()}
    return dict(model=model, bb=bb, cfg=cfg, out=out, taps=taps, emb_o=emb_o.detach(), loss_o=float(loss_o), logits_o=logits_o.detach(), grads=grads,
                trainable=trainable, N=N, launches=launches)


class gemm_launches:
    """Counts the GEMM-category launches of the enclosed region through libgg's event profiler (csrc/prof.h): ``.split`` = launches that carry the
    split-product flag (bit 4: gemm_nt_split3a / b, gemm_tn_split3, the plane-fed form), ``.plain`` = the other GEMM launches.  The fp32_split gates
    assert these, so that a routing threshold cannot silently send the mode's GEMMs back to the f32-MFMA kernels."""
    def __enter__(self):
        from geoguessr_ai_amd import _lib as L
        self.L = L
        L.lib().gg_prof_reset(); L.lib().gg_prof_enable(1)
        return self

    def __exit__(self, *exc):
        import ctypes as C
        L = self.L
        lib = L.lib()
        torch.cuda.synchronize()
        lib.gg_prof_enable(0)
        cat, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self.split = self.plain = 0
        self.split_flops = self.plain_flops = 0.0
        for i in range(lib.gg_prof_count()):
            L.check(lib.gg_prof_record(i, C.byref(cat), C.byref(ms), C.byref(fl), C.byref(by)), "gg_prof_record")
            if cat.value & 15 == 0:
                if cat.value & 16:
                    self.split += 1; self.split_flops += fl.value
                else:
                    self.plain += 1; self.plain_flops += fl.value
        lib.gg_prof_reset()
        return False


def split_launches_expected(cfg, trainable, head=True):
    """Split-product launches of one training step (forward + backward) of the TinyViT schedule when EVERY route is taken: four Linears per transformer
    block forward + four data gradients, four weight gradients per TRAINABLE block, and the dense convolutions of the ConvNorms that have planes
    (counted from the run itself: see the callers).  Returns (linears_fwd_and_dgrad, wgrads)."""
    blocks = sum(cfg.depths[1:])
    tb = sum(1 for s in range(1, 4) for i in range(cfg.depths[s]) if f"stages.{s}.blocks.{i}.mlp.fc1.weight" in trainable)
    return 8 * blocks, 4 * tb


def _grad_table(case, tol, label, median_tol=None):
    model, bb = case["model"], case["bb"]
    rows = []
    # a parameter whose effect is cancelled downstream (a bias in front of a conv + BatchNorm, e.g. the last fc2.bias of a stage) has a
    # gradient of exactly zero up to rounding noise (~1e-8) on both sides: not comparable, skipped by a noise floor
    floor = 1e-4 * float(np.median([float(g.norm()) for g in case["grads"].values()]))
    for name, gref in case["grads"].items():
        p = model.cell_layer.weight if name == "cell_layer.weight" else model.cell_layer.bias if name == "cell_layer.bias" else bb._params[name]
        assert p.grad is not None, name
        if float(gref.norm()) > floor:
            rows.append((name, relerr(p.grad, gref)))
        else:
            assert float(p.grad.norm()) < 10 * floor, (name, float(p.grad.norm()), floor)
    rows.sort(key=lambda r: -r[1])
    print(f"[{label}] per-tensor gradient rel-L2 error over {len(rows)} tensors: worst {rows[0][0]} {rows[0][1]:.3e}, median {rows[len(rows) // 2][1]:.3e}")
    bad = [r for r in rows if r[1] > tol]
    assert not bad, (label, bad[:8])
    if median_tol is not None:
        assert rows[len(rows) // 2][1] < median_tol, (label, "median", rows[len(rows) // 2])
    assert all(bb._params[n].grad is None for n in bb._params if n not in case["trainable"])


@pytest.mark.parametrize("model_name,N,unfrozen", [("tiny_vit_5m_224", 2, True), ("tiny_vit_21m_224", 4, False), ("tiny_vit_21m_224", 1, True), ("tiny_vit_11m_224", 2, False)])
def test_fp32_mode_train_step_matches_fp32_oracle(centroids, model_name, N, unfrozen):
    """Reference-precision mode: forward, loss, every stage's activations and every parameter gradient against the fp32 oracle at
    fp32-rounding tolerances (rtol 1e-4 on embeddings, loss 1e-5 rel)."""
    case = _train_step_case(model_name, "fp32", N, centroids, unfrozen, seed=11, drop_path_rate=0.1)
    label = f"fp32 {model_name} N={N} {'unfrozen' if unfrozen else 'ref-freeze'}"
    _compare_taps(case["bb"], case["cfg"], case["taps"], 4 * N, F32, 2e-4, label)
    emb = case["out"].embedding.detach().cpu()
    e_abs = float((emb - case["emb_o"]).abs().max())
    l_rel = abs(float(case["out"].loss) - case["loss_o"]) / case["loss_o"]
    print(f"[{label}] embedding max|err| {e_abs:.3e}, rel-L2 {relerr(emb, case['emb_o']):.3e}, loss rel {l_rel:.3e}")
    assert e_abs < 5e-4 and relerr(emb, case["emb_o"]) < 1e-4
    assert l_rel < 1e-5
    _grad_table(case, 2e-3, label)


def _fp32_gate(case, label):
    """The fp32 mode's training-step assertions (per-stage taps <= 2e-4, embedding 1e-4 / 5e-4 abs, loss 1e-5, every gradient tensor 2e-3)."""
    _compare_taps(case["bb"], case["cfg"], case["taps"], 4 * case["N"], F32, 2e-4, label)
    emb = case["out"].embedding.detach().cpu()
    e_abs = float((emb - case["emb_o"]).abs().max())
    l_rel = abs(float(case["out"].loss) - case["loss_o"]) / case["loss_o"]
    print(f"[{label}] embedding max|err| {e_abs:.3e}, rel-L2 {relerr(emb, case['emb_o']):.3e}, loss rel {l_rel:.3e}")
    assert e_abs < 5e-4 and relerr(emb, case["emb_o"]) < 1e-4
    assert l_rel < 1e-5
    _grad_table(case, 2e-3, label)


@pytest.mark.parametrize("model_name,N,unfrozen", [("tiny_vit_21m_224", 4, False), ("tiny_vit_21m_224", 1, False), ("tiny_vit_21m_384", 1, False), ("tiny_vit_5m_224", 3, True),
                                                   ("tiny_vit_11m_224", 2, True)])
def test_fp32_split_mode_passes_the_fp32_gate(centroids, model_name, N, unfrozen):
    """The gate of the "fp32_split" mode (f32 storage; GEMMs as fp32-accurate split products on the bf16 MFMA, the f32 activation split inside the GEMM's
    loader): the SAME assertions at the SAME tolerances as the fp32 mode's training-step test, under the reference freeze policy and with every parameter
    trainable.  At these batch sizes (4-16 images) the DEFAULT routing sends only the large-M calls to the split kernels (csrc/tinyvit.hip: a Linear needs
    128 tiles, a weight gradient 1024 rows) -- stage 1 and part of stage 2; the launch counts are printed.  The gates in which EVERY route is taken are
    test_fp32_split_gate_with_every_split_route_forced (thresholds lowered by dev switch, launch count asserted) and
    test_fp32_split_mode_gate_at_64_images (default thresholds at a size where all but two Linears of stage 3 qualify)."""
    case = _train_step_case(model_name, "fp32_split", N, centroids, unfrozen, seed=11, drop_path_rate=0.1)
    label = f"fp32_split {model_name} N={N} {'unfrozen' if unfrozen else 'ref-freeze'}"
    print(f"[{label}] GEMM launches: {case['launches'].split} split-product, {case['launches'].plain} f32-MFMA")
    assert case["launches"].split > 0
    _fp32_gate(case, label)


def test_fp32_split_mode_gate_at_64_images(centroids):
    """Headline model, reference freeze policy, 16 panoramas = 64 images, DEFAULT routing thresholds: every Linear of stages 1 and 2, qkv / fc1 of stage 3
    (M = 3 136: 13 x 14 / 13 x 18 tiles), their data gradients and every weight gradient of the trainable stage (M >= 1024) run as split products; only
    proj / fc2 of stage 3 (65 tiles) stay on the f32-MFMA kernel at this size.  Same assertions and tolerances as the fp32 mode's gate; the split
    launch count is asserted so the routing cannot fall back silently."""
    case = _train_step_case("tiny_vit_21m_224", "fp32_split", 16, centroids, False, seed=17, drop_path_rate=0.1)
    label = "fp32_split tiny_vit_21m_224 N=16 ref-freeze (default thresholds)"
    la = case["launches"]
    lin, wg = split_launches_expected(case["cfg"], case["trainable"])
    print(f"[{label}] GEMM launches: {la.split} split-product ({la.split_flops / 1e12:.3f} TFLOP), {la.plain} f32-MFMA ({la.plain_flops / 1e12:.3f} TFLOP); "
          f"block Linears fwd + dgrad {lin}, trainable-block weight gradients {wg}")
    # stage 3: proj / fc2 forward + data gradient of its two blocks (8 launches) are below the tile threshold; everything else of the Linear family qualifies
    assert la.split >= lin - 8 + wg, (la.split, lin, wg)
    assert la.split_flops > 0.75 * (la.split_flops + la.plain_flops)
    _fp32_gate(case, label)


@pytest.mark.parametrize("kernels", ["default", "generic_epilogue"])
def test_fp32_split_gate_with_every_split_route_forced(kernels):
    """The fp32 gate with EVERY split route taken at a batch the CPU oracle finishes in seconds: a subprocess (dev switches are read once per process) runs
    tools/split_gate.py under GG_DEV_SWITCHES=1 GG_SPLIT_MIN_TILES=1 GG_SPLIT_TN_MIN_M=1 -- TinyViT-21M-224 at 4 panoramas under the reference freeze policy
    and TinyViT-5M-224 at 3 panoramas with every parameter trainable: all block Linears (forward + data gradient), all weight gradients of trainable
    blocks and the ConvNorm convolutions as split products, the expected launch count (105 at the 21M schedule: the bench step's) asserted inside, fp32
    tolerances.  "generic_epilogue": the same gate with every split product leaving through the generic (runtime-switched) row epilogue, the form that
    plane outputs and column statistics take."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GG_DEV_SWITCHES="1", GG_SPLIT_MIN_TILES="1", GG_SPLIT_TN_MIN_M="1", GG_SPLIT_GATE_EXPECT_21M="105")
    if kernels == "generic_epilogue":
        env.update(GG_SPLIT3_NO_EC="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "split_gate.py")], env=env, capture_output=True, text=True, timeout=1500, cwd=root)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("-> ok") == 2


def test_fp32_split_mode_tracks_fp32_over_optimizer_steps(centroids):
    """The split mode reads the weights of its Linears from CACHED bf16 planes: after an optimizer step the planes of the trainable tensors must be re-split
    (gg_tinyvit_refresh_weights_masked).  Four AdamW steps at a large learning rate from the same initial state in both modes: losses and the trained
    parameters agree at fp32 rounding level -- with stale planes the second forward would already differ at the size of the first update."""
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from geoguessr_ai_amd.optim import AdamW
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 4, 3, 224, 224, generator=g).cuda()
    lab = torch.stack([torch.rand(3, generator=g) * 360 - 180, torch.rand(3, generator=g) * 180 - 90], 1).cuda()
    runs = {}
    for precision in ("fp32", "fp32_split"):
        torch.manual_seed(21)
        base = TinyViTAdapter("tiny_vit_5m_224", pretrained=False, precision=precision, drop_path_rate=0.0)
        _randomize(base.backbone, 22)
        model = SuperGuessr(base.cuda(), panorama=True, should_smooth_labels=True).cuda().train()
        for p_ in model.parameters():
            p_.requires_grad_(True)
        opt = AdamW(model, lr=3e-3, betas=(0.9, 0.999), weight_decay=0.01)
        losses = []
        for _ in range(4):
            out = model(pixel_values=x, labels=lab)
            out.loss.backward()
            opt.step(); opt.zero_grad()
            losses.append(float(out.loss))
        runs[precision] = (losses, {n: p_.detach().float().cpu().clone() for n, p_ in model.named_parameters()})
    la, lb = runs["fp32"][0], runs["fp32_split"][0]
    print("[fp32 vs fp32_split, 4 steps] losses", la, lb)
    assert abs(la[0] - la[-1]) > 1e-3 * abs(la[0])                     # the steps are large enough to matter
    # (a forward on stale planes would repeat the previous step's loss: 9.3 instead of 6.0.  Four steps that take the loss from 9.3 to 3.8 amplify rounding-level
    # differences between the two product forms: 2e-5 after the first update, a few 1e-4 after the third)
    assert abs(la[1] - lb[1]) <= 1e-4 * abs(la[1]), (la, lb)
    for a, b in zip(la, lb):
        assert abs(a - b) <= 2e-3 * abs(a), (la, lb)
    # (matrices; bias / norm vectors that start at zero take Adam's sign-like first updates from gradients near zero: percent-level differences, no signal)
    errs = sorted(((relerr(runs["fp32_split"][1][n], t), n) for n, t in runs["fp32"][1].items() if t.dim() >= 2), reverse=True)
    print("[fp32 vs fp32_split, 4 steps] worst matrix rel-L2", errs[:4])
    assert errs[0][0] < 5e-3
    vec = max(relerr(runs["fp32_split"][1][n], t) for n, t in runs["fp32"][1].items() if t.dim() == 1 and t.numel() > 1)
    assert vec < 5e-2


def test_a_half_frozen_parameter_pair_is_refused_by_name(centroids):
    """The TinyViT schedule forms the gradients of a (weight, bias) / (gamma, beta) pair together; a mask that trains ``mlp.norm.bias`` while
    ``mlp.norm.weight`` stays frozen has no schedule and must fail loudly in backward (it used to leave the bias gradient at zero in the fused
    frozen-block path) -- while whole modules added to the freeze policy train and match the oracle."""
    from geoguessr_ai_amd import _lib as L
    with pytest.raises(L.GgError, match="must be trainable or frozen together"):
        _train_step_case("tiny_vit_5m_224", "fp32", 2, centroids, False, seed=13, drop_path_rate=0.0, extra_trainable=("stages.1.blocks.0.mlp.norm.bias",))
    extra = ("stages.1.blocks.0.mlp.norm.bias", "stages.1.blocks.0.mlp.norm.weight", "stages.1.blocks.1.local_conv.bn.bias", "stages.1.blocks.1.local_conv.bn.weight")
    case = _train_step_case("tiny_vit_5m_224", "fp32", 2, centroids, False, seed=13, drop_path_rate=0.0, extra_trainable=extra)
    assert all(n in case["grads"] for n in extra)
    _grad_table(case, 2e-3, "fp32 5m extra norm modules in frozen stages")


@pytest.mark.parametrize("model_name,N", [("tiny_vit_21m_224", 4), ("tiny_vit_5m_224", 3)])
def test_bf16_mode_train_step_matches_bf16_emulating_oracle(centroids, model_name, N):
    """Headline model in the bf16 mode against the oracle that rounds storage to bf16 at the same points: SURVEY 8(c)'s bf16 numbers --
    embedding rel err <= 2e-2, per-stage activations, per-tensor gradient error."""
    case = _train_step_case(model_name, "bf16", N, centroids, False, seed=21)
    label = f"bf16 {model_name} N={N}"
    # bf16 storage: ~60 rounding points of 2^-9 between the image and stage 3 -> a few percent of drift on the raw residual stream is
    # rounding, not algorithm; the bound that matters is SURVEY 8(c)'s 2e-2 on the embedding (after head.norm), asserted below.  A wrong
    # layer shows up as a jump by an order of magnitude at its tap (the fp32-mode test above pins the same code path to 1e-5).
    rows = _compare_taps(case["bb"], case["cfg"], case["taps"], 4 * N, BF, 8e-2, label)
    errs = dict(rows)
    assert errs["patch_embed"] < 1e-2 and errs["stages.1.downsample.out"] < 2e-2
    emb = case["out"].embedding.detach().cpu()
    rel = relerr(emb, case["emb_o"])
    l_rel = abs(float(case["out"].loss) - case["loss_o"]) / case["loss_o"]
    print(f"[{label}] embedding rel-L2 {rel:.3e} max|err| {float((emb - case['emb_o']).abs().max()):.3e}, loss rel {l_rel:.3e}")
    assert rel < 2e-2 and l_rel < 2e-3
    # gradients cross the same ~60 bf16 rounding points twice (forward values, backward gradients): the deepest tensors (patch_embed, reached
    # through all 12 blocks) carry ~10 % relative L2 noise, the stage-3 / head tensors ~3 %; every tensor keeps cosine > 0.98 (rel < 0.2)
    _grad_table(case, 2e-1, label, median_tol=6e-2)


@pytest.mark.parametrize("precision", ["fp32", "fp32_split", "bf16"])
def test_headline_model_prediction_agreement(centroids, precision):
    """top-1 geocell agreement >= 99 % and top-5 overlap >= 4.9 / 5 on synthetic batches -- TinyViT-21M-224 + 12 647-cell head,
    eval mode, 64 panoramas, against the fp32 oracle's predictions (ties closer than 1e-4 in logit are not counted against)."""
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    from geoguessr_ai_amd.models.super_guessr import SuperGuessr
    from oracle import tinyvit_ref as R
    torch.manual_seed(5)
    base = TinyViTAdapter("tiny_vit_21m_224", pretrained=False, precision=precision)
    _randomize(base.backbone, 6)
    model = SuperGuessr(base, panorama=True, should_smooth_labels=True).cuda().eval()
    with torch.no_grad():
        model.cell_layer.weight.copy_(0.3 * torch.randn(model.cell_layer.weight.shape))      # logit gaps well above rounding
    cfg = R.config_for("tiny_vit_21m_224")
    st = {k: v.detach().cpu().clone() for k, v in base.backbone.state_dict().items()}
    N = 64
    x = torch.randn(N, 4, 3, 224, 224, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        with gemm_launches() as la:
            out = model(pixel_values=x.cuda())
        if precision == "fp32_split":       # 256 images: every Linear of every transformer block qualifies for the split kernels (stage 3: 49 x 5 tiles)
            print(f"[fp32_split, 256 images] GEMM launches: {la.split} split-product, {la.plain} f32-MFMA")
            assert la.split >= 4 * sum(R.config_for("tiny_vit_21m_224").depths[1:])
        else:
            assert la.split == 0
        emb_o = torch.cat([R.forward(cfg, st, x[i:i + 8].reshape(-1, 3, 224, 224), training=False) for i in range(0, N, 8)]).view(N, 4, -1)
        logits_o = F.linear(emb_o.mean(1), model.cell_layer.weight.cpu(), model.cell_layer.bias.cpu())
    top_o = logits_o.topk(5, -1).indices
    gap = (logits_o.topk(2, -1).values[:, 0] - logits_o.topk(2, -1).values[:, 1])
    agree = (out.preds_geocell.cpu() == top_o[:, 0]) | (gap < 1e-4)
    overlap = np.mean([len(set(a.tolist()) & set(b.tolist())) for a, b in zip(out.top5_geocells.indices.cpu(), top_o)])
    rel = relerr(out.embedding, emb_o)
    print(f"\n[{precision}] top-1 agreement {float(agree.float().mean()):.4f}, top-5 overlap {overlap:.3f}/5, embedding rel-L2 vs fp32 oracle {rel:.3e}")
    assert float(agree.float().mean()) >= 0.99 and overlap >= 4.9
    assert rel < (2e-2 if precision == "bf16" else 1e-4)
    # lat/lon are a centroid gather: identical wherever the arg-max agrees
    same = out.preds_geocell.cpu() == top_o[:, 0]
    np.testing.assert_array_equal(out.preds_LLH.cpu().numpy()[same.numpy()], centroids[top_o[:, 0].numpy()][same.numpy()])


def test_fp32_split_inference_embeddings_match_the_fp32_mode():
    """Inference in the fp32_split mode (every transformer block's qkv / proj / fc1 / fc2 as split-bf16 products from 64 tokens per call on: the bulk-embedding job of the "next" row f2)
    gives the fp32 mode's embeddings to fp32 rounding (rel-L2 <= 1e-5: the two product forms differ by ~3e-7 per GEMM)."""
    import warnings
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    outs = {}
    x = torch.randn(8, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    for prec in ("fp32", "fp32_split"):
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = TinyViTAdapter("tiny_vit_21m_224", pretrained=False, precision=prec)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for name, p in m.backbone.named_parameters():
                if name.endswith(("bn.weight", "norm.weight")): p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
                elif name.endswith(".bias") and p.dim() == 1: p.copy_(0.1 * torch.randn(p.shape, generator=g))
                elif name.endswith("attention_biases"): p.copy_(0.5 * torch.randn(p.shape, generator=g))
                elif name.endswith(".weight") and p.dim() == 2: p.copy_(0.05 * torch.randn(p.shape, generator=g))
        m = m.cuda().eval()
        with torch.no_grad():
            outs[prec] = m(pixel_values=x).pooler_output.clone()
        del m
    assert torch.isfinite(outs["fp32_split"]).all() and not torch.equal(outs["fp32"], outs["fp32_split"])      # the split path did run
    assert relerr(outs["fp32_split"].cpu(), outs["fp32"].cpu()) < 1e-5
