"""The three kernels of include/gg_fp8.h on the GPU against the contract restated in tests/clip_fp8_ref.py.

1. gg_quant_rows_e4m3: codes and scales bit for bit (zero row, one-nonzero row, subnormal range, exact rounding ties; fp16 and f32 input, padded rows).
2. gg_gemm_nt_e4m3 on exact integer data, bit for bit: A = I against an asymmetric W (any k-permutation between the operand maps, or a row / column swap, moves
   an element), and sparse {-1, 0, 1} x [-8, 8] products with power-of-two scales whose results are exact in fp16.
3. gg_gemm_nt_e4m3 on random codes and scales, every epilogue, against fp64 on the dequantised operands.  Bound (the fp16 GEMM's form): the
   e4m3 x e4m3 products are exact, the f32 accumulation of K terms is within K * 2^-24 of sum |terms| (taken twice), and the result is rounded to fp16 once
   (2^-11 relative; the residual form rounds the sum once more); QuickGELU adds the device exponential's 1e-6 relative.
4. gg_layernorm_fwd_e4m3 against fp64 LayerNorm: the scale within 1e-5 of amax(y) / 448, every element within half an e4m3 spacing (+ 1e-5 amax).
5. every refusal names itself and leaves the outputs untouched."""
import ctypes as C

import pytest
import torch

from tests import clip_fp8_ref as R

pytestmark = pytest.mark.gpu
F16, F32, U8 = torch.float16, torch.float32, torch.uint8


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as O
    return O


def _codes_of(v):
    """Exactly representable values -> e4m3fn codes."""
    c = v.to(torch.float32).to(torch.float8_e4m3fn)
    assert torch.equal(c.to(torch.float32), v.to(torch.float32))
    return c.view(U8)


def _padded(t, ld, fill):
    """t [M, K] as a view with row stride ld of a buffer pre-filled with `fill`."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


# ------------------------------------------------------------------------------------------------------------------- 1. the row quantiser
def _quant_input(M, K, dtype):
    g = torch.Generator().manual_seed(1000 * M + K)
    x = torch.randn(M, K, generator=g) * (10.0 ** torch.randint(-3, 3, (M, 1), generator=g).float())
    ties = torch.tensor([17.0, 19.0, -1.0625, 2.0 ** -10, 3 * 2.0 ** -10, 432.0, -2.0 ** -10, 208.0, -17.0, 5 * 2.0 ** -10, 2.0 ** -6 + 2.0 ** -10, -0.0, 464.0 / 2, 26.0])
    kinds = ["ties", "zero", "one", "subnormal"]
    for r in range(min(M, 4)):
        kind = kinds[r]
        if kind == "ties":                                  # amax = 448: inv == 1, scale == 1, the listed values sit on e4m3 rounding ties
            x[r] = torch.randint(-8, 9, (K,), generator=g).float()
            x[r, 0] = -448.0
            x[r, 1:1 + len(ties)] = ties
        elif kind == "zero":
            x[r] = 0.0
        elif kind == "one":
            x[r] = 0.0; x[r, K - 3] = -0.37
        else:                                               # one large element; the rest lands in and around e4m3's subnormal range after scaling
            x[r] = torch.randn(K, generator=g) * 2.0 ** -13
            x[r, 5] = 3.0
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("K", [128, 512, 4096])
@pytest.mark.parametrize("M", [1, 5, 67])
def test_quant_rows_bit_for_bit(ops, M, K, dtype):
    x = _quant_input(M, K, dtype)
    codes_ref, scale_ref = R.quant_rows(x.float())
    xv = _padded(x, K + 24, 7.0)
    q = torch.full((M, K + 40), 0xEE, dtype=U8, device="cuda")
    codes, scale = ops.quant_rows_e4m3(xv, q=q[:, :K])
    torch.cuda.synchronize()
    assert torch.equal(scale.cpu().view(torch.int32), scale_ref.view(torch.int32)), (scale.cpu(), scale_ref)
    bad = codes.cpu() != codes_ref
    assert not bool(bad.any()), (int(bad.sum()), torch.nonzero(bad)[:5].tolist(), codes.cpu()[bad][:5].tolist(), codes_ref[bad][:5].tolist())
    assert bool((q[:, K:] == 0xEE).all())                   # the padding of the code rows is not written


# ------------------------------------------------------------------------------------------------------------------- 2. exact integer data
@pytest.mark.parametrize("K,N", [(128, 48), (256, 144)])
def test_gemm_identity_against_asymmetric_w(ops, K, N):
    g = torch.Generator().manual_seed(K)
    W = torch.randint(-8, 9, (N, K), generator=g).float()
    assert not torch.equal(W[:min(N, K), :min(N, K)], W[:min(N, K), :min(N, K)].T)
    A = torch.eye(K)
    out = ops.gemm_nt_e4m3(_codes_of(A).cuda(), _codes_of(W).cuda(), torch.ones(K, device="cuda"), torch.ones(N, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().float(), W.T.contiguous())


@pytest.mark.parametrize("K", [128, 512, 4096])
def test_gemm_sparse_integers_bit_for_bit(ops, K):
    M, N = 67, 192
    g = torch.Generator().manual_seed(K + 1)
    A = torch.zeros(M, K)
    for m in range(M):                                      # at most 200 nonzeros per row: |sum| <= 200 * 8 < 2048, exact in fp16
        idx = torch.randperm(K, generator=g)[:min(K, 200)]
        A[m, idx] = torch.randint(0, 2, (idx.numel(),), generator=g).float() * 2 - 1
    W = torch.randint(-8, 9, (N, K), generator=g).float()
    sa = 2.0 ** torch.randint(-2, 3, (M,), generator=g).float()
    sw = 2.0 ** torch.randint(-2, 3, (N,), generator=g).float()
    ref = (A.double() @ W.double().T) * sa.double()[:, None] * sw.double()[None, :]
    assert float(ref.abs().max()) <= 2048 * 16 and torch.equal(ref.to(F16).double(), ref)
    Av, Wv = _padded(_codes_of(A), K + 16, 0x7F), _padded(_codes_of(W), K + 48, 0x7F)      # (the padding holds NaN codes)
    out = ops.gemm_nt_e4m3(Av, Wv, sa.cuda(), sw.cuda())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), ref)


# ------------------------------------------------------------------------------------------------------------------- 3. random codes, every epilogue
_REF = {}


def _gemm_case(M, N, K):
    """Operands, and the fp64 products on the dequantised operands, once per shape."""
    if (M, N, K) not in _REF:
        g = torch.Generator().manual_seed(M * 131 + N * 7 + K)
        ca, sa = R.quant_rows(torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g)))
        cw, sw = R.quant_rows(torch.randn(N, K, generator=g) * (K ** -0.5) * (0.5 + torch.rand(N, 1, generator=g)))
        a, w = R.decode(ca), R.decode(cw)
        s = sa.double()[:, None] * sw.double()[None, :]
        bias = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g).to(F16)
        _REF[(M, N, K)] = dict(ca=ca, sa=sa, cw=cw, sw=sw, bias=bias, res=res, acc=(a @ w.T) * s, mag=(a.abs() @ w.abs().T) * s)
    return _REF[(M, N, K)]


@pytest.mark.parametrize("epi", ["plain", "bias", "quick_gelu", "residual", "residual_inplace"])
@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (15, 192, 512), (17, 384, 128), (200, 64, 4096), (577, 192, 512), (577, 384, 4096), (200, 384, 512)])
def test_gemm_random_codes_every_epilogue(ops, M, N, K, epi):
    c = _gemm_case(M, N, K)
    Av, Wv = _padded(c["ca"], K + 32, 0x7F), _padded(c["cw"], K + 16, 0x7F)
    bias = None if epi == "plain" else c["bias"].cuda()
    pre = c["acc"] + (0 if epi == "plain" else c["bias"].double()[None, :])
    acc_tol = 2.0 * K * 2.0 ** -24 * c["mag"]
    outbuf = torch.full((M, N + 24), 9.0, dtype=F16, device="cuda")
    out = outbuf[:, :N]
    if epi == "quick_gelu":
        ref = pre * torch.sigmoid(1.702 * pre)
        tol = 1.13 * acc_tol + 2.0 ** -11 * ref.abs() + 1e-6 * (pre.abs() + 1) + 2.0 ** -25      # (|QuickGELU'| <= 1.13)
        ops.gemm_nt_e4m3(Av, Wv, c["sa"].cuda(), c["sw"].cuda(), bias=bias, act="quick_gelu", out=out)
    elif epi.startswith("residual"):
        ref = pre + c["res"].double()
        tol = acc_tol + 2.0 ** -11 * (pre.abs() + ref.abs()) + 2.0 ** -24
        if epi == "residual_inplace":
            out.copy_(c["res"].cuda())
            ops.gemm_nt_e4m3(Av, Wv, c["sa"].cuda(), c["sw"].cuda(), bias=bias, residual=out, out=out)
        else:
            ops.gemm_nt_e4m3(Av, Wv, c["sa"].cuda(), c["sw"].cuda(), bias=bias, residual=_padded(c["res"], N + 8, 3.0), out=out)
    else:
        ref = pre
        tol = acc_tol + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        ops.gemm_nt_e4m3(Av, Wv, c["sa"].cuda(), c["sw"].cuda(), bias=bias, out=out)
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    worst = float((err / tol).max())
    print(f"\n[gemm_nt_e4m3 {M}x{N}x{K} {epi}] worst err / bound {worst:.3f}, max err {float(err.max()):.3e}")
    assert worst <= 1.0
    assert bool((outbuf[:, N:] == 9.0).all())


# ------------------------------------------------------------------------------------------------------------------- 4. LayerNorm + quantiser
@pytest.mark.parametrize("Cc", [128, 768, 1024])
@pytest.mark.parametrize("M", [1, 5, 67])
def test_layernorm_e4m3(ops, M, Cc):
    g = torch.Generator().manual_seed(M * 17 + Cc)
    x = torch.randn(M, Cc, generator=g) * 2.0
    if M > 1:
        x[1] = 1000.0 + torch.randint(-8, 9, (Cc,), generator=g).float() * 0.5      # a large common offset (the noise is representable in fp16 beside it)
        x[2] = 3.25                                                                # a constant row: y = beta
    x = x.to(F16)
    gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    q = torch.full((M, Cc + 8), 0xEE, dtype=U8, device="cuda")
    codes, scale = ops.layernorm_fwd_e4m3(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5, q=q[:, :Cc])
    torch.cuda.synchronize()
    y = torch.nn.functional.layer_norm(x.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
    amax = y.abs().amax(-1)
    sc = scale.cpu().double()
    assert bool(((sc - amax / 448.0).abs() <= 1e-5 * amax / 448.0).all()), ((sc * 448.0 / amax) - 1).abs().max()
    val = R.decode(codes.cpu())
    assert not bool(((codes.cpu() & 0x7F) == 0x7F).any())
    err = (val * sc[:, None] - y).abs()
    bound = sc[:, None] * 0.5 * R.e4m3_spacing(y / sc[:, None]) + 1e-5 * amax[:, None]
    print(f"\n[layernorm_fwd_e4m3 {M}x{Cc}] worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((q[:, Cc:] == 0xEE).all())


# ------------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_name_themselves_and_touch_nothing():
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    M, N, K = 8, 64, 128
    A = torch.zeros(M, K, dtype=U8, device="cuda"); W = torch.zeros(N, 256, dtype=U8, device="cuda")
    sa, sw = torch.ones(M, device="cuda"), torch.ones(N, device="cuda")
    out = torch.full((M, N), 5.0, dtype=F16, device="cuda")
    other = torch.full((M, N), 6.0, dtype=F16, device="cuda")
    stats = torch.full((4, 2, N), 7.0, device="cuda")

    def args(**kw):
        a = L.GemmArgs()
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N, a.K, a.split_k = A.data_ptr(), K, W.data_ptr(), 256, out.data_ptr(), N, M, N, K, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for word, kw in (("preact", dict(preact=other.data_ptr())), ("dact", dict(dact_preact=other.data_ptr(), dact=2)), ("colstats", dict(colstats=stats.data_ptr())),
                     ("split", dict(split_k=2)), ("K must be a multiple of 128", dict(K=192)), ("K must be a multiple of 128", dict(K=64)),
                     ("N must be a multiple of 16", dict(N=40)), ("act", dict(act=1))):
        assert lib.gg_gemm_nt_e4m3(C.byref(args(**kw)), sa.data_ptr(), sw.data_ptr(), L.stream()) != 0, word
        msg = lib.gg_last_error().decode()
        assert "gg_gemm_nt_e4m3" in msg and word in msg, (word, msg)
    q = torch.full((M, K), 0xEE, dtype=U8, device="cuda"); s = torch.full((M,), 3.0, device="cuda")
    x = torch.ones(M, K, dtype=F16, device="cuda")
    assert lib.gg_quant_rows_e4m3(x.data_ptr(), 0, K, M, 100, q.data_ptr(), K, s.data_ptr(), L.stream()) != 0 and "gg_quant_rows_e4m3" in lib.gg_last_error().decode()
    assert lib.gg_layernorm_fwd_e4m3(x.data_ptr(), sa.data_ptr(), sa.data_ptr(), M, 100, L.f32(1e-5), q.data_ptr(), K, s.data_ptr(), L.stream()) != 0
    assert "gg_layernorm_fwd_e4m3" in lib.gg_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((other == 6.0).all()) and bool((stats == 7.0).all()) and bool((q == 0xEE).all()) and bool((s == 3.0).all())
