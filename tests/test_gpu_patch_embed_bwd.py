"""The backward of patch_embed.conv2 in the fp32_split mode: the data gradient by input parity with BatchNorm1's backward reduce as epilogue
(include/gg_conv_dgrad_parity.h) and the weight gradient on split products with the whole output resident in one workgroup (include/gg_wgrad_resident.h).

Data gradient.  References: fp64 on the CPU (conv_transpose2d, the GELU' . BN factor and the two sums in float64) and today's two launches on the same tensors
(gg_gemm_nt_split3_af32 for dcol, then gg_col2im_nhwc_bnbwd_f32).  Bound: the rel-L2 error against fp64 of dz and of each of the two sums is at most 1.5 times that
of today's path (the order of the tap sums differs, so no bit equality).  Shapes: 48 -> 96 channels, two images with maps 4 x 4, 6 x 10 and 10 x 6 -- every class meets
its missing border tap, and a swapped stride shows -- and three images of 2 x 2, where every odd pixel has a tap outside the map.  Both errors are printed.

Weight gradient.  References: fp64 on the CPU, and gg_gemm_tn_f32 -- the launch the resident form replaces in the fp32_split step, not the code under test -- on the same tensors.
Bound: the rel-L2 error of the resident form against fp64 is at most 1.5 times that of gg_gemm_tn_f32, the margin the split-GEMM tests give over the f32 kernel.
Both errors are printed.  Shapes: conv2's output (N, K) = (96, 432) over 1024 + 37 rows (four slabs, the last one partial: six stages and five rows) and over 64
rows (two slabs of one stage); a narrower output that exercises the column masks; and an output that does not fit, refused by name."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


# ------------------------------------------------------------------------------------------- data gradient
CIN, COUT, NPARTS = 48, 96, 8


def _gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z / 2.0 ** 0.5)) + z * torch.exp(-0.5 * z * z) / (2.0 * torch.pi) ** 0.5


def _dgrad_case(B, H, W):
    g = torch.Generator().manual_seed(100 * H + W + B)
    H0, W0 = H // 2, W // 2
    dy = torch.randn(B, H0, W0, COUT, generator=g)
    y = torch.randn(B, H, W, CIN, generator=g)
    w = torch.randn(COUT, CIN, 3, 3, generator=g) / (9 * CIN) ** 0.5
    gamma, beta = 1.0 + 0.3 * torch.randn(CIN, generator=g), 0.3 * torch.randn(CIN, generator=g)
    y64 = y.double().reshape(-1, CIN)
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    stat = torch.cat([mean, (var + 1e-5).rsqrt()]).float()                       # [mean | rstd], BatchNorm1's statistics of y itself
    wt = w.permute(2, 3, 1, 0).reshape(9 * CIN, COUT).contiguous()                 # Wt[(ky 3 + kx) Cin + c][co]
    da = torch.nn.functional.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1).reshape(-1, CIN)
    xh = (y64 - stat[:CIN].double()) * stat[CIN:].double()
    dz = da * _gelu_grad64(gamma.double() * xh + beta.double())
    return {"dy": dy, "y": y, "wt": wt, "gamma": gamma, "beta": beta, "stat": stat, "dz": dz, "s": dz.sum(0), "q": (dz * xh).sum(0)}


@pytest.mark.parametrize("B,H,W", [(2, 4, 4), (2, 6, 10), (2, 10, 6), (3, 2, 2)])
def test_data_gradient_by_parity_against_fp64_and_todays_path(L, B, H, W):
    lib, st = L.lib(), L.stream()
    c = _dgrad_case(B, H, W)
    M1, M0, K9 = B * H * W, B * (H // 2) * (W // 2), 9 * CIN
    dy, y, wt, stat, gamma, beta = (c[k].cuda().contiguous() for k in ("dy", "y", "wt", "stat", "gamma", "beta"))
    assert lib.gg_conv3x3s2_dgrad_fits(H, W, CIN, COUT) == 1

    def errs(dz, part):
        dz, part = dz.cpu().double(), part.cpu().double().sum(0)
        return tuple(float((a - b).norm() / b.norm()) for a, b in ((dz, c["dz"]), (part[0], c["s"]), (part[1], c["q"])))
    # today's path: dcol = dy . Wt^T as a split product, then the gather with the BatchNorm-backward reduce
    planes = torch.empty((3, K9, COUT), dtype=torch.bfloat16, device="cuda")
    L.check(lib.gg_split3_bf16(wt.data_ptr(), K9, COUT, COUT, planes.data_ptr(), st), "gg_split3_bf16")
    dcol = torch.empty(M0, K9, device="cuda")
    a = L.Split3Args()
    a.b_planes, a.ldb, a.M, a.N, a.K, a.C, a.ldc = planes.data_ptr(), COUT, M0, K9, COUT, dcol.data_ptr(), K9
    L.check(lib.gg_gemm_nt_split3_af32_stats(C.byref(a), dy.data_ptr(), COUT, 0, None, st), "gg_gemm_nt_split3_af32_stats")
    dz_old, part_old = torch.full((M1, CIN), float("nan"), device="cuda"), torch.full((NPARTS, 2, CIN), float("nan"), device="cuda")
    L.check(lib.gg_col2im_nhwc_bnbwd_f32(dcol.data_ptr(), y.data_ptr(), stat.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1, dz_old.data_ptr(), part_old.data_ptr(),
                                         NPARTS, B, H, W, CIN, st), "gg_col2im_nhwc_bnbwd_f32")
    # the parity form
    scratch = torch.empty(lib.gg_conv3x3s2_dgrad_planes_bytes(CIN, COUT), dtype=torch.uint8, device="cuda")
    dz_new, part_new = torch.full((M1, CIN), float("nan"), device="cuda"), torch.full((NPARTS, 2, CIN), float("nan"), device="cuda")
    L.check(lib.gg_conv3x3s2_dgrad_bnbwd_split3(dy.data_ptr(), wt.data_ptr(), COUT, y.data_ptr(), stat.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1, dz_new.data_ptr(),
                                                part_new.data_ptr(), NPARTS, scratch.data_ptr(), B, H, W, CIN, COUT, st), "gg_conv3x3s2_dgrad_bnbwd_split3")
    torch.cuda.synchronize()
    e_old, e_new = errs(dz_old, part_old), errs(dz_new, part_new)
    print(f"[conv2 data gradient B={B} map {H}x{W}] rel-L2 against fp64 (dz, sum dz, sum dz xhat): parity {e_new[0]:.3e} {e_new[1]:.3e} {e_new[2]:.3e}; "
          f"gemm + col2im {e_old[0]:.3e} {e_old[1]:.3e} {e_old[2]:.3e}")
    for what, n, o in zip(("dz", "sum dz", "sum dz xhat"), e_new, e_old):
        assert n <= 1.5 * o, (what, n, o)


def test_data_gradient_refuses_shapes_it_does_not_cover(L):
    lib = L.lib()
    t = torch.zeros(4096, device="cuda")
    p = t.data_ptr()
    for H, W, cin, cout in ((5, 4, 48, 96), (4, 6, 32, 64), (4, 4, 48, 80)):
        assert lib.gg_conv3x3s2_dgrad_fits(H, W, cin, cout) == 0
        assert lib.gg_conv3x3s2_dgrad_bnbwd_split3(p, p, cout, p, p, p, p, 1, p, p, 4, p, 1, H, W, cin, cout, L.stream()) != 0
        assert b"needs an even input map, Cin = 48 and Cout a multiple of 32" in lib.gg_last_error()
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ------------------------------------------------------------------------------------------- weight gradient
def _operands(M, N, K, mixed):
    g = torch.Generator().manual_seed(1000 * M + N + K + int(mixed))
    dY, X = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    sy, sx = torch.ones(N), torch.ones(K)
    if mixed:            # columns of both operands scaled by 2^-20, 1 or 2^20 (exact): every output element keeps its own magnitude class
        sy = 2.0 ** (20 * torch.randint(-1, 2, (N,), generator=g).float())
        sx = 2.0 ** (20 * torch.randint(-1, 2, (K,), generator=g).float())
    return dY * sy, X * sx, sy[:, None].double() * sx[None, :].double()


def _reduced(L, fn, splits_fn, dY, X, M, N, K, resident):
    lib, st = L.lib(), L.stream()
    splits = splits_fn(M, N, K)
    assert splits >= 1, lib.gg_last_error()
    part = torch.full((splits, N, K), float("nan"), device="cuda")
    if resident:
        L.check(fn(dY.data_ptr(), N, X.data_ptr(), K, M, N, K, part.data_ptr(), splits, st), "gg_gemm_tn_split3_resident")
    else:
        L.check(fn(dY.data_ptr(), N, X.data_ptr(), K, M, N, K, None, 0, part.data_ptr(), splits, st), "gg_gemm_tn_f32")
    out = torch.empty(N, K, device="cuda")
    L.check(lib.gg_splitk_reduce(part.data_ptr(), out.data_ptr(), N * K, splits, 0, L.f32(1.0), st), "gg_splitk_reduce")
    torch.cuda.synchronize()
    return out.cpu().double(), splits


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("M,N,K", [(1024 + 37, 96, 432), (64, 96, 432), (300, 64, 288)])
def test_resident_weight_gradient_against_fp64_and_the_f32_kernel(L, M, N, K, mixed):
    """dW = dY^T X.  The error is taken over the outputs divided by their columns' power-of-two scales (all ones in the plain case), so that with mixed magnitudes the
    small classes count as much as the large one."""
    lib = L.lib()
    dY, X, scale = _operands(M, N, K, mixed)
    ref = (dY.double().t() @ X.double()) / scale
    dYd, Xd = dY.cuda(), X.cuda()
    new, s_new = _reduced(L, lib.gg_gemm_tn_split3_resident, lib.gg_gemm_tn_split3_resident_splits, dYd, Xd, M, N, K, True)
    old, s_old = _reduced(L, lib.gg_gemm_tn_f32, lib.gg_gemm_tn_f32_splits, dYd, Xd, M, N, K, False)
    e_new = float((new / scale - ref).norm() / ref.norm())
    e_old = float((old / scale - ref).norm() / ref.norm())
    print(f"[resident weight gradient M={M} N={N} K={K} mixed={mixed}] rel-L2 against fp64: resident {e_new:.3e} ({s_new} slabs), gg_gemm_tn_f32 {e_old:.3e} ({s_old} slabs)")
    assert e_new <= 1.5 * e_old, (e_new, e_old)
    if (M, N, K) == (1024 + 37, 96, 432):
        assert s_new == 4 and M % 288 == 197                      # the last slab is partial


@pytest.mark.parametrize("N,K", [(128, 432), (96, 452)])
def test_an_output_that_does_not_fit_is_refused_by_name(L, N, K):
    lib = L.lib()
    M = 256
    dY, X, part = torch.zeros(M, N, device="cuda"), torch.zeros(M, K, device="cuda"), torch.full((N * K,), 7.0, device="cuda")
    assert lib.gg_gemm_tn_split3_resident_fits(N, K) == 0 and lib.gg_gemm_tn_split3_resident_fits(96, 432) == 1
    assert lib.gg_gemm_tn_split3_resident_splits(M, N, K) < 0
    assert f"the {N} x {K} output does not fit one workgroup".encode() in lib.gg_last_error()
    assert lib.gg_gemm_tn_split3_resident(dY.data_ptr(), N, X.data_ptr(), K, M, N, K, part.data_ptr(), 1, L.stream()) != 0
    assert f"the {N} x {K} output does not fit one workgroup".encode() in lib.gg_last_error()
    torch.cuda.synchronize()
    assert bool((part == 7.0).all())                              # a refused call writes nothing


def test_routing_changes_only_patch_embed_gradients():
    """tools/patch_embed_bwd_check.py in a subprocess under the dev switch that lets the split routes be taken at 8 images: one step of tiny_vit_21m_224 under the
    reference freeze policy with both new routes on and off -- loss, embedding and every other gradient equal, patch_embed's gradients within the f32 kernels' own
    tolerances (far inside the fp32 gate's), exactly one more split launch."""
    env = dict(os.environ, GG_DEV_SWITCHES="1", GG_SPLIT_MIN_TILES="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "patch_embed_bwd_check.py")], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("-> ok") == 1
