"""Memory discipline of include/gg_wgrad_resident.h and include/gg_conv_dgrad_parity.h, in the way tests/test_gpu_guards.py holds include/gg.h: every tensor of the call lives in a
guarded buffer (tests/guards.py), each case runs under the NaN fill and the large-finite fill of bands, row padding and neighbouring columns, and asserts that the
inputs are unchanged, that only -- and all of -- the logical outputs were written, that the two runs agree bit for bit, and that the values match an fp64 reference.
The partials have exactly the size gg_gemm_tn_split3_resident_splits answers.  The places to look: the rows behind a slab's last partial stage (the descriptor's range
ends with the slab, row padding included), the columns between K and the operand's pitch, and the stages loaded ahead beyond the slab's end; for the data gradient
the zero rows of dy at the lower and right borders (taps beyond the map load nothing), the rows of a tile behind the last pixel of its class, and the last image's
end.  part has exactly nparts rows, the plane scratch exactly gg_conv3x3s2_dgrad_planes_bytes."""
import os
import re

import pytest
import torch

from tests.test_gpu_guards import BF, F32, rel_l2, rnd, run_guarded

gpu = pytest.mark.gpu
CASES = {"test_resident_weight_gradient": ("gg_gemm_tn_split3_resident",), "test_data_gradient_by_parity": ("gg_conv3x3s2_dgrad_bnbwd_split3",)}
EXEMPT = {
    "gg_gemm_tn_split3_resident_fits": "query: host arithmetic on two integers, no device pointer",
    "gg_gemm_tn_split3_resident_splits": "capacity function: host arithmetic; its ANSWER sizes the partials of the guard case exactly, which is how it is tested",
    "gg_conv3x3s2_dgrad_fits": "query: host arithmetic on four integers, no device pointer",
    "gg_conv3x3s2_dgrad_planes_bytes": "capacity function: host arithmetic; its ANSWER sizes the plane scratch of the guard case exactly, which is how it is tested",
}


def test_every_wgrad_resident_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_wgrad_resident.h and include/gg_conv_dgrad_parity.h is called by the guard case of this file or is in EXEMPT with its reason -- exactly one of the two."""
    from tests.test_guards_cpu import _coverage_gaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = "".join(re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", h)).read(), flags=re.S) for h in ("gg_wgrad_resident.h", "gg_conv_dgrad_parity.h"))
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    guarded = {e for es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing and not unknown and not both, (missing, unknown, both)
    assert len(guarded) + len(EXEMPT) == len(declared) == 6


@gpu
@pytest.mark.parametrize("M,N,K,pad", [(1024 + 37, 96, 432, 8), (64, 96, 432, 0), (33, 8, 260, 24), (300, 64, 288, 4)])
def test_resident_weight_gradient(M, N, K, pad):
    """partials [splits][N][K], reduced by gg_splitk_reduce; rel-L2 < 2e-6 against fp64, gg_gemm_tn_split3's tolerance in tests/test_gpu_guards.py."""
    dY, X = rnd(M, N, seed=61, scale=0.1), rnd(M, K, seed=62)
    ref = dY.double().t() @ X.double()

    def call(S, L):
        lib, st = L.lib(), L.stream()
        splits = lib.gg_gemm_tn_split3_resident_splits(M, N, K)
        assert splits >= 1
        dYi, Xi = S.inp("dY", dY, ld=N + pad, misalign=16), S.inp("X", X, ld=K + pad + 8, col_off=8)
        P = S.out("partials", splits * N, K, F32)
        L.check(lib.gg_gemm_tn_split3_resident(dYi.ptr, dYi.ld, Xi.ptr, Xi.ld, M, N, K, P.ptr, splits, st), "gg_gemm_tn_split3_resident")
        torch.cuda.synchronize()
        Pi = S.inp("partials_in", P.view.cpu())
        o = S.out("dW", 1, N * K, F32)
        L.check(lib.gg_splitk_reduce(Pi.ptr, o.ptr, N * K, splits, 0, L.f32(1.0), st), "gg_splitk_reduce")

        def check(v):
            got = v["dW"].view(N, K)
            assert rel_l2(got, ref) < 2e-6, rel_l2(got, ref)
        return {"partials": P, "dW": o}, check
    run_guarded(call)


@gpu
@pytest.mark.parametrize("B,H,W,nparts", [(2, 4, 4, 8), (2, 6, 10, 3), (2, 10, 6, 8), (3, 2, 2, 16), (1, 24, 24, 5)])
def test_data_gradient_by_parity(B, H, W, nparts):
    """The shapes of tests/test_gpu_patch_embed_bwd.py plus a 24 x 24 map (144 pixels per class: two tiles, the second partial) with fewer workgroups than tiles, and
    more workgroups than tiles (their rows of part are zeros).  dz within 2e-6 rel-L2 of fp64 and the two sums within 1e-5 of their largest magnitude."""
    from tests.test_gpu_patch_embed_bwd import CIN, COUT, _dgrad_case
    c = _dgrad_case(B, H, W)
    M1 = B * H * W

    def call(S, L):
        lib, st = L.lib(), L.stream()
        i = {k: S.inp(k, c[k].reshape(-1, c[k].shape[-1]) if c[k].dim() > 1 else c[k]) for k in ("dy", "y", "wt", "stat", "gamma", "beta")}
        nbytes = lib.gg_conv3x3s2_dgrad_planes_bytes(CIN, COUT)
        assert nbytes == 3 * 9 * CIN * COUT * 2
        planes = S.out("planes", 1, nbytes // 2, BF)
        dz, part = S.out("dz", M1, CIN, F32), S.out("part", nparts, 2 * CIN, F32)
        L.check(lib.gg_conv3x3s2_dgrad_bnbwd_split3(i["dy"].ptr, i["wt"].ptr, COUT, i["y"].ptr, i["stat"].ptr, i["gamma"].ptr, i["beta"].ptr, 1, dz.ptr, part.ptr, nparts,
                                                    planes.ptr, B, H, W, CIN, COUT, st), "gg_conv3x3s2_dgrad_bnbwd_split3")

        def check(v):
            assert rel_l2(v["dz"], c["dz"]) < 2e-6, rel_l2(v["dz"], c["dz"])
            sums = v["part"].double().view(nparts, 2, CIN).sum(0)
            assert float((sums[0] - c["s"]).abs().max()) <= 1e-5 * float(c["s"].abs().max())
            assert float((sums[1] - c["q"]).abs().max()) <= 1e-5 * float(c["q"].abs().max())
        return {"dz": dz, "part": part, "planes": planes}, check
    run_guarded(call)
