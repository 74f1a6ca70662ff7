"""CPU-only checks of the resident weight gradient (include/gg_wgrad_resident.h) and the data gradient by parity (include/gg_conv_dgrad_parity.h): the header against the binding, the slab counts (host arithmetic) and the
refusals, which answer on the host before any launch.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "gg_gemm_tn_split3_resident"


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_wgrad_resident.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.WGRAD_RESIDENT_SYMBOLS) == {WHO, WHO + "_fits", WHO + "_splits"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.WGRAD_RESIDENT_SIGNATURES[n][1]), n
    assert "gg_wgrad_resident.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "gg_wgrad_resident.h" in mk.split("gemm_split3.hip.o ../lib/obj/tinyvit.hip.o:")[1].split("\n")[0]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg.h")).read(), flags=re.S)      # the new symbols live in their own header
    assert not (declared & set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", text)))
    assert not (declared & set(L.SYMBOLS))


def test_data_gradient_header_symbols_match_the_binding(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg_conv_dgrad_parity.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.DGRAD_PARITY_SYMBOLS) == {"gg_conv3x3s2_dgrad_fits", "gg_conv3x3s2_dgrad_planes_bytes", "gg_conv3x3s2_dgrad_bnbwd_split3"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.DGRAD_PARITY_SIGNATURES[n][1]), n
    assert L.DGRAD_PARITY_SIGNATURES["gg_conv3x3s2_dgrad_planes_bytes"][0] is C.c_int64
    assert "gg_conv_dgrad_parity.h" in open(os.path.join(ROOT, "geoguessr-ai_amd", "_lib.py")).read().split("def source_hash")[1]
    mk = open(os.path.join(ROOT, "geoguessr-ai_amd", "csrc", "Makefile")).read()
    assert "gg_conv_dgrad_parity.h" in mk.split("gemm_split3.hip.o ../lib/obj/tinyvit.hip.o:")[1].split("\n")[0]
    assert not (declared & set(L.SYMBOLS))
    # the routing condition's shape part, and the refusal, on the host
    assert lib.gg_conv3x3s2_dgrad_fits(112, 112, 48, 96) == 1 and lib.gg_conv3x3s2_dgrad_fits(112, 112, 32, 64) == 0 and lib.gg_conv3x3s2_dgrad_fits(111, 112, 48, 96) == 0
    assert lib.gg_conv3x3s2_dgrad_planes_bytes(48, 96) == 3 * 9 * 48 * 96 * 2
    buf = C.create_string_buffer(256)
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    assert lib.gg_conv3x3s2_dgrad_bnbwd_split3(p, p, 96, p, p, p, p, 1, p, p, 4, p, 1, 7, 8, 48, 96, None) != 0
    assert b"gg_conv3x3s2_dgrad_bnbwd_split3: needs an even input map" in lib.gg_last_error()
    assert lib.gg_conv3x3s2_dgrad_bnbwd_split3(p, p, 96, p, p, p, p, 1, p, p, 0, p, 1, 8, 8, 48, 96, None) != 0 and b"bad args" in lib.gg_last_error()


def test_slab_counts(L):
    """One slab per CU at the bench step's shape (and at least a quarter more slabs than gg_gemm_tn_f32 takes: the accuracy rule of gg_gemm_tn_split3_splits); slabs of
    whole 32-row stages, never more than 128 MiB of partials."""
    lib = L.lib()
    N, K = 96, 432
    assert lib.gg_gemm_tn_split3_resident_splits(1024 * 56 * 56, N, K) == 256
    for M in (1, 31, 32, 33, 64, 1061, 25088, 50176, 200704, 1024 * 56 * 56):
        for n, k in ((N, K), (64, 288), (8, 8), (96, 448)):
            s = lib.gg_gemm_tn_split3_resident_splits(M, n, k)
            rows = -(-(-(-M // s)) // 32) * 32
            assert s >= 1 and rows * (s - 1) < M, (M, n, k, s)
            assert s * n * k * 4 <= 128 << 20
            need = -(-5 * lib.gg_gemm_tn_f32_splits(M, n, k) // 4)          # a slab's chain is no longer than with a quarter more slabs than gg_gemm_tn_f32 takes,
            assert rows <= -(-(-(-M // need)) // 32) * 32 or (s + 1) * n * k * 4 > 128 << 20, (M, n, k, s)      # in whole stages (or the 128 MiB cap binds)


@pytest.mark.parametrize("N,K", [(100, 432), (96, 452), (128, 128), (0, 8)])
def test_refusals_answer_on_the_host(L, N, K):
    lib = L.lib()
    buf = C.create_string_buffer(256)
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)                 # (16-byte aligned; never dereferenced)
    assert lib.gg_gemm_tn_split3_resident_fits(N, K) == 0
    assert lib.gg_gemm_tn_split3_resident_splits(256, N, K) < 0
    assert lib.gg_gemm_tn_split3_resident(p, max(N, 4), p, max(K, 4), 256, N, K, p, 1, None) != 0
    err = lib.gg_last_error()
    assert WHO.encode() in err and (N <= 0 or b"does not fit one workgroup" in err), err


def test_argument_checks(L):
    lib = L.lib()
    buf = C.create_string_buffer(256)
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)                 # (16-byte aligned; never dereferenced)
    assert lib.gg_gemm_tn_split3_resident(p, 96, p, 430, 256, 96, 430, p, 1, None) != 0 and b"multiples of 4" in lib.gg_last_error()
    assert lib.gg_gemm_tn_split3_resident(p, 92, p, 432, 256, 96, 432, p, 1, None) != 0 and b"ld >= columns" in lib.gg_last_error()
    assert lib.gg_gemm_tn_split3_resident(p, 96, p, 432, 64, 96, 432, p, 3, None) != 0 and b"more splits than 32-row stages" in lib.gg_last_error()
    assert lib.gg_gemm_tn_split3_resident(None, 96, p, 432, 64, 96, 432, p, 1, None) != 0 and b"bad args" in lib.gg_last_error()
