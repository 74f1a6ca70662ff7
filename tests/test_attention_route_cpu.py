"""CPU checks of gg_attention_route (include/gg_attn_route.h; host arithmetic, no GPU): the report is the struct the attention launchers execute, so it is held here
to the dispatch of the commit in front of it -- restated below as literals (ROUTES' recorded kernels, the edge table) and as ``parent_route``, the if-chains of that
commit's gg_attention_fwd / _fwd_f16 / _bwd, gg_attention_flash_fwd / _bwd and the causal entries written out in Python with their development switches --, the
public capacity queries to that commit's closed forms, and the workspace plans to that commit's totals (tests/golden/attention_plan_bytes_parent.json)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests import attention_cases as A
from tests import attention_route_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = 1024


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _align(x, n):
    return -(-x // n) * n


# ------------------------------------------------------------------------------------------- the parent's dispatch, restated
def parent_route(entry, dtype, *, N, D, ws=0, windows=2, dbias=False, ds=False, bias=False, bias_table=False, sw=()):
    """(kernel name, variant, block of the first pass) the parent commit's launchers chose.  sw: names of the GG_ATTN_* switches that are set (GG_ATTN_SMALL=0 as
    "GG_ATTN_SMALL")."""
    npad, strips = _align(N, 16), _align(N, 16) // 16
    nbpad = _align(max(4, (2 * ws - 1) ** 2), 4)
    if entry in ("FWD", "FWD_F16", "BWD"):
        bwd = entry == "BWD"
        beyond = N > 256 or ws > 16                                                             # attn_use_flash
        split_bwd = bwd and "GG_ATTN_NO_SPLIT" not in sw and D == 32 and ws > 0 and (N + 15) // 16 in (13, 9) and (not bias or bias_table)      # attn_use_split_bwd
        if beyond or split_bwd:
            return parent_route("FLASH_BWD" if bwd else "FLASH_FWD", 2 if entry == "FWD_F16" else 0, N=N, D=D, ws=ws, windows=windows, dbias=dbias, ds=ds, sw=sw)
        nkt = 4 if N <= 64 else 10 if N <= 160 else 14 if N <= 224 else 16
        if entry != "FWD_F16" and D == 32 and nkt == 4 and "GG_ATTN_SMALL" not in sw and windows >= 64:
            return ("BWD_GROUPED" if bwd else "FWD_GROUPED"), 0, 256
        return ("BWD" if bwd else "FWD"), nkt, 256
    lds_dkv = lambda Rr, db: (2 * Rr * (D + 4) + nbpad * (2 if db else 1) + 3 * Rr) * 4
    lds_fused = lambda db: (3 * npad * (D + 4) + nbpad * (2 if db else 1) + 3 * npad + 2 * strips * 320) * 4
    split_strips = D == 32 and "GG_ATTN_NO_SPLIT" not in sw and strips in (4, 9, 13)
    if entry in ("CAUSAL_FWD", "CAUSAL_BWD"):
        if dtype != 0:
            return ("FLASH64_BWD_SPLIT" if entry == "CAUSAL_BWD" else "FLASH64_FWD_SPLIT"), 0, 256
        return ("FLASH_FWD_STREAM", 0, 256) if entry == "CAUSAL_FWD" else ("FLASH_BWD_FUSED", 0, 64 * strips)
    if dtype == 3:
        return ("FLASH64_BWD_SPLIT" if entry == "FLASH_BWD" else "FLASH64_FWD_SPLIT"), 0, 256
    if entry == "FLASH_FWD":
        if dtype == 1 and split_strips:
            return "FLASH_FWD_SPLIT", strips, 64 * strips
        res = "GG_ATTN_FLASH_NO_RES" not in sw and lds_dkv(npad, False) <= 64 * KB                 # flash_fwd_resident
        tail = res and "GG_ATTN_FWD_NO_TAIL" not in sw and 4 < strips <= 17 and strips % 4 == 1  # flash_fwd_tail
        return ("FLASH_FWD_RESIDENT" if res else "FLASH_FWD_STREAM"), int(tail), (64 * (strips - 1 if tail else min(16, strips)) if res else 256)
    assert entry == "FLASH_BWD"
    if split_strips:
        npl, np_ = (3 if dtype == 1 else 1), (strips + 1) // 2
        assert 2 * npl * 32 * np_ * 64 + (32 * np_ * 36 + nbpad * (2 if dbias else 1) + 3 * 32 * np_ + np_ * 320) * 4 <= 160 * KB      # sp_lds_bwd: holds for every such shape
        return "FLASH_BWD_SPLIT", strips, 64 * np_
    if "GG_ATTN_NO_FUSED_BWD" not in sw and npad <= 256 and lds_fused(dbias) <= 160 * KB:        # flash_fused_ok
        waves = strips - 1 if ("GG_ATTN_FUSED_NO_TAIL" not in sw and strips > 4 and strips % 4 == 1 and strips - 1 >= 2 * (D // 16)) else strips
        return "FLASH_BWD_FUSED", (13 if strips == 13 else 4 if strips == 4 else 0), 64 * waves
    return ("FLASH_BWD_STREAM_DS" if ds else "FLASH_BWD_STREAM"), 0, 256


def parent_of_route(r, bwd, sw=()):
    entry, dtype = R.entry_of(r, bwd)
    has_dbias = bwd and r["bias"] and not r.get("window_map")
    return parent_route(entry, dtype, N=r["N"], D=r["hd"], ws=r["ws"], windows=r["windows"], dbias=has_dbias, ds=bwd and r["ds_handoff"], bias=r["bias"],
                        bias_table=r["bias"], sw=sw)[:2]


def args(L, N, D, *, ws=0, windows=2, heads=2, map_hw=None, bwd=False, given=()):
    """Numeric GgAttnArgs with 16-byte-aligned placeholder pointers: qkv, out, lse (and dout, dqkv for ``bwd``) plus the fields named in ``given``."""
    a = L.AttnArgs()
    a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = 3 * heads * D, 0, heads * D, 2 * heads * D, D, D
    a.num_heads, a.num_windows, a.tokens_per_window, a.window_size = heads, windows, N, ws
    a.map_h = a.map_w = (map_hw or ws) if ws else 0
    a.scale, a.ldo, a.lddo = D ** -0.5, heads * D, heads * D
    for f in ("qkv", "out", "lse") + (("dout", "dqkv") if bwd else ()) + tuple(given):
        setattr(a, f, R.FAKE)
    return a


def ask(L, a, entry, dtype=0):
    rt = L.attention_route(a, entry, dtype)
    return L.ATTN_KERNELS[rt.kernel], rt.variant, rt.pass_[0].block


def refusal(L, a, entry, dtype=0):
    rt = L.AttnRoute()
    assert L.lib().gg_attention_route(C.byref(a), L.ATTN_ENTRY[entry], dtype, C.byref(rt)) == -1
    return L.lib().gg_last_error().decode()


# ------------------------------------------------------------------------------------------- 1. ROUTES reaches what it says
def test_routes_report_their_recorded_kernels(L):
    reached = set()
    for r in R.DIGEST_CASES:
        for bwd in ((False, True) if r["bwd"] else (False,)):
            entry, dtype = R.entry_of(r, bwd)
            a = R.route_args(L, r, bwd)
            got, rt = R.reported(L, a, entry, dtype)
            assert got == r["kernels"][int(bwd)] == parent_of_route(r, bwd), (r["name"], "bwd" if bwd else "fwd", got, r["kernels"][int(bwd)], parent_of_route(r, bwd))
            assert rt.passes == (2 if got[0] in ("FLASH_BWD_STREAM", "FLASH_BWD_STREAM_DS", "FLASH64_BWD_SPLIT") else 1)
            assert rt.reads_ds_scratch == int(got[0] == "FLASH_BWD_STREAM_DS")
            assert rt.rounded_bias == int(bwd and r["api"] == "attention" and r["bias"] and got[0].startswith("FLASH"))
            assert (rt.dbias_rows > 0) == bool(a.dbias)
            if r in A.ROUTES:
                reached.add(got[0])
    # every kernel but the four of the flash16 entries (checked below: each entry has one route): the table as a whole reaches all that need no development switch
    assert reached == set(L.ATTN_KERNELS) - {"NONE", "FLASH16_FWD", "FLASH16_WIN_FWD", "FLASH16_BWD", "FLASH16_WIN_BWD"}


def test_flash16_entries_report_their_one_route(L):
    lin = lambda bwd: args(L, 300, 64, bwd=bwd)
    win = lambda bwd, given=(): args(L, 576, 32, ws=24, bwd=bwd, given=given)
    assert ask(L, lin(False), "FLASH16_FWD", 0) == ask(L, lin(False), "FLASH16_FWD", 2) == ("FLASH16_FWD", 0, 256)
    assert ask(L, lin(True), "FLASH16_BWD", 0) == ("FLASH16_BWD", 0, 256)
    assert ask(L, win(False), "FLASH16_WIN_FWD") == ("FLASH16_WIN_FWD", 0, 256) and ask(L, win(False, ("bias_table",)), "FLASH16_WIN_FWD") == ("FLASH16_WIN_FWD", 1, 256)
    for given, variant in (((), 0), (("bias_table",), 1), (("bias_table", "dbias"), 2)):
        rt = L.attention_route(win(True, given), "FLASH16_WIN_BWD", 0)
        assert (L.ATTN_KERNELS[rt.kernel], rt.variant, rt.passes) == ("FLASH16_WIN_BWD", variant, 2)
        assert rt.pass_[0].grid == rt.pass_[1].grid == 2 * 2 * 5          # (window, head, 128-key block)
        assert rt.dbias_rows == (2 * 5 + 64 if variant == 2 else 0) and rt.dbias_rows <= L.lib().gg_attention_flash16_win_dbias_rows(2, 576)
    assert "head_dim must be 32 (got 64" in refusal(L, lin(True), "FLASH16_WIN_BWD")
    assert "fp16 storage is inference-only" in refusal(L, lin(True), "FLASH16_BWD", 2)
    assert "window_map / num_windows_dev are a form of gg_attention_flash_bwd only" in refusal(L, args(L, 300, 64, given=("window_map", "num_windows_dev")), "FLASH16_FWD")
    assert "unknown entry 99" in (L.lib().gg_attention_route(C.byref(lin(False)), 99, 0, C.byref(L.AttnRoute())) == -1 and L.lib().gg_last_error().decode())


# ------------------------------------------------------------------------------------------- 2. edges of every threshold
def test_threshold_edges(L):
    S, RES, FUSED = "FLASH_FWD_STREAM", "FLASH_FWD_RESIDENT", "FLASH_BWD_FUSED"
    table = []          # (what, entry, dtype, args kw, expected (kernel, variant, block))
    # key tiles of the register-resident kernels, and the hand-over to the online-softmax kernels beyond 256 tokens
    for N, nkt in ((64, 4), (65, 10), (160, 10), (161, 14), (224, 14), (225, 16), (256, 16)):
        table.append(("nkt", "FWD", 0, dict(N=N, D=64), ("FWD", nkt, 256)))
        table.append(("nkt", "FWD_F16", 0, dict(N=N, D=64), ("FWD", nkt, 256)))
        table.append(("nkt", "BWD", 0, dict(N=N, D=32, bwd=True), ("BWD", nkt, 256)))
    table += [("beyond", "FWD", 0, dict(N=257, D=64), (S, 0, 256)), ("beyond", "FWD_F16", 0, dict(N=257, D=64), (S, 0, 256)),
              ("beyond", "BWD", 0, dict(N=257, D=32, bwd=True), ("FLASH_BWD_STREAM", 0, 256))]
    # the grouped kernels from 64 windows on
    for W, grouped in ((63, False), (64, True), (65, True)):
        table.append(("grouped", "FWD", 0, dict(N=49, D=32, ws=7, windows=W), ("FWD_GROUPED", 0, 256) if grouped else ("FWD", 4, 256)))
        table.append(("grouped", "BWD", 0, dict(N=49, D=32, ws=7, windows=W, bwd=True), ("BWD_GROUPED", 0, 256) if grouped else ("BWD", 4, 256)))
    table.append(("grouped", "FWD", 0, dict(N=49, D=64, ws=7, windows=64), ("FWD", 4, 256)))          # head dim 32 only
    # the split kernels: 4 / 9 / 13 strips at head dim 32
    for strips in (4, 9, 13):
        table.append(("split", "FLASH_FWD", 1, dict(N=16 * strips, D=32), ("FLASH_FWD_SPLIT", strips, 64 * strips)))
        table.append(("split", "FLASH_FWD", 0, dict(N=16 * strips, D=32), (RES, int(strips != 4), 64 * (strips - 1 if strips != 4 else 4))))      # bf16 forward: never split
        for dt in (1, 0):
            table.append(("split", "FLASH_BWD", dt, dict(N=16 * strips, D=32, bwd=True), ("FLASH_BWD_SPLIT", strips, 64 * ((strips + 1) // 2))))
        table.append(("split", "FLASH_BWD", 1, dict(N=16 * strips, D=64, bwd=True), (FUSED, 4, 256) if strips == 4 else (FUSED, 0, 512) if strips == 9 else ("FLASH_BWD_STREAM", 0, 256)))
    for strips, fwd, bwd_block in ((5, (RES, 1, 256), 256), (10, (RES, 0, 640), 640), (12, (RES, 0, 768), 768)):
        table.append(("split", "FLASH_FWD", 1, dict(N=16 * strips, D=32), fwd))
        for dt in (1, 0):
            table.append(("split", "FLASH_BWD", dt, dict(N=16 * strips, D=32, bwd=True), (FUSED, 0, bwd_block)))
    # the forward's cooperative tail (strips = 4 n + 1 of a resident window) and the single-pass backward's owner waves (one fewer where strips - 1 >= 2 (D / 16))
    for strips, exp in ((4, (RES, 0, 256)), (5, (RES, 1, 256)), (8, (RES, 0, 512)), (9, (RES, 1, 512)), (13, (RES, 1, 768)), (16, (S, 0, 256)), (17, (S, 0, 256))):
        table.append(("tail", "FLASH_FWD", 0, dict(N=16 * strips, D=32), exp))
    for strips, exp in ((4, (RES, 0, 256)), (5, (RES, 1, 256)), (8, (S, 0, 256)), (9, (S, 0, 256))):
        table.append(("tail", "FLASH_FWD", 1, dict(N=16 * strips, D=64), exp))
    for strips, D, exp in ((4, 64, (FUSED, 4, 256)), (5, 64, (FUSED, 0, 320)), (8, 64, (FUSED, 0, 512)), (9, 64, (FUSED, 0, 512)), (5, 32, (FUSED, 0, 256)), (8, 32, (FUSED, 0, 512)),
                           (16, 32, (FUSED, 0, 1024)), (17, 32, ("FLASH_BWD_STREAM", 0, 256)), (13, 64, ("FLASH_BWD_STREAM", 0, 256)), (17, 64, ("FLASH_BWD_STREAM", 0, 256))):
        table.append(("waves", "FLASH_BWD", 1, dict(N=16 * strips, D=D, bwd=True), exp))
    # the single-pass LDS bound: head dim 64 between 160 and 176 padded tokens, head dim 32 between 256 and 272; with a bias gradient on the nearest windows
    table += [("lds", "FLASH_BWD", 1, dict(N=160, D=64, bwd=True), (FUSED, 0, 640)), ("lds", "FLASH_BWD", 1, dict(N=161, D=64, bwd=True), ("FLASH_BWD_STREAM", 0, 256)),
              ("lds", "FLASH_BWD", 1, dict(N=256, D=32, bwd=True), (FUSED, 0, 1024)), ("lds", "FLASH_BWD", 1, dict(N=257, D=32, bwd=True), ("FLASH_BWD_STREAM", 0, 256)),
              ("lds", "FLASH_BWD", 1, dict(N=144, D=64, ws=12, bwd=True, given=("bias_table", "dbias")), (FUSED, 0, 512)),
              ("lds", "FLASH_BWD", 1, dict(N=169, D=64, ws=13, bwd=True, given=("bias_table", "dbias")), ("FLASH_BWD_STREAM", 0, 256)),
              ("lds", "FLASH_BWD", 1, dict(N=256, D=32, ws=16, bwd=True, given=("bias_table", "dbias")), (FUSED, 0, 1024)),
              ("lds", "FLASH_BWD", 1, dict(N=289, D=32, ws=17, bwd=True, given=("bias_table", "dbias")), ("FLASH_BWD_STREAM", 0, 256)),
              ("lds", "FLASH_BWD", 1, dict(N=289, D=32, ws=17, bwd=True, given=("bias_table", "dbias", "ds_scratch")), ("FLASH_BWD_STREAM_DS", 0, 256))]
    # the largest resident forward and the next padded length up
    table += [("resident", "FLASH_FWD", 0, dict(N=208, D=32), (RES, 1, 768)), ("resident", "FLASH_FWD", 0, dict(N=209, D=32), (S, 0, 256)),
              ("resident", "FLASH_FWD", 1, dict(N=112, D=64), (RES, 0, 448)), ("resident", "FLASH_FWD", 1, dict(N=113, D=64), (S, 0, 256))]
    # window sides: 16 / 17 between the two sources, 32 the last the bias table holds
    table += [("ws", "FWD", 0, dict(N=256, D=32, ws=16, given=("bias", "bias_table")), ("FWD", 16, 256)), ("ws", "FWD", 0, dict(N=289, D=32, ws=17, given=("bias_table",)), (S, 0, 256)),
              ("ws", "BWD", 0, dict(N=256, D=32, ws=16, bwd=True, given=("bias", "bias_table", "dbias")), ("BWD", 16, 256)),
              ("ws", "BWD", 0, dict(N=289, D=32, ws=17, bwd=True, given=("bias_table", "dbias")), ("FLASH_BWD_STREAM", 0, 256)),
              ("ws", "FLASH_FWD", 1, dict(N=1024, D=32, ws=32, given=("bias_table",)), (S, 0, 256))]
    for what, entry, dtype, kw, exp in table:
        a = args(L, **kw)
        got = ask(L, a, entry, dtype)
        given = kw.get("given", ())
        model = parent_route(entry, dtype, N=kw["N"], D=kw["D"], ws=kw.get("ws", 0), windows=kw.get("windows", 2), dbias="dbias" in given, ds="ds_scratch" in given,
                             bias="bias" in given, bias_table="bias_table" in given)
        assert got == exp == model, (what, entry, dtype, kw, got, exp, model)
    # a sweep: the report against the restated dispatch at every length
    for N in list(range(1, 300)) + [576, 577, 1024]:
        for D in (32, 64):
            for entry, dtype in (("FWD", 0), ("FWD_F16", 0), ("BWD", 0), ("FLASH_FWD", 0), ("FLASH_FWD", 1), ("FLASH_FWD", 2), ("FLASH_BWD", 0), ("FLASH_BWD", 1)) + \
                    ((("FLASH_FWD", 3), ("FLASH_BWD", 3)) if D == 64 else ()) + ((("CAUSAL_FWD", 0), ("CAUSAL_BWD", 0), ("CAUSAL_FWD", 1), ("CAUSAL_BWD", 3)) if D == 64 and N <= 77 else ()):
                if entry == "BWD" and D == 64 and N <= 256:
                    continue          # (refused: only head dim 32 is built)
                bwd = entry.endswith("BWD")
                assert ask(L, args(L, N, D, bwd=bwd), entry, dtype) == parent_route(entry, dtype, N=N, D=D), (N, D, entry, dtype)
    # grids, LDS bytes and the rows of the second stage on a few routes
    rt = L.attention_route(args(L, 49, 32, ws=7, windows=65, bwd=True, given=("bias", "bias_table", "dbias")), "BWD")
    assert (rt.pass_[0].grid, rt.pass_[0].lds, rt.dbias_rows) == (9 * 2, 0, 9 + 64)
    rt = L.attention_route(args(L, 49, 32, ws=7, windows=63, bwd=True, given=("bias", "bias_table", "dbias")), "BWD")
    assert (rt.pass_[0].grid, rt.dbias_rows) == (63 * 2, 63 + 64)
    rt = L.attention_route(args(L, 576, 32, ws=24, windows=3, bwd=True, given=("bias_table", "dbias")), "FLASH_BWD", 1)
    assert (rt.passes, rt.pass_[0].grid, rt.pass_[1].grid, rt.dbias_rows) == (2, 3 * 2 * 9, 3 * 2 * 9, 3 * 9 + 64)
    assert rt.pass_[0].lds == (2 * 64 * 36 + 2212 + 64) * 4 and rt.pass_[1].lds == (2 * 64 * 36 + 2 * 2212 + 3 * 64) * 4
    rt = L.attention_route(args(L, 196, 32, ws=14, windows=3, bwd=True, given=("bias", "bias_table", "dbias")), "BWD")          # leaves attention.hip, bias rounded as its forward's
    assert (L.ATTN_KERNELS[rt.kernel], rt.variant, rt.rounded_bias, rt.dbias_rows, rt.pass_[0].grid, rt.pass_[0].block) == ("FLASH_BWD_SPLIT", 13, 1, 3 + 64, 6, 448)
    rt = L.attention_route(args(L, 196, 32, ws=14, windows=3, bwd=True, given=("bias_table", "dbias")), "FLASH_BWD", 0)
    assert (L.ATTN_KERNELS[rt.kernel], rt.rounded_bias) == ("FLASH_BWD_SPLIT", 0)


def test_refusals_carry_the_launchers_texts(L):
    # window_map: accepted on its one route (f32 storage, head dim 32, the split kernel, no bias gradient), refused by name everywhere else
    wm = ("window_map", "num_windows_dev")
    assert ask(L, args(L, 49, 32, ws=7, map_hw=14, windows=8, bwd=True, given=wm + ("bias_table",)), "FLASH_BWD", 1) == ("FLASH_BWD_SPLIT", 4, 128)
    assert refusal(L, args(L, 49, 32, ws=7, map_hw=14, windows=8, bwd=True, given=wm + ("bias_table", "dbias")), "FLASH_BWD", 1) == \
        "gg_attention_flash_bwd: window_map is f32 storage without a bias gradient"
    assert refusal(L, args(L, 49, 32, ws=7, map_hw=14, windows=8, bwd=True, given=wm), "FLASH_BWD", 0) == "gg_attention_flash_bwd: window_map is f32 storage without a bias gradient"
    assert refusal(L, args(L, 100, 32, ws=10, bwd=True, given=wm), "FLASH_BWD", 1) == \
        "gg_attention_flash_bwd: window_map needs the single-pass split kernel (f32 storage, head dim 32, 7 x 7 / 12 x 12 / 14 x 14 windows)"
    assert refusal(L, args(L, 49, 64, ws=7, bwd=True, given=wm), "FLASH_BWD", 1).startswith("gg_attention_flash_bwd: window_map needs the single-pass split kernel")
    assert refusal(L, args(L, 49, 32, ws=7, given=wm), "FLASH_FWD", 1) == "gg_attention_flash_fwd: window_map is a form of gg_attention_flash_bwd only"
    assert refusal(L, args(L, 49, 32, ws=7, bwd=True, given=("window_map",)), "FLASH_BWD", 1) == "gg_attention_flash_bwd: window_map and num_windows_dev go together"
    assert refusal(L, args(L, 49, 64, given=wm), "CAUSAL_FWD", 1) == "gg_attention_causal_fwd: window_map is a form of gg_attention_flash_bwd only"
    # the bias and its gradient
    assert refusal(L, args(L, 576, 32, ws=24, bwd=True, given=("dbias",)), "FLASH_BWD", 1) == "gg_attention_flash_bwd: dbias without bias_table"
    assert refusal(L, args(L, 576, 32, bwd=True, given=("bias_table",)), "FLASH_BWD", 1) == "gg_attention_flash_bwd: the relative-position bias needs a window geometry"
    assert refusal(L, args(L, 289, 32, ws=17, given=("bias",)), "FWD") == "gg_attention_fwd: this window shape takes the bias as bias_table (compact f32)"
    assert refusal(L, args(L, 289, 32, ws=17, bwd=True, given=("bias",)), "BWD") == "gg_attention_bwd: this window shape takes the bias as bias_table (compact f32)"
    assert refusal(L, args(L, 50, 64, given=("bias_table",)), "FWD_F16") == "gg_attention_fwd_f16: the fp16 forward takes no bias"
    assert refusal(L, args(L, 49, 32, given=("bias",)), "FWD") == "gg_attention_fwd: bias needs a window geometry"
    # dtypes
    assert refusal(L, args(L, 300, 64, bwd=True), "FLASH_BWD", 2) == "gg_attention_flash_bwd: fp16 storage is inference-only"
    assert refusal(L, args(L, 300, 32), "FLASH_FWD", 3) == "gg_attention_flash_fwd: dtype 3 (split-bf16 products) is head dim 64 without windows or bias (got head_dim 32, window_size 0)"
    assert refusal(L, args(L, 50, 64), "CAUSAL_FWD", 2) == "gg_attention_causal_fwd: dtype must be 0 (bf16), 1 (f32) or 3 (f32, split products); got 2"
    assert refusal(L, args(L, 78, 64, bwd=True), "CAUSAL_BWD", 0) == "gg_attention_causal_bwd: 78 tokens exceed the position table (77)"
    # geometry, pointers, alignment
    assert refusal(L, args(L, 1089, 32, ws=33), "FLASH_FWD", 1) == "gg_attention_flash_fwd: window_size > 32 unsupported (bias table of at most 1024 entries)"
    assert refusal(L, args(L, 50, 32, ws=7), "FLASH_FWD", 1) == "gg_attention_flash_fwd: window_size^2 != tokens_per_window"
    assert refusal(L, args(L, 49, 32, ws=7, map_hw=15), "FWD") == "gg_attention_fwd: map not divisible by window"
    assert refusal(L, args(L, 49, 32, ws=7, map_hw=14, windows=6), "FWD") == "gg_attention_fwd: window count"
    assert refusal(L, args(L, 64, 64, bwd=True), "BWD") == "gg_attention_bwd: only head_dim 32 (TinyViT) is built"
    a = args(L, 64, 32, bwd=True); a.lse = None
    assert refusal(L, a, "BWD") == "gg_attention_bwd: needs the forward's lse and out"
    a = args(L, 300, 64); a.qkv = R.FAKE + 8
    assert refusal(L, a, "FLASH_FWD", 1) == "gg_attention_flash_fwd: qkv must be 16-byte aligned"
    a = args(L, 300, 64); a.out = None
    assert refusal(L, a, "FLASH_FWD", 0) == "gg_attention_flash_fwd: bad out"
    rt = L.AttnRoute()
    assert L.lib().gg_attention_route(None, L.ATTN_ENTRY["FLASH_BWD"], 1, C.byref(rt)) == -1 and L.lib().gg_last_error() == b"gg_attention_flash_bwd: null qkv"
    assert L.lib().gg_attention_route(None, L.ATTN_ENTRY["FWD"], 0, C.byref(rt)) == -1 and L.lib().gg_last_error() == b"gg_attention_fwd: null qkv"


# ------------------------------------------------------------------------------------------- 3. development switches
def _dump(env):
    code = "import json; from geoguessr_ai_amd import _lib as L; from tests import attention_route_cases as R; print(json.dumps(R.dump_routes(L)))"
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _attention_groups():
    from tests.test_gpu_switches import GROUPS
    return {g: {k: v for k, v in sw.items() if k.startswith("GG_ATTN_")} for g, sw in GROUPS.items() if any(k.startswith("GG_ATTN_") for k in sw)}


@pytest.mark.parametrize("group", sorted(_attention_groups()))
def test_development_switches_move_the_report(group):
    """One subprocess per group (the library reads a switch once per process): under GG_DEV_SWITCHES the report moves every ROUTES case to the fallback the
    restated dispatch names for the group's switches; without the gate the same variables change nothing."""
    switches = _attention_groups()[group]
    base = {k: v for k, v in os.environ.items() if not k.startswith("GG_") or k == "GG_LIB"}
    sw = tuple(k for k, v in switches.items() if k != "GG_ATTN_SMALL" or v == "0")
    moved = 0
    for gate in (True, False):
        got = _dump(dict(base, **switches, **({"GG_DEV_SWITCHES": "1"} if gate else {})))
        for r in R.DIGEST_CASES:
            # (with the one route that takes a window map switched off, that call is refused: in the launcher and in the report alike)
            want = ["refused" if gate and r.get("window_map") and b and "GG_ATTN_NO_SPLIT" in sw else list(parent_of_route(r, b, sw if gate else ()))
                    for b in ((False, True) if r["bwd"] else (False,))]
            assert got[r["name"]] == want, (group, gate, r["name"], got[r["name"]], want)
            moved += gate and want != [list(k) for k in r["kernels"]]
    assert moved > 0, "the group's switches move no ROUTES case"


def test_switch_group_with_a_refused_route_is_refused_in_the_report():
    base = {k: v for k, v in os.environ.items() if not k.startswith("GG_") or k == "GG_LIB"}
    code = "import ctypes as C; from geoguessr_ai_amd import _lib as L; from tests import attention_route_cases as R; r = R.EXTRA[1]; " \
           "print(L.lib().gg_attention_route(C.byref(R.route_args(L, r, True)), L.ATTN_ENTRY['FLASH_BWD'], 1, C.byref(L.AttnRoute())), L.lib().gg_last_error().decode())"
    out = subprocess.run([sys.executable, "-c", code], env=dict(base, GG_DEV_SWITCHES="1", GG_ATTN_NO_SPLIT="1"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("-1 gg_attention_flash_bwd: window_map needs the single-pass split kernel"), (out.stdout, out.stderr[-1000:])


# ------------------------------------------------------------------------------------------- 4. the public queries
def test_capacity_queries_keep_their_closed_forms(L):
    lib = L.lib()
    for N in range(1, 1101, 7):
        npad = _align(N, 16)
        for W in (1, 2, 63, 64, 65, 130):
            assert lib.gg_attention_flash_dbias_rows(W, N) == W * ((N + 63) // 64) + 64
            assert lib.gg_attention_flash16_win_dbias_rows(W, N) == W * ((N + 127) // 128) + 64
        for ws in (0, 7, 12, 14, 16, 17, 24, 32):
            nbpad = _align(max(4, (2 * ws - 1) ** 2), 4)
            for D in (32, 64, 48):
                for db in (0, 1):
                    fused = (3 * npad * (D + 4) + nbpad * (2 if db else 1) + 3 * npad + 2 * (npad // 16) * 320) * 4
                    assert lib.gg_attention_flash_single_pass(N, D, ws, db) == int(D in (32, 64) and npad <= 256 and fused <= 160 * KB), (N, D, ws, db)
    for W in range(1, 131):
        assert lib.gg_attention_flash_dbias_rows(W, 576) == W * 9 + 64 and lib.gg_attention_flash16_win_dbias_rows(W, 576) == W * 5 + 64
    # no route needs more rows than the public query of its family promises
    for r in R.DIGEST_CASES + WORKLOAD_SHAPES:
        if not (r["bwd"] and r["bias"]) or r.get("window_map"):
            continue
        entry, dtype = R.entry_of(r, True)
        rows = L.attention_route(R.route_args(L, r, True), entry, dtype).dbias_rows
        assert 0 < rows <= lib.gg_attention_flash_dbias_rows(r["windows"], r["N"]), r["name"]
        if r["api"] == "attention" and r["N"] <= 256:
            assert rows <= r["windows"] + 64, r["name"]          # (what ops.attention allocated before it asked the route)


# the window attentions of the model classes at batch 8: tiny_vit_21m at 224 / 384 / 512 (7 / 12 / 16 / 24 / 32 windows per stage and the 14 x 14 of stage 2), bf16 and f32
WORKLOAD_SHAPES = [A._route(f"tinyvit_{st}_{ws}x{ws}_{side}", api, "tinyvit", ws * ws, 32, ws=ws, map_hw=side, windows=8 * (side // ws) ** 2, storage=st, bias=True,
                            kernels=(("NONE", 0), ("NONE", 0)))
                   for st, api in (("bf16", "attention"), ("f32", "flash")) for ws, side in ((7, 56), (7, 28), (14, 14), (7, 7), (12, 48), (12, 24), (24, 24), (12, 12), (16, 64), (16, 32), (32, 32), (16, 16))]


# ------------------------------------------------------------------------------------------- 5. plans to the byte
def test_workspace_plans_unchanged_from_the_parent_build():
    """Every workspace total of tests/golden/make_golden_attention_plan_bytes.py (TinyViT at every size its variants accept, the CLIP towers, the text tower) equals
    what the build in front of the route struct planned: the planners now ask gg_attention_route whether a dS region is read, and answer as before."""
    from tests.golden.make_golden_attention_plan_bytes import plan_bytes
    with open(os.path.join(ROOT, "tests", "golden", "attention_plan_bytes_parent.json")) as f:
        gold = json.load(f)
    got = plan_bytes()
    assert sorted(got) == sorted(gold) and len(got) > 300
    bad = {k: (got[k], gold[k]) for k in got if got[k] != gold[k]}
    assert not bad, bad
