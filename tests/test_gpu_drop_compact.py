"""DropPath row compaction (include/gg_drop.h; the row-compaction fields of GgSplit3Args / GgAttnArgs; csrc/tinyvit.hip block_compacts).

Every kept row goes through the same kernel arithmetic as in the uncompacted schedule and a dropped row contributed exact zeros, so every check here is EQUALITY:
a mapped call against the unmapped call on pre-gathered (or scattered) operands, element for element (`torch.equal`; `+ 0.0` first where a result may be a zero of
either sign), and whatever lies behind the compact extent -- or belongs to a dropped sample -- keeps the fill it had before the call.

Shapes: the smallest that cross the boundaries of the 256 x 128 tile and of a 196-row sample -- 245 rows (under one tile), 1372 rows (five full tiles and a partial
one, samples straddling tiles) -- and kept sets all / none / first and last dropped / alternating."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 777.25            # what untouched output memory must still hold after a call


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return _lib


def kept_sets(B):
    return {"all": list(range(B)), "none": [], "ends_dropped": list(range(1, B - 1)), "alternating": list(range(0, B, 2))}


def make_list(L, kept, B):
    """The device list of one slot through gg_drop_kept_lists itself, from a scale row that keeps `kept`."""
    sc = torch.zeros(1, B, device="cuda")
    if kept:
        sc[0, kept] = 1.25
    lst = torch.full((L.lib().gg_drop_list_ints(B),), -7, dtype=torch.int32, device="cuda")
    L.check(L.lib().gg_drop_kept_lists(sc.data_ptr(), 1, B, lst.data_ptr(), L.stream()), "gg_drop_kept_lists")
    return lst, sc[0].contiguous()


def rows_of(kept, rps):
    return torch.tensor([b * rps + r for b in kept for r in range(rps)], dtype=torch.long, device="cuda")


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


# ------------------------------------------------------------------------------------------- kept lists
@pytest.mark.parametrize("B", [1, 5, 7, 256, 300, 1027])
def test_kept_lists_are_ascending_and_complete(L, B):
    g = torch.Generator().manual_seed(B)
    keep = torch.rand(4, B, generator=g) > 0.3
    keep[1] = True
    keep[2] = False
    scales = (keep.float() * 1.4).cuda().contiguous()
    n = L.lib().gg_drop_list_ints(B)
    assert n >= L.DROP_LIST_HEAD + 2 * B
    lists = torch.full((4, n), -7, dtype=torch.int32, device="cuda")
    L.check(L.lib().gg_drop_kept_lists(scales.data_ptr(), 4, B, lists.data_ptr(), L.stream()), "gg_drop_kept_lists")
    lists = lists.cpu()
    for s in range(4):
        kept = torch.nonzero(keep[s]).flatten().tolist()
        assert int(lists[s, 0]) == len(kept) and int(lists[s, 1]) == B
        assert lists[s, L.DROP_LIST_HEAD:L.DROP_LIST_HEAD + len(kept)].tolist() == kept
        pos = [-1] * B
        for i, b in enumerate(kept):
            pos[b] = i
        assert lists[s, L.DROP_LIST_HEAD + B:L.DROP_LIST_HEAD + 2 * B].tolist() == pos


# ------------------------------------------------------------------------------------------- split GEMM
def _planes(L, W):
    N, K = W.shape
    P = torch.empty((3, N, K), dtype=torch.bfloat16, device="cuda")
    L.check(L.lib().gg_split3_bf16(W.data_ptr(), N, K, K, P.data_ptr(), L.stream()), "gg_split3_bf16")
    return P


def _gemm(L, A, Wp, M, N, K, Cout, *, bias=None, act=0, preact=None, rowscale=None, rps=0, residual=None, dact=None, lst=None, group_rows=0, a_map=False, c_map=False):
    a = L.Split3Args()
    a.b_planes, a.ldb, a.M, a.N, a.K, a.C, a.ldc = Wp.data_ptr(), K, M, N, K, Cout.data_ptr(), N
    if bias is not None: a.bias = bias.data_ptr()
    a.act = act
    if preact is not None: a.preact = preact.data_ptr()
    if rowscale is not None: a.rowscale, a.rows_per_scale = rowscale.data_ptr(), rps
    if residual is not None: a.residual, a.ldr = residual.data_ptr(), N
    if dact is not None: a.dact_preact, a.dact = dact.data_ptr(), 1
    if lst is not None:
        a.groups_dev, a.group_rows = lst.data_ptr(), group_rows
        maps = lst.data_ptr() + 4 * L.DROP_LIST_HEAD
        if a_map: a.a_map = maps
        if c_map: a.c_map = maps
    L.check(L.lib().gg_gemm_nt_split3_af32_stats(C.byref(a), A.data_ptr(), K, 0, None, L.stream()), "gg_gemm_nt_split3_af32_stats")


# epilogue forms of the compacted block: fc1 / qkv data gradient and fc1 forward (compact to compact), fc2 data gradient (A map), proj data gradient (A map, generic epilogue), fc2 / proj forward
# (C / residual map), and both maps at once
FORMS = {"cc_plain": (False, False), "cc_gelu": (False, False), "a_dgelu": (True, False), "a_scale": (True, False), "c_residual": (False, True), "both_residual": (True, True)}


@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("rps,B", [(49, 5), (196, 7)])
def test_split_gemm_row_maps_equal_the_call_on_gathered_rows(L, N, rps, B):
    K, M, GUARD = 384, rps * B, 300                                    # GUARD rows behind every output: never written
    W = rnd(N, K, seed=1, scale=K ** -0.5)
    Wp = _planes(L, W)
    A_phys, bias = rnd(M, K, seed=2), rnd(N, seed=3)
    res_phys, pre_phys = rnd(M, N, seed=4), rnd(M, N, seed=5)
    for kname, kept in kept_sets(B).items():
        lst, scale = make_list(L, kept, B)
        rows, live = rows_of(kept, rps), len(kept) * rps
        for form, (am, cm) in FORMS.items():
            tag = f"N={N} rps={rps} B={B} kept={kname} form={form}"
            # mapped operands: A physical when mapped, else compact (the kept rows first, FILL behind them -- rows the kernel must not read into a result)
            A_in = A_phys if am else torch.cat([A_phys[rows], torch.full((M - live, K), float("nan"), device="cuda")])
            kw, kw_ref = {}, {}
            pre_out = pre_ref = None
            if form == "cc_gelu":
                pre_out = torch.full((M + GUARD, N), FILL, device="cuda")
                pre_ref = torch.full((max(live, 1), N), FILL, device="cuda")
                kw, kw_ref = dict(bias=bias, act=1, preact=pre_out), dict(bias=bias, act=1, preact=pre_ref)
            elif form == "a_dgelu":                                   # saved pre-activation compact; scale per physical sample
                pre_c = torch.cat([pre_phys[rows], torch.full((M - live, N), float("nan"), device="cuda")])
                kw = dict(dact=pre_c, rowscale=scale, rps=rps)
                kw_ref = dict(dact=pre_phys[rows].contiguous(), rowscale=scale[kept].contiguous(), rps=rps)
            elif form == "cc_plain":
                pass
            elif form == "a_scale":
                kw, kw_ref = dict(rowscale=scale, rps=rps), dict(rowscale=scale[kept].contiguous(), rps=rps)
            else:                                                     # residual read and C written through the map
                kw = dict(bias=bias, rowscale=scale, rps=rps, residual=res_phys)
                kw_ref = dict(bias=bias, rowscale=scale[kept].contiguous(), rps=rps, residual=res_phys[rows].contiguous())
            Cm = torch.full((M + GUARD, N), FILL, device="cuda")
            _gemm(L, A_in, Wp, M, N, K, Cm, lst=lst, group_rows=rps, a_map=am, c_map=cm, **kw)
            torch.cuda.synchronize()
            written = rows if cm else torch.arange(live, device="cuda")
            mask = torch.ones(M + GUARD, dtype=torch.bool, device="cuda")
            mask[written] = False
            assert bool((Cm[mask] == FILL).all()), f"{tag}: rows outside the live extent were written"
            if pre_out is not None:
                assert bool((pre_out[live:] == FILL).all()), f"{tag}: pre-activation rows behind the compact extent were written"
            if live == 0:
                continue
            Cr = torch.full((live, N), FILL, device="cuda")
            _gemm(L, A_phys[rows].contiguous(), Wp, live, N, K, Cr, **kw_ref)
            torch.cuda.synchronize()
            assert torch.equal(Cm[written], Cr), f"{tag}: result differs from the unmapped call on gathered rows"
            assert not bool(torch.isnan(Cr).any())
            if pre_out is not None:
                assert torch.equal(pre_out[:live], pre_ref), f"{tag}: saved pre-activation differs"


def test_split_gemm_row_map_refusals(L):
    """What the compacted form does not implement is refused before anything is launched."""
    lib = L.lib()
    W = rnd(128, 384, seed=1); Wp = _planes(L, W)
    A, Cm = rnd(98, 384, seed=2), torch.zeros(98, 128, device="cuda")
    lst, _ = make_list(L, [0], 2)
    a = L.Split3Args()
    a.b_planes, a.ldb, a.M, a.N, a.K, a.C, a.ldc = Wp.data_ptr(), 384, 98, 128, 384, Cm.data_ptr(), 128
    a.a_map = lst.data_ptr() + 16
    assert lib.gg_gemm_nt_split3_af32_stats(C.byref(a), A.data_ptr(), 384, 0, None, L.stream()) != 0 and b"need groups_dev" in lib.gg_last_error()
    a.groups_dev, a.group_rows = lst.data_ptr(), 48
    assert lib.gg_gemm_nt_split3_af32_stats(C.byref(a), A.data_ptr(), 384, 0, None, L.stream()) != 0 and b"divides M" in lib.gg_last_error()
    a.group_rows, a.K = 49, 192                                        # the 128 x 128 form of the short contractions takes no map
    assert lib.gg_gemm_nt_split3_af32_stats(C.byref(a), A.data_ptr(), 384, 0, None, L.stream()) != 0 and b"256 x 128 form only" in lib.gg_last_error()
    torch.cuda.synchronize()
    assert bool((Cm == 0).all())


# ------------------------------------------------------------------------------------------- LayerNorm kernels
LN_M, LN_C, LN_RPS, LN_B = 7 * 196, 384, 196, 7


@pytest.fixture(scope="module")
def ln_case(L):
    """Inputs and the UNMAPPED kernels' results (computed once, shared): norm2's forward over BatchNorm(y), and the statistics its backward reads."""
    Cc, M = LN_C, LN_M
    y = rnd(M, Cc, seed=11)
    bn_stat = torch.cat([rnd(Cc, seed=12, scale=0.3), torch.rand(Cc, generator=torch.Generator().manual_seed(13)).cuda() + 0.5]).contiguous()
    bg, bb_, g, b = rnd(Cc, seed=14) * 0.3 + 1.0, rnd(Cc, seed=15, scale=0.2), rnd(Cc, seed=16) * 0.2 + 1.0, rnd(Cc, seed=17, scale=0.1)
    xout, out, mean, rstd = torch.empty(M, Cc, device="cuda"), torch.empty(M, Cc, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    L.check(L.lib().gg_layernorm_fwd_bn_f32(y.data_ptr(), bn_stat.data_ptr(), bg.data_ptr(), bb_.data_ptr(), xout.data_ptr(), g.data_ptr(), b.data_ptr(), M, Cc,
                                            L.f32(1e-5), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), L.stream()), "gg_layernorm_fwd_bn_f32")
    torch.cuda.synchronize()
    return dict(y=y, bn_stat=bn_stat, bg=bg, bb=bb_, g=g, b=b, xout=xout, out=out, mean=mean, rstd=rstd, dout=rnd(M, Cc, seed=18), dres=rnd(M, Cc, seed=19))


@pytest.mark.parametrize("kname", ["all", "none", "ends_dropped", "alternating"])
def test_layernorm_forward_map(L, ln_case, kname):
    c, M, Cc, rps, B = ln_case, LN_M, LN_C, LN_RPS, LN_B
    kept = kept_sets(B)[kname]
    lst, _ = make_list(L, kept, B)
    rows, live = rows_of(kept, rps), len(kept) * rps
    dropped = rows_of([b for b in range(B) if b not in kept], rps)
    pos = lst.data_ptr() + 4 * (L.DROP_LIST_HEAD + B)
    xout, out, xcopy = (torch.full((M + 64, Cc), FILL, device="cuda") for _ in range(3))
    mean, rstd = torch.full((M + 64,), FILL, device="cuda"), torch.full((M + 64,), FILL, device="cuda")
    L.check(L.lib().gg_layernorm_fwd_bn_f32_map(c["y"].data_ptr(), c["bn_stat"].data_ptr(), c["bg"].data_ptr(), c["bb"].data_ptr(), xout.data_ptr(), c["g"].data_ptr(),
                                                c["b"].data_ptr(), M, Cc, L.f32(1e-5), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), pos, rps, xcopy.data_ptr(),
                                                L.stream()), "gg_layernorm_fwd_bn_f32_map")
    torch.cuda.synchronize()
    assert torch.equal(xout[:M], c["xout"]) and torch.equal(mean[:M], c["mean"]) and torch.equal(rstd[:M], c["rstd"])
    assert torch.equal(out[:live], c["out"][rows]) and bool((out[live:] == FILL).all())                   # compact, nothing behind the compact extent
    assert torch.equal(xcopy[dropped], c["xout"][dropped])                                               # the dropped samples' pass-through
    keep_mask = torch.ones(M + 64, dtype=torch.bool, device="cuda"); keep_mask[dropped] = False
    assert bool((xcopy[keep_mask] == FILL).all())
    assert bool((xout[M:] == FILL).all() and (mean[M:] == FILL).all() and (rstd[M:] == FILL).all())


@pytest.mark.parametrize("colsum", [True, False])
@pytest.mark.parametrize("kname", ["all", "none", "ends_dropped", "alternating"])
def test_layernorm_backward_map(L, ln_case, kname, colsum):
    """gg_layernorm_bwd_colsum (norm2: + the column partials of local_conv's BatchNorm backward) and gg_layernorm_bwd (norm1) against their unmapped calls on a dout
    that holds zeros on the dropped samples' rows -- what the uncompacted branch hands over."""
    c, M, Cc, rps, B = ln_case, LN_M, LN_C, LN_RPS, LN_B
    lib = L.lib()
    kept = kept_sets(B)[kname]
    lst, _ = make_list(L, kept, B)
    rows, live = rows_of(kept, rps), len(kept) * rps
    pos = lst.data_ptr() + 4 * (L.DROP_LIST_HEAD + B)
    dout_full = torch.zeros(M, Cc, device="cuda"); dout_full[rows] = c["dout"][rows]
    dout_c = torch.cat([c["dout"][rows], torch.full((M - live, Cc), float("nan"), device="cuda")]).contiguous()      # NaN behind the compact extent: never read
    nrows = lib.gg_layernorm_bwd_colsum_rows(M)
    pfloats = lib.gg_layernorm_bwd_scratch_floats(M, Cc)
    dx_r, dx_m = torch.full((M + 64, Cc), FILL, device="cuda"), torch.full((M + 64, Cc), FILL, device="cuda")
    part_r, part_m = torch.zeros(pfloats, device="cuda"), torch.zeros(pfloats, device="cuda")
    common = (c["mean"].data_ptr(), c["rstd"].data_ptr(), c["g"].data_ptr(), M, Cc, c["dres"].data_ptr())
    if colsum:
        L.check(lib.gg_layernorm_bwd_colsum(dout_full.data_ptr(), c["xout"].data_ptr(), 1, *common, dx_r.data_ptr(), part_r.data_ptr(), L.stream()), "gg_layernorm_bwd_colsum")
    else:
        L.check(lib.gg_layernorm_bwd(dout_full.data_ptr(), c["xout"].data_ptr(), 1, *common, dx_r.data_ptr(), None, None, None, 0, L.stream()), "gg_layernorm_bwd")
    L.check(lib.gg_layernorm_bwd_map(dout_c.data_ptr(), c["xout"].data_ptr(), *common, dx_m.data_ptr(), part_m.data_ptr() if colsum else None, pos, rps, L.stream()),
            "gg_layernorm_bwd_map")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dx_m).any())
    assert torch.equal(dx_m + 0.0, dx_r + 0.0) and bool((dx_m[M:] == FILL).all())
    dropped = rows_of([b for b in range(B) if b not in kept], rps)
    assert torch.equal(dx_m[dropped], c["dres"][dropped])                                                 # dx = dres on the dropped samples' rows
    if colsum:
        assert torch.equal(part_m[:nrows * 2 * Cc] + 0.0, part_r[:nrows * 2 * Cc] + 0.0) and bool(part_r[:nrows * 2 * Cc].abs().sum() > 0)


# ------------------------------------------------------------------------------------------- attention backward
@pytest.mark.parametrize("kname", ["all", "none", "ends_dropped", "alternating"])
def test_attention_backward_window_map(L, kname):
    """flash_bwd_split_kernel at stage 2's shape (14 x 14 windows, 12 heads of 32, one window per image), B = 5: the mapped call reads the forward's qkv / out / lse
    at the physical window and dout at the compact one; its dqkv (compact) equals the unmapped call's on gathered tensors."""
    lib = L.lib()
    nh, ws, B = 12, 14, 5
    T, Cc = ws * ws, nh * 32
    kept = kept_sets(B)[kname]
    lst, _ = make_list(L, kept, B)
    rows, live = rows_of(kept, T), len(kept) * T
    qkv, dout_phys = rnd(B * T, 3 * Cc, seed=21), rnd(B * T, Cc, seed=22)
    table = rnd(nh, T, seed=23, scale=0.5)
    out, lse = torch.empty(B * T, Cc, device="cuda"), torch.empty(B * T, nh, device="cuda")

    def args(nw, qkv_, out_, lse_):
        a = L.AttnArgs()
        a.qkv, a.ld, a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = qkv_.data_ptr(), 3 * Cc, 0, 32, 64, 96, 32
        a.num_heads, a.num_windows, a.tokens_per_window, a.window_size, a.map_h, a.map_w = nh, nw, T, ws, ws, ws
        a.bias_table, a.scale, a.out, a.ldo, a.lse = table.data_ptr(), 32 ** -0.5, out_.data_ptr(), Cc, lse_.data_ptr()
        return a
    L.check(lib.gg_attention_flash_fwd(C.byref(args(B, qkv, out, lse)), 1, L.stream()), "gg_attention_flash_fwd")
    dout_c = torch.cat([dout_phys[rows], torch.full((B * T - live, Cc), float("nan"), device="cuda")]).contiguous()
    dq_m = torch.full((B * T + 64, 3 * Cc), FILL, device="cuda")
    a = args(B, qkv, out, lse)
    a.dout, a.lddo, a.dqkv = dout_c.data_ptr(), Cc, dq_m.data_ptr()
    a.window_map, a.num_windows_dev = lst.data_ptr() + 4 * L.DROP_LIST_HEAD, lst.data_ptr()
    L.check(lib.gg_attention_flash_bwd(C.byref(a), 1, L.stream()), "gg_attention_flash_bwd (window map)")
    torch.cuda.synchronize()
    assert bool((dq_m[live:] == FILL).all()), "rows behind the compact extent were written"
    if live:
        qg, og, lg, dg = qkv[rows].contiguous(), out[rows].contiguous(), lse[rows].contiguous(), dout_phys[rows].contiguous()
        dq_r = torch.full((live, 3 * Cc), FILL, device="cuda")
        r = args(len(kept), qg, og, lg)
        r.dout, r.lddo, r.dqkv = dg.data_ptr(), Cc, dq_r.data_ptr()
        L.check(lib.gg_attention_flash_bwd(C.byref(r), 1, L.stream()), "gg_attention_flash_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dq_m[:live], dq_r) and not bool(torch.isnan(dq_r).any())
    # a map on a call that has no mapped kernel is refused (here: with a bias gradient)
    dbias = torch.zeros(nh, T, device="cuda")
    a.dbias = dbias.data_ptr()
    assert lib.gg_attention_flash_bwd(C.byref(a), 1, L.stream()) != 0 and b"window_map" in lib.gg_last_error()


# ------------------------------------------------------------------------------------------- whole steps
def test_model_steps_are_bit_identical():
    """tools/drop_compact_check.py in a subprocess under the dev switch that lets the split routes (and so the compaction) be taken at 8 images: three AdamW steps of
    tiny_vit_21m_224 under the reference freeze policy at drop_path_rate 0.5 with compaction on and off from the same state -- loss, embedding, taps, every gradient,
    running statistics equal element for element, the same split launch count, fewer declared split flops -- without and with grad_checkpointing."""
    env = dict(os.environ, GG_DEV_SWITCHES="1", GG_SPLIT_MIN_TILES="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "drop_compact_check.py")], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("-> ok") == 2
