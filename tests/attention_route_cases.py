"""The attention calls behind tests/attention_cases.py::ROUTES as raw GgAttnArgs: what tests/test_attention_route_cpu.py asks gg_attention_route about (numeric
arguments, placeholder pointers, no GPU) and what tests/test_gpu_attention_routes.py and tools/make_attention_routes_parent_golden.py launch and digest on the GPU.
A plain module (no tests, no fixtures).

``route_args`` fills the arguments the way geoguessr_ai_amd.ops does for the route's api: the flash entries get the compact bias table, gg_attention_fwd / _bwd the
expanded table AND the compact one, a backward of a biased route asks for the bias gradient, ``ds_handoff`` routes get a dS region.  The entry points are called
directly, not through ops, so that the golden tool runs on a build that has no route report: it sizes dbias_scratch by the public capacity queries (the largest
of them), which every build answers alike."""
import ctypes as C

import torch

from tests import attention_cases as A

FAKE = 0x10000          # a 16-byte-aligned placeholder: the route report tests pointers for null and alignment only
DTYPE = {"bf16": 0, "f32": 1, "f16": 2}

# Cases of the digest test beyond ROUTES (same fields): the grouped kernels with 65 windows -- the last group of eight holds one window -- and the window_map form
# of the single-pass split backward with 3 of 8 windows live.
EXTRA = [
    A._route("attn_bf16_grouped_65", "attention", "tinyvit", 49, 32, ws=7, map_hw=7, windows=65, storage="bf16", bias=True, kernels=(("FWD_GROUPED", 0), ("BWD_GROUPED", 0))),
    dict(A._route("split_f32_7x7_map", "flash", "tinyvit", 49, 32, ws=7, map_hw=14, windows=8, bias=True, kernels=A._SPLIT(4)), window_map=(5, 0, 6)),
]
DIGEST_CASES = A.ROUTES + EXTRA


def entry_of(r, bwd):
    """(entry name of geoguessr_ai_amd._lib.ATTN_ENTRIES, dtype code) of the route's forward / backward call."""
    if r["api"] == "causal":
        return ("CAUSAL_BWD" if bwd else "CAUSAL_FWD"), r["dtype_code"]
    if r["api"] == "flash":
        return ("FLASH_BWD" if bwd else "FLASH_FWD"), (3 if r["split"] else DTYPE[r["storage"]])
    return ("BWD" if bwd else "FWD_F16" if r["storage"] == "f16" else "FWD"), 0


def route_args(L, r, bwd, *, ptr=None, want_dbias=True):
    """GgAttnArgs of the route's forward / backward.  ``ptr``: {field: device pointer} of a real call; None: placeholders (route report only)."""
    c_kw = A.case(r["layout"], r["N"], r["hd"], r["heads"], r["windows"], r["ws"], r["causal"], r["storage"], "plain", r["map_hw"] if r["layout"] == "tinyvit" else 0)["kw"] \
        if ptr is not None else None
    q_off, k_off, v_off, hs = A.columns(r["layout"], r["heads"], r["hd"])
    a = L.AttnArgs()
    a.ld = 3 * r["heads"] * r["hd"]
    a.q_off, a.k_off, a.v_off, a.head_stride, a.head_dim = q_off, k_off, v_off, hs, r["hd"]
    a.num_heads, a.num_windows, a.tokens_per_window = r["heads"], r["windows"], r["N"]
    a.window_size, a.map_h, a.map_w = r["ws"], (r["map_hw"] if r["ws"] else 0), (r["map_hw"] if r["ws"] else 0)
    a.scale = r["hd"] ** -0.5
    a.ldo = a.lddo = r["heads"] * r["hd"]
    assert c_kw is None or all(getattr(a, k) == v for k, v in c_kw.items()), "route_args and attention_cases.case disagree on the geometry"
    given = ["qkv", "out", "lse"]
    if r["bias"]:
        given += ["bias_table"] + (["bias"] if r["api"] == "attention" else [])
    if bwd:
        given += ["dout", "dqkv"] + (["dbias"] if r["bias"] and want_dbias else []) + (["ds_scratch"] if r["ds_handoff"] else [])
        if r.get("window_map"):
            given += ["window_map", "num_windows_dev"]
            given = [f for f in given if f != "dbias"]          # (the window_map form takes no bias gradient)
    for f in given:
        setattr(a, f, FAKE if ptr is None else ptr[f])
    return a


def reported(L, a, entry, dtype):
    """((kernel name, variant), GgAttnRoute) that gg_attention_route reports for exactly these arguments."""
    rt = L.attention_route(a, entry, dtype)
    return (L.ATTN_KERNELS[rt.kernel], rt.variant), rt


def _call(L, entry, a, dtype):
    lib = L.lib()
    fn = {"FWD": lambda: lib.gg_attention_fwd(C.byref(a), L.stream()), "FWD_F16": lambda: lib.gg_attention_fwd_f16(C.byref(a), L.stream()),
          "BWD": lambda: lib.gg_attention_bwd(C.byref(a), L.stream()), "FLASH_FWD": lambda: lib.gg_attention_flash_fwd(C.byref(a), dtype, L.stream()),
          "FLASH_BWD": lambda: lib.gg_attention_flash_bwd(C.byref(a), dtype, L.stream()), "CAUSAL_FWD": lambda: lib.gg_attention_causal_fwd(C.byref(a), dtype, L.stream()),
          "CAUSAL_BWD": lambda: lib.gg_attention_causal_bwd(C.byref(a), dtype, L.stream())}[entry]
    L.check(fn(), "gg_attention " + entry)


def route_bits(L, r, check_route=None):
    """{"inputs": {tensor: digest}, "out", "lse"[, "dqkv"[, "dbias"]]: digest} of the route's forward and backward on its `plain` case (fixed seed), launched
    through the entry points themselves.  ``check_route(r, bwd, args, entry, dtype)`` is called on the very arguments of each launch, before it, and
    returns their GgAttnRoute.
    dbias is not hashed, although every biased backward here passes a dbias_scratch and the second stage sums its partial rows in fp64 in a fixed order: the
    partial rows themselves are not order-fixed.  Every backward kernel bins dS with LDS float atomics inside a workgroup (dbias_s / the signed-offset table), so two
    runs of ONE build differ in the last bits: two runs of the build in front of the route struct gave different dbias digests on all 15 biased cases and equal
    digests of everything else.  What is order-fixed is asserted instead, bit for bit and on the route's own row count (``check_route`` given): dbias equals the fp64
    sum, in row order, of the scratch rows the second stage finalizes from.  tests/test_gpu_attention_conditioning.py holds dbias of every biased route to fp64."""
    c = A.case(r["layout"], r["N"], r["hd"], r["heads"], r["windows"], r["ws"], r["causal"], r["storage"], "plain", r["map_hw"] if r["layout"] == "tinyvit" else 0)
    lib = L.lib()
    F32 = torch.float32
    H, D, ws, W = r["heads"], r["hd"], r["ws"], r["windows"]
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    t = dict(qkv=qkv, dout=dout, out=torch.zeros(qkv.shape[0], H * D, dtype=qkv.dtype, device="cuda"), lse=torch.zeros(qkv.shape[0], H, dtype=F32, device="cuda"),
             dqkv=torch.zeros_like(qkv))
    inputs = dict(qkv=A._sha(qkv), dout=A._sha(dout))
    if r["bias"]:
        t["bias_table"] = c["table"].cuda()
        inputs["table"] = A._sha(t["bias_table"])
        t["dbias"] = torch.zeros_like(t["bias_table"])
        rows = max(lib.gg_attention_flash_dbias_rows(W, r["N"]), W + 64)
        t["dbias_scratch"] = torch.empty(rows * H * ws * ws, dtype=F32, device="cuda")
        if r["api"] == "attention":
            Np = lib.gg_attention_padded_tokens(r["N"])
            t["bias"] = torch.empty(H, Np, Np, dtype=torch.bfloat16, device="cuda")
            L.check(lib.gg_attention_expand_bias(t["bias_table"].data_ptr(), H, ws, C.c_float(D ** -0.5), t["bias"].data_ptr(), L.stream()), "gg_attention_expand_bias")
    if r["ds_handoff"]:
        t["ds_scratch"] = torch.empty(lib.gg_attention_flash_ds_scratch_floats(W, H, r["N"]), dtype=F32, device="cuda")
    if r.get("window_map"):
        live = list(r["window_map"])
        t["window_map"] = torch.tensor(live + [0] * (W - len(live)), dtype=torch.int32, device="cuda")
        t["num_windows_dev"] = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
        inputs["window_map"] = A._sha(t["window_map"].float())
    ptr = {k: v.data_ptr() for k, v in t.items()}
    res = dict(inputs=inputs)
    for bwd in ((False, True) if r["bwd"] else (False,)):
        entry, dtype = entry_of(r, bwd)
        a = route_args(L, r, bwd, ptr=ptr)
        if bwd and a.dbias:
            a.dbias_scratch = ptr["dbias_scratch"]
        rt = check_route(r, bwd, a, entry, dtype) if check_route is not None else None
        _call(L, entry, a, dtype)
        torch.cuda.synchronize()
        if rt is not None and a.dbias:
            # the part of dbias that IS order-fixed, bit for bit: the second stage's fp64 sum, in row order, of the rows it finalizes from -- the partial rows
            # themselves up to 64 of them, else the rows gg_reduce_rows folded them into, which lie behind them in the scratch -- rounded to f32 once
            n, Wd = rt.dbias_rows - 64, H * ws * ws
            rows = t["dbias_scratch"].view(-1, Wd)
            rows = rows[:n] if n <= 64 else rows[n:n + -(-n // -(-n // 64))]
            acc = torch.zeros(Wd, dtype=torch.float64, device="cuda")
            for row in rows:
                acc += row.double()
            assert torch.equal(acc.float(), t["dbias"].view(-1)), f"{r['name']}: dbias is not the fixed-order fp64 sum of its {len(rows)} scratch rows"
        if not bwd:
            res["out"], res["lse"] = A._sha(t["out"]), A._sha(t["lse"])
        else:
            res["dqkv"] = A._sha(t["dqkv"])          # (dbias is requested, through a dbias_scratch, and not hashed: see route_bits' docstring)
    return res


def dump_routes(L):
    """{case name: [(kernel name, variant) of the forward, of the backward]} of DIGEST_CASES under the switches of this process; "refused" where the entry refuses."""
    out = {}
    for r in DIGEST_CASES:
        out[r["name"]] = []
        for bwd in ((False, True) if r["bwd"] else (False,)):
            try:
                out[r["name"]].append(list(reported(L, route_args(L, r, bwd), *entry_of(r, bwd))[0]))
            except L.GgError:
                out[r["name"]].append("refused")
    return out
