"""CPU self-test of tests/guards.py: a stray write into each region of a guarded tensor is detected and NAMED, a NaN left in a logical output is
detected, a clean call passes, and the band rule (256 rows of the leading dimension, at least 64 KiB) holds."""
import pytest
import torch

from tests import guards as G


def _set(fill):
    s = G.GuardSet(fill, device="cpu")
    x = s.inp("x", torch.arange(5 * 24, dtype=torch.float32).reshape(5, 24), ld=32)
    w = s.inp("w", torch.ones(3, 8, dtype=torch.bfloat16), ld=40, col_off=16, misalign=16)
    y = s.out("y", 5, 24, torch.float32, ld=37)
    return s, x, w, y


def _clean_call(x, y):
    y.view.copy_(x.view * 2)


@pytest.mark.parametrize("fill", ["nan", "finite"])
def test_clean_call_passes(fill):
    s, x, w, y = _set(fill)
    _clean_call(x, y)
    s.check()
    assert torch.equal(y.view, x.view * 2)


@pytest.mark.parametrize("fill", ["nan", "finite"])
@pytest.mark.parametrize("who,region,byte", [
    ("y", "output front band", -1), ("y", "output back band", 5 * 37 * 4), ("y", "output row padding", 24 * 4), ("y", "output row padding", 4 * 37 * 4 + 36 * 4),
    ("x", "input payload", 0), ("x", "input payload", 4 * 32 * 4 + 23 * 4 + 3), ("x", "input front band", -65536), ("x", "input back band", 5 * 32 * 4 + 60000),
    ("x", "input row padding", 24 * 4), ("w", "input row padding", 0), ("w", "input row padding", 24 * 2), ("w", "input payload", 16 * 2)])
def test_one_stray_byte_is_detected_and_named(fill, who, region, byte):
    s, x, w, y = _set(fill)
    _clean_call(x, y)
    g = {"x": x, "w": w, "y": y}[who]
    g.buf[g.front + byte] ^= 0x10                        # one byte, relative to the payload start
    with pytest.raises(G.GuardViolation) as e:
        s.check()
    msg = str(e.value)
    assert f"{who}: {region} changed (1 bytes, first at byte {byte:+d}" in msg, msg
    assert msg.count("changed") == 1 and f"[{fill} fill]" in msg


def test_unwritten_logical_output_is_detected():
    s, x, w, y = _set("finite")
    _clean_call(x, y)
    y.view[3, 23] = float("nan")
    with pytest.raises(G.GuardViolation, match=r"y: output payload has 1 NaN logical elements.*first at \[3, 23\]"):
        s.check()
    s, x, w, y = _set("finite")                          # nothing written at all: the NaN pre-fill of the logical elements is still there
    with pytest.raises(G.GuardViolation, match="y: output payload has 120 NaN"):
        s.check()


def test_layout_rules():
    s, x, w, y = _set("nan")
    assert x.front == x.back == 65536 and x.ptr == x.buf.data_ptr() + 65536
    assert w.front == 65536 + 16 and w.ptr == w.buf.data_ptr() + w.front + 16 * 2 and w.view.stride(0) == 40
    big = s.inp("big", torch.zeros(2, 100, dtype=torch.float32), ld=1000)
    assert big.back == 256 * 1000 * 4                    # 256 rows of the leading dimension once that exceeds 64 KiB
    assert torch.isnan(y.view).all() and (y.buf[:y.front] == 0xFF).all()
    f = G.GuardSet("finite", device="cpu")
    o = f.out("o", 2, 3, torch.float32, ld=8)
    assert torch.isnan(o.view).all()                     # logical outputs start as NaN under either fill
    assert float(o.buf[o.front:].view(torch.float32)[3]) == pytest.approx(51015.28, rel=1e-6)
    i = f.out("i", 1, 4, torch.int64)
    assert (i.view == -1).all() and int(i.buf[:8].view(torch.int64)[0]) == 0x4747474747474747
    acc = f.out("acc", 1, 4, torch.float32, init=torch.zeros(4))
    assert (acc.view == 0).all()
    sc = f.scratch("sc", 1000)
    assert sc.payload_bytes == 1000 and sc.back >= 65536
    o.view.fill_(1.0)
    sc.view.fill_(3)                                     # scratch contents are free
    f.check()
    sc.buf[sc.front + 1000] = 0
    with pytest.raises(G.GuardViolation, match="sc: scratch back band changed"):
        f.check()


def test_fill_dependence_is_reported():
    a, b = torch.ones(4), torch.ones(4)
    G.assert_bit_identical(a, b, "same")
    b[2] = 1 + 2 ** -23
    with pytest.raises(G.GuardViolation, match="differs between the NaN fill and the finite fill"):
        G.assert_bit_identical(a, b, "y")


def test_guard_registry_names_entry_points_of_the_header():
    """The registry of tests/test_gpu_guards.py (CASES: which entry points each guard test calls) and of tests/test_gpu_guards_model.py holds only names the header
    declares, every registered case is a test function of the module, and no entry point is named by a case that does not exist.  (Completeness against the header:
    test_every_entry_point_is_guarded_or_exempt.)"""
    import os
    import re
    from tests import test_gpu_guards as K, test_gpu_guards_model as M
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert len(K.CASES) >= 30
    for name, (fn, entries) in K.CASES.items():
        assert name.startswith("test_") and getattr(K, name) is fn and entries, name
        assert set(entries) <= declared, (name, set(entries) - declared)
        src = open(K.__file__).read()
        body = src[src.index(f"def {name}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        helpers = src if any(h in body for h in ("_nt_case(",)) else body
        for e in entries:                                   # the case really calls what it registers
            assert re.search(r"\b" + e + r"\b", helpers), (name, e)
    assert set(M.MODEL_ENTRIES) <= declared
    guarded = {e for _, es in K.CASES.values() for e in es} | set(M.MODEL_ENTRIES)
    assert len(guarded) >= 80, len(guarded)


# Entry points that take no device tensor (or none of the caller's), with the reason each is outside the guard suites.
_QUERY = "query: host arithmetic on shapes / configuration, no device pointer"
_CAP = "capacity function: host arithmetic; its ANSWER sizes the scratch of a guard case exactly, which is how it is tested"
EXEMPT = {
    "gg_version": "version call", "gg_last_error": "error call: host string",
    **{n: _QUERY for n in ("gg_attention_padded_tokens", "gg_attention_flash_single_pass", "gg_clip_num_tensors", "gg_clip_tensor_info", "gg_clip_param_floats",
                           "gg_clip_first_trained_layer", "gg_tinyvit_num_tensors", "gg_tinyvit_tensor_info", "gg_tinyvit_param_floats", "gg_tinyvit_buffer_floats",
                           "gg_tinyvit_num_counters", "gg_tinyvit_num_drop_slots", "gg_tinyvit_activation_info", "gg_tinyvit_activation_info_masked")},
    "gg_gemm_nt_route": "route report: host arithmetic on a GgGemmArgs whose pointers are only tested for alignment, never dereferenced (tests/test_gemm16_cases_cpu.py)",
    "gg_gemm_nt_split3_route": "route report: host arithmetic on a GgSplit3Args whose pointers are only tested for null and alignment, never dereferenced (tests/test_split3_cases_cpu.py)",
    "gg_attention_route": "route report: host arithmetic on a GgAttnArgs whose pointers are only tested for null and alignment, never dereferenced (tests/test_attention_route_cpu.py)",
    **{n: _CAP for n in ("gg_gemm_colstats_rows", "gg_stat_rows_capacity", "gg_gemm_tn_splits", "gg_gemm_tn_f32_splits", "gg_gemm_tn_split3_splits", "gg_colsum_scratch_floats",
                         "gg_bn_bwd_rows", "gg_bn_bwd_scratch_floats", "gg_layernorm_bwd_scratch_floats", "gg_layernorm_bwd_colsum_rows", "gg_attention_flash_dbias_rows",
                         "gg_attention_flash_ds_scratch_floats", "gg_dwconv_stat_rows", "gg_dwconv_fused_stat_rows", "gg_dwconv_fwd_fused_stat_rows",
                         "gg_dwconv_s2_fused_stat_rows", "gg_dwconv_wgrad_scratch_floats", "gg_dwconv_f32_stat_rows", "gg_dwconv_f32_s2_fused_stat_rows",
                         "gg_dwconv_f32_wgrad_scratch_floats", "gg_preprocess_pil_workspace_bytes", "gg_tinyvit_wcache_bytes", "gg_tinyvit_workspace_bytes",
                         "gg_tinyvit_workspace_bytes_masked", "gg_clip_wcache_bytes", "gg_clip_workspace_bytes")},
    **{n: "gg_prof_*: host-side launch log, no caller tensor" for n in ("gg_prof_enable", "gg_prof_reset", "gg_prof_read", "gg_prof_count", "gg_prof_record")},
    **{n: "gg_graph_*: graph-cache control, no caller tensor (replay itself is covered by the whole-step tests)" for n in ("gg_graph_set_mode", "gg_graph_stats", "gg_graph_clear")},
    **{n: "gg_comm_*: RCCL collectives over a communicator; needs several ranks (tests/test_gpu_distributed.py)" for n in
       ("gg_comm_unique_id", "gg_comm_create", "gg_comm_destroy", "gg_comm_rank", "gg_comm_world", "gg_comm_allreduce_sum_f32", "gg_comm_broadcast", "gg_comm_barrier")},
}


@pytest.mark.parametrize("Cc", [1032, 12])
def test_bf16_depthwise_channel_contract_is_refused_before_the_device(Cc):
    """include/gg.h: the bf16 depthwise family takes C % 8 == 0, C <= 1024 and nothing else.  Every entry point refuses the first multiple of 8 above the bound and
    a C that is no multiple of 8 with gg_last_error() naming C, and every row / scratch count answers negative -- on a machine without a GPU and with pointers
    that are never dereferenced, so the check comes before anything touches the device.  The counts still answer at both ends of the contract."""
    import ctypes as C
    from geoguessr_ai_amd import _lib as L
    lib = L.lib()
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    B, H, W = 1, 6, 6
    entries = {
        "gg_dwconv3x3_fwd": lambda s: lib.gg_dwconv3x3_fwd(p, p, p, B, H, W, Cc, s, p, None),
        "gg_dwconv3x3_fwd_fused": lambda s: lib.gg_dwconv3x3_fwd_fused(p, p, p, p, 1, p, p, B, H, W, Cc, s, p, None),
        "gg_dwconv3x3_bwd_data": lambda s: lib.gg_dwconv3x3_bwd_data(p, p, p, B, H, W, Cc, s, None),
        "gg_dwconv3x3_bwd_data_fused": lambda s: lib.gg_dwconv3x3_bwd_data_fused(p, p, p, p, p, B, H, W, Cc, p, p, p, p, 1, p, None),
        "gg_dwconv3x3_s2_bwd_data_fused": lambda s: lib.gg_dwconv3x3_s2_bwd_data_fused(p, p, p, p, p, B, H, W, Cc, p, p, p, p, 1, p, None),
        "gg_dwconv3x3_bwd_weight": lambda s: lib.gg_dwconv3x3_bwd_weight(p, p, B, H, W, Cc, s, p, p, 0, None),
    }
    counts = {
        "gg_dwconv_stat_rows": lambda c, s: lib.gg_dwconv_stat_rows(B, H, W, c, s),
        "gg_dwconv_fwd_fused_stat_rows": lambda c, s: lib.gg_dwconv_fwd_fused_stat_rows(B, H, W, c, s),
        "gg_dwconv_fused_stat_rows": lambda c, s: lib.gg_dwconv_fused_stat_rows(B, H, W, c, 1),
        "gg_dwconv_s2_fused_stat_rows": lambda c, s: lib.gg_dwconv_s2_fused_stat_rows(B, H, W, c),
        "gg_dwconv_wgrad_scratch_floats": lambda c, s: lib.gg_dwconv_wgrad_scratch_floats(B, H, W, c, s),
    }
    for stride in (1, 2):
        for name, call in entries.items():
            assert call(stride) != 0, (name, stride)
            err = lib.gg_last_error()
            assert name.encode() in err and f"C = {Cc}".encode() in err, (name, stride, err)
        for name, call in counts.items():
            assert call(Cc, stride) < 0, (name, stride)
            assert f"C = {Cc}".encode() in lib.gg_last_error(), (name, stride)
            assert call(8, stride) > 0 and call(1024, stride) > 0, (name, stride)


def _declared():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = "".join(re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", h)).read(), flags=re.S) for h in ("gg.h", "gg_attn_route.h"))      # (the route report's header rides along: its one prototype is exempt by name)
    return set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))


def _coverage_gaps(declared, guarded, exempt):
    """(entry points in neither table, names in a table that the header does not declare, names in both tables)."""
    return sorted(declared - guarded - set(exempt)), sorted((guarded | set(exempt)) - declared), sorted(guarded & set(exempt))


def test_every_entry_point_is_guarded_or_exempt():
    """Every gg_* prototype of include/gg.h is either called by a guard case (the registry: CASES of tests/test_gpu_guards.py, MODEL_ENTRIES of
    tests/test_gpu_guards_model.py) or in EXEMPT with its reason -- exactly one of the two.  A new entry point without a guard test fails here by name, and so does one
    dropped from the registry."""
    from tests import test_gpu_guards as K, test_gpu_guards_model as M
    declared = _declared()
    guarded = {e for _, es in K.CASES.values() for e in es} | set(M.MODEL_ENTRIES)
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing, f"entry points of include/gg.h with neither a guard test nor an exemption: {missing}"
    assert not unknown, f"registry / exemption names the header does not declare: {unknown}"
    assert not both, f"both guarded and exempt: {both}"
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())
    # only the kinds of entry point that take none of the caller's tensors may be exempt
    ok = ("_rows", "_floats", "_splits", "_bytes", "_capacity", "_info", "_num_", "gg_prof_", "gg_graph_", "gg_comm_", "gg_version", "gg_last_error", "_padded_tokens",
          "_single_pass", "_first_trained_layer", "_workspace_bytes_masked", "_info_masked", "_nt_route", "gg_attention_route", "_split3_route")
    assert all(any(k in n for k in ok) for n in EXEMPT), [n for n in EXEMPT if not any(k in n for k in ok)]
    # the detector itself: taking any one entry point out of the registry is reported by name
    for victim in ("gg_gemm_nt", "gg_proto_refine", "gg_tinyvit_backward", "gg_dwconv3x3_s2_bwd_data_fused_f32"):
        assert _coverage_gaps(declared, guarded - {victim}, EXEMPT)[0] == [victim]
    assert _coverage_gaps(declared | {"gg_new_kernel"}, guarded, EXEMPT)[0] == ["gg_new_kernel"]
