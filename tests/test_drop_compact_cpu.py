"""CPU-only checks of the DropPath row compaction's boundary (include/gg_drop.h and the row-compaction fields of GgSplit3Args / GgAttnArgs): the header, the
binding and the struct layouts agree, the workspace plan keeps its size, and bad arguments are refused without a device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_drop_header_symbols_match_the_binding(L):
    hdr = open(os.path.join(ROOT, "include", "gg_drop.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.DROP_SYMBOLS) == {"gg_drop_list_ints", "gg_drop_kept_lists", "gg_layernorm_fwd_bn_f32_map", "gg_layernorm_bwd_map", "gg_tinyvit_set_drop_compact"}
    lib = L.lib()
    for n in declared:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert len(m.group(1).split(",")) == len(L.DROP_SIGNATURES[n][1]), n
    assert int(re.search(r"#define GG_DROP_LIST_HEAD (\d+)", hdr).group(1)) == L.DROP_LIST_HEAD


def test_row_compaction_fields_sit_where_the_header_puts_them(L):
    """offsetof of the new fields (and sizeof) from the host compiler against the ctypes mirrors."""
    fields = {"GgSplit3Args": (L.Split3Args, ["groups_dev", "group_rows", "a_map", "c_map"]), "GgAttnArgs": (L.AttnArgs, ["window_map", "num_windows_dev"])}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gg.h"\n#include "gg_drop.h"\nint main(){'
    want = []
    for cname, (mirror, names) in fields.items():
        src += f'printf("%zu ", sizeof({cname}));' + "".join(f'printf("%zu ", offsetof({cname}, {f}));' for f in names)
        want += [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in names]
    src += "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == want


def test_list_size_switch_and_refusals_without_a_device(L):
    lib = L.lib()
    for B in (1, 5, 8, 1024, 1027):
        n = lib.gg_drop_list_ints(B)
        assert n >= L.DROP_LIST_HEAD + 2 * B and n % 4 == 0
    assert lib.gg_drop_list_ints(0) < 0
    assert lib.gg_tinyvit_set_drop_compact(0) == 1 and lib.gg_tinyvit_set_drop_compact(1) == 0 and lib.gg_tinyvit_set_drop_compact(1) == 1      # default on; returns the previous value
    assert lib.gg_drop_kept_lists(None, 1, 4, None, None) != 0 and b"gg_drop_kept_lists" in lib.gg_last_error()
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) & ~15                                   # 16-byte aligned host memory: only the argument checks run
    assert lib.gg_layernorm_bwd_map(p, p, p, p, p, 10, 8, p, p, None, p, 4, None) != 0 and b"whole samples" in lib.gg_last_error()
    assert lib.gg_layernorm_fwd_bn_f32_map(p, p, p, p, p, p, p, 8, 8, L.f32(1e-5), p, p, p, None, 4, None, None) != 0 and b"bad args" in lib.gg_last_error()
    a = L.AttnArgs()
    a.qkv, a.head_dim, a.num_heads, a.num_windows, a.tokens_per_window, a.ld = p, 32, 1, 1, 16, 96
    a.window_map = p                                                   # without its device-side count
    assert lib.gg_attention_flash_bwd(C.byref(a), 1, None) != 0 and b"go together" in lib.gg_last_error()
    a.num_windows_dev = p
    assert lib.gg_attention_flash_fwd(C.byref(a), 1, None) != 0 and b"gg_attention_flash_bwd only" in lib.gg_last_error()


def test_workspace_plan_is_unchanged(L):
    """The kept lists of a compacted block live in scratch.colsum (idle in a frozen block): the fp32_split plan keeps the fp32 plan's size and the switch does not move it."""
    from geoguessr_ai_amd.models.tinyvit import TinyViTAdapter
    lib = L.lib()
    sizes = {}
    for prec in ("fp32", "fp32_split"):
        m = TinyViTAdapter("tiny_vit_21m_224", pretrained=False, precision=prec)
        m.freeze_all_but_last_stage()
        bb = m.backbone
        mask = bb.trainable_mask()
        sizes[prec] = [lib.gg_tinyvit_workspace_bytes_masked(C.byref(bb.cfg), B, 1, mask) for B in (8, 1024)]
        if prec == "fp32_split":
            lib.gg_tinyvit_set_drop_compact(0)
            assert [lib.gg_tinyvit_workspace_bytes_masked(C.byref(bb.cfg), B, 1, mask) for B in (8, 1024)] == sizes[prec]
            lib.gg_tinyvit_set_drop_compact(1)
            off, nb = C.c_int64(), C.c_int64()
            for B in (8, 1024):      # room for a block's two lists
                assert lib.gg_tinyvit_activation_info_masked(C.byref(bb.cfg), B, b"scratch.colsum", mask, C.byref(off), C.byref(nb)) == 0
                assert nb.value >= 2 * 4 * lib.gg_drop_list_ints(B)
    assert sizes["fp32"] == sizes["fp32_split"]
