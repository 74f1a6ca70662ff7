"""CLIP tower at any input size, the parts that need no GPU: the fp64 reference of tests/clip_interp_cases.py against torch and against transformers' own run
(tests/golden/clip_interp_tiny.npz), and the host side of the plan through libgg.so -- token counts, byte counts, the zero tail, every refusal by name."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import clip_interp_cases as IC


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.mark.parametrize("geom", IC.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_reference_matches_torch_interpolate_in_fp64(geom):
    Gs, Gh, Gw = geom
    pos = IC.table(Gs, 8, seed=sum(geom)).astype(np.float64)
    want = IC.torch_interp(torch.from_numpy(pos), Gh, Gw).numpy()
    got = IC.interp_ref(pos, Gh, Gw)
    err = float(np.abs(got - want).max())
    print(f"\n[{geom}] separable fp64 form vs torch fp64: max abs {err:.2e}")
    assert got.shape == (Gh * Gw + 1, 8) and err < 1e-12
    # the transposed form is the adjoint: <W x, y> == <x, W^T y>
    y = np.random.default_rng(1).standard_normal(got.shape)
    a, b = float((got * y).sum()), float((pos * IC.interp_ref_bwd(y, Gs, Gh, Gw)).sum())
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a))
    if Gs == Gh == Gw:
        assert np.array_equal(got, pos)


def test_reference_reproduces_the_transformers_fixture(golden_dir):
    """The fp64 oracle forward on the separable-form table against transformers' fp32 ``last_hidden_state`` mean, and its position gradient, at the fp32 class of
    tests/test_gpu_clip.py (rel-L2 1e-4): the restatement the GPU tests are held to IS the library's semantics."""
    g = np.load(os.path.join(golden_dir, "clip_interp_tiny.npz"))
    assert tuple(int(v) for v in g["cfg"]) == IC.TINY and int(g["weight_seed"]) == IC.WEIGHT_SEED
    st = IC.tiny_weights()
    assert abs(sum(float(v.double().sum()) for v in st.values()) - float(g["w_checksum"])) < 1e-6, "rng stream changed"
    ps = IC.TINY[5]
    for H, W in g["sizes"]:
        H, W = int(H), int(W)
        key = f"{H}x{W}"
        x = IC.tiny_input(H, W)
        assert abs(float(x.double().sum()) - float(g["x_checksum." + key])) < 1e-6, "rng stream changed"
        assert g["last_hidden_state." + key].shape == (2, (H // ps) * (W // ps) + 1, IC.TINY[0])
        np.testing.assert_allclose(g["last_hidden_state." + key].mean(1), g["pooled." + key], rtol=0, atol=1e-6)
        # the matrix form feeds the oracle in place of F.interpolate
        from oracle import clip_ref as R
        st64 = {k: v.double() for k, v in st.items()}
        pos = st64["embeddings.position_embedding.weight"].clone().requires_grad_(True)
        Wh, Ww = torch.from_numpy(IC.cubic_matrix(4, H // ps)), torch.from_numpy(IC.cubic_matrix(4, W // ps))
        grid = torch.einsum("ys,sxd,wx->ywd", Wh, pos[1:].reshape(4, 4, -1), Ww).reshape((H // ps) * (W // ps), -1)
        st64["embeddings.position_embedding.weight"] = torch.cat([pos[:1], grid], 0)
        pooled = R.forward(IC.tiny_spec(), st64, x.double())
        pooled.square().sum().backward()
        rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
        e_p, e_g = rel(pooled.detach().numpy(), g["pooled." + key].astype(np.float64)), rel(pos.grad.numpy(), g["g_pos." + key].astype(np.float64))
        print(f"\n[{key}] fp64 oracle on the matrix-form table vs transformers fp32: pooled rel-L2 {e_p:.2e}, position gradient rel-L2 {e_g:.2e}")
        assert e_p < 1e-4 and e_g < 1e-4
        np.testing.assert_allclose(IC.oracle_forward(st, x).numpy(), pooled.detach().numpy(), rtol=0, atol=1e-12)


def _cfg(L, act=1, image=32, patch=8, h=0, w=0, hidden=128, heads=2, recompute=0):
    c = L.ClipCfg()
    c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads, c.image_size, c.patch_size = hidden, 256, 2, heads, image, patch
    c.ln_eps, c.act_dtype, c.recompute, c.input_h, c.input_w = 1e-5, act, recompute, h, w
    return c


def test_plan_honours_the_call_size(L):
    lib = L.lib()
    al = lambda n: (n + 255) // 256 * 256
    for act in (0, 1, 2, 3, 8):
        native = _cfg(L, act)
        floats, wc0 = lib.gg_clip_param_floats(C.byref(native)), lib.gg_clip_wcache_bytes(C.byref(native))
        ws0 = {(tr, B): lib.gg_clip_workspace_bytes(C.byref(native), B, tr, None) for tr in (0, 1) for B in (1, 3)}
        assert floats > 0 and wc0 > 0 and all(v > 0 for v in ws0.values())
        # the size named explicitly, and any size with the native GRID, is the native plan: a zero tail changes nothing
        same = _cfg(L, act, h=32, w=32)
        assert lib.gg_clip_wcache_bytes(C.byref(same)) == wc0 and lib.gg_clip_param_floats(C.byref(same)) == floats
        assert all(lib.gg_clip_workspace_bytes(C.byref(same), B, tr, None) == v for (tr, B), v in ws0.items())
        prev = None
        for H, W in ((24, 24), (40, 56), (48, 48), (128, 128), (128, 136)):
            c = _cfg(L, act, h=H, w=W)
            T = (H // 8) * (W // 8) + 1
            # image_size still shapes the parameter table; the resampled f32 table (T x D) is the one region the cache gains
            assert lib.gg_clip_param_floats(C.byref(c)) == floats and lib.gg_clip_num_tensors(C.byref(c)) == lib.gg_clip_num_tensors(C.byref(native))
            assert lib.gg_clip_wcache_bytes(C.byref(c)) - wc0 == al(T * 128 * 4), (act, H, W)
            ws = lib.gg_clip_workspace_bytes(C.byref(c), 3, 0, None)
            assert ws > 0 and (prev is None or ws > prev), (act, H, W)      # the workspace grows with the size
            assert (ws < ws0[(0, 3)]) == (T < 17)
            prev = ws
            if act in (0, 1, 3):
                assert lib.gg_clip_workspace_bytes(C.byref(c), 3, 1, None) > ws
    # the position table keeps image_size's shape
    c = _cfg(L, 1, h=40, w=56)
    name, off, numel, ndim, shape = C.create_string_buffer(256), C.c_int64(), C.c_int64(), C.c_int(), (C.c_int64 * 4)()
    for i in range(lib.gg_clip_num_tensors(C.byref(c))):
        assert lib.gg_clip_tensor_info(C.byref(c), i, name, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape) == 0
        if name.value == b"embeddings.position_embedding.weight":
            assert (shape[0], shape[1]) == (17, 128)
    # recompute and a trainable mask plan at a foreign size too
    assert 0 < lib.gg_clip_workspace_bytes(C.byref(_cfg(L, 0, h=128, w=128, recompute=1)), 2, 1, None) < lib.gg_clip_workspace_bytes(C.byref(_cfg(L, 0, h=128, w=128)), 2, 1, None)


def test_plan_refusals_by_name(L):
    lib = L.lib()
    err = lambda: lib.gg_last_error().decode()
    for entry in (lambda c: lib.gg_clip_wcache_bytes(C.byref(c)), lambda c: lib.gg_clip_workspace_bytes(C.byref(c), 2, 0, None),
                  lambda c: lib.gg_clip_workspace_bytes(C.byref(c), 2, 1, None), lambda c: lib.gg_clip_num_tensors(C.byref(c)),
                  lambda c: lib.gg_clip_param_floats(C.byref(c)), lambda c: lib.gg_clip_refresh_weights(C.byref(c), 0x10000, 0x10000, None),
                  lambda c: lib.gg_clip_forward(C.byref(c), 1, 0, 0x10000, 0x10000, 0x10000, 0x10000, 0x10000, None, None, None),
                  lambda c: lib.gg_clip_backward(C.byref(c), 1, 0x10000, 0x10000, 0x10000, 0x10000, None, 0x10000, None, None)):
        assert entry(_cfg(L, h=44, w=48)) < 0 and "44 x 48 is not a multiple of the patch size 8" in err()
        assert entry(_cfg(L, h=48, w=44)) < 0 and "48 x 44 is not a multiple of the patch size 8" in err()
        assert entry(_cfg(L, h=-8, w=48)) < 0 and "input_h / input_w" in err()
        assert entry(_cfg(L, h=8 * 65, w=48)) < 0 and "above the cap of 64" in err()       # the call's grid
        assert entry(_cfg(L, image=8 * 65, h=48, w=48)) < 0 and "above the cap of 64" in err()      # the table's grid, once it has to be resampled
    assert lib.gg_clip_wcache_bytes(C.byref(_cfg(L, image=8 * 65))) > 0      # ... a native call of such a tower is today's plan
    assert lib.gg_clip_wcache_bytes(C.byref(_cfg(L, h=8 * 64, w=8))) > 0     # 64 x 1: the cap itself, and a one-patch side


def test_kernel_entry_points_refuse_by_name(L):
    lib = L.lib()
    assert set(L.CLIP_INTERP_SYMBOLS) == {"gg_clip_pos_interp_fwd", "gg_clip_pos_interp_bwd"} and L.CLIP_INTERP_MAX_SIDE == 64
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gg_clip_interp.h")).read()
    assert "#define GG_CLIP_INTERP_MAX_SIDE 64" in hdr
    p = 0x10000
    for fn, who in ((lib.gg_clip_pos_interp_fwd, "gg_clip_pos_interp_fwd"), (lib.gg_clip_pos_interp_bwd, "gg_clip_pos_interp_bwd")):
        for args, text in (((None, 4, 5, 7, 64, p), "null pointer"), ((p, 4, 5, 7, 64, None), "null pointer"), ((p, 4, 5, 7, 66, p), "multiple of 4"),
                           ((p, 4, 5, 7, 0, p), "multiple of 4"), ((p, 0, 5, 7, 64, p), "below 1"), ((p, 4, 0, 7, 64, p), "below 1"),
                           ((p, 4, 5, -1, 64, p), "below 1"), ((p, 65, 5, 7, 64, p), "above the cap of 64"), ((p, 4, 65, 7, 64, p), "above the cap of 64"),
                           ((p, 4, 5, 65, 64, p), "above the cap of 64"), ((p + 4, 4, 5, 7, 64, p), "16-byte aligned")):
            assert fn(*args, None) < 0
            e = lib.gg_last_error().decode()
            assert e.startswith(who) and text in e, e
