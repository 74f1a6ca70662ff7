"""Memory discipline of include/gg_pad.h, in the way tests/test_gpu_guards_text.py holds its header: every tensor of a call lives in a guarded buffer
(tests/guards.py), each case runs under the NaN fill and the large-finite fill of the bands, and asserts that inputs are unchanged, that only -- and all of -- the
logical outputs were written, that the two runs agree bit for bit, and that the values are those of torch indexing.

CASES is the registry; test_every_pad_entry_point_is_guarded_or_exempt (no GPU needed) holds it and EXEMPT against the header's prototypes."""
import os
import re

import pytest
import torch

from tests.test_gpu_guards import rnd, run_guarded

gpu = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
CASES = {}
EXEMPT = {}                  # both prototypes take the caller's tensors: nothing is exempt


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


def _declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gg_pad.h")).read(), flags=re.S)
    return set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", hdr))


def test_every_pad_entry_point_is_guarded_or_exempt():
    """Every prototype of include/gg_pad.h is called by a guard case of this file or is in EXEMPT with its reason -- exactly one of the two; and a case really calls
    what it registers."""
    from tests.test_guards_cpu import _coverage_gaps
    declared = _declared()
    guarded = {e for _, es in CASES.values() for e in es}
    missing, unknown, both = _coverage_gaps(declared, guarded, EXEMPT)
    assert not missing, f"entry points of include/gg_pad.h with neither a guard test nor an exemption: {missing}"
    assert not unknown, f"registry / exemption names the header does not declare: {unknown}"
    assert not both, f"both guarded and exempt: {both}"
    src = open(__file__).read()
    for name, (fn, entries) in CASES.items():
        body = src[src.index(f"def {name}("):]
        body = body[:body.index("\n\n\n")] if "\n\n\n" in body else body
        for e in entries:
            assert re.search(r"\b" + e + r"\b", body), (name, e)
    for victim in ("gg_window_pad", "gg_window_crop_add"):
        assert _coverage_gaps(declared, guarded - {victim}, EXEMPT)[0] == [victim]
    assert len(guarded) == len(declared) == 2 and not EXEMPT


# (B, H, Hp, C): one pixel of padding on a multi-window map, a map padded to one large window, a one-image map, the widest stage
SHAPES = [(3, 20, 21, 64), (2, 10, 14, 160), (1, 5, 7, 576), (2, 20, 32, 64)]


@case("gg_window_pad")
@gpu
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("B,H,Hp,Cc", SHAPES)
def test_window_pad(dtype, B, H, Hp, Cc):
    """gg_window_pad: x exactly [B * H * H, C], y exactly [B * Hp * Hp, C]; every element of y is written (the guard's NaN pre-fill of the logical output is gone),
    nothing around either tensor is touched."""
    dt = F32 if dtype == 1 else BF
    x = rnd(B * H * H, Cc, seed=11, dtype=dt)
    want = torch.zeros(B, Hp, Hp, Cc)
    want[:, :H, :H] = x.view(B, H, H, Cc)

    def call(S, L):
        xi = S.inp("x", x.to(dt))
        y = S.out("y", B * Hp * Hp, Cc, dt)
        L.check(L.lib().gg_window_pad(xi.ptr, y.ptr, B, H, H, Hp, Hp, Cc, dtype, L.stream()), "gg_window_pad")

        def check(val):
            assert torch.equal(val["y"].float(), want.view(-1, Cc))
        return {"y": y}, check
    run_guarded(call)


@case("gg_window_crop_add")
@gpu
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("variant", ["res+scale", "plain", "alias"])
@pytest.mark.parametrize("B,H,Hp,Cc", SHAPES)
def test_window_crop_add(dtype, variant, B, H, Hp, Cc):
    """gg_window_crop_add: t exactly [B * Hp * Hp, C] (read at the padded pitch: its pad rows and columns are read by nobody, and nothing beyond it is), res / y exactly
    [B * H * H, C], rowscale exactly [B]; with y == res the accumulating output is the only tensor written."""
    dt = F32 if dtype == 1 else BF
    t, res = rnd(B * Hp * Hp, Cc, seed=21, dtype=dt), rnd(B * H * H, Cc, seed=22, dtype=dt)
    rs = torch.tensor([1.25, 0.0, 1.0 / 0.9][:B])
    crop = t.view(B, Hp, Hp, Cc)[:, :H, :H]
    want = crop if variant == "plain" else res.view(B, H, H, Cc) + crop * rs[:, None, None, None]
    want = want.to(dt).float().reshape(-1, Cc)

    def call(S, L):
        ti = S.inp("t", t.to(dt))
        if variant == "alias":
            y = S.out("y", B * H * H, Cc, dt, init=res.to(dt))
            ri, si = y, S.inp("rowscale", rs.view(1, B))
        elif variant == "plain":
            y, ri, si = S.out("y", B * H * H, Cc, dt), None, None
        else:
            y, ri, si = S.out("y", B * H * H, Cc, dt), S.inp("res", res.to(dt)), S.inp("rowscale", rs.view(1, B))
        L.check(L.lib().gg_window_crop_add(ti.ptr, ri.ptr if ri is not None else None, si.ptr if si is not None else None, y.ptr, B, H, H, Hp, Hp, Cc, dtype, L.stream()),
                "gg_window_crop_add")

        def check(val):
            assert torch.equal(val["y"].float(), want)
        return {"y": y}, check
    run_guarded(call)
