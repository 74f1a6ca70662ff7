"""CPU-side checks of tests/act_cases.py: the probe sets are what they say, the bounds csrc/common.h states hold for the restated forms (fused and unfused),
the faithful restatement is inside every gate at every probe, and every listed defect is rejected.  No GPU, no libgg.

Measured (`pytest -s`): supremum of restated gg_gelu_grad_f32 against fp64 over P32 1.14e-7 at z = 0.75179 (1.40e-7 unfused); the other suprema are in the
docstring of tests/act_cases.py."""
import math

import pytest
import torch

from tests import act_cases as A


def _sup(got, ref):
    e = (got.double() - ref).abs()
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    i = int(e.argmax())
    return float(e[i]), i


def _union():
    return torch.cat([A.probes("P16").float(), A.probes("P32")])


def test_probe_sets_have_the_stated_sizes_and_members():
    p16, p16h, p32, nf = (A.probes(n) for n in ("P16", "P16H", "P32", "NONFINITE"))
    for p in (p16, p16h, p32, nf):
        assert p.numel() == 65536 == A.ROWS * A.COLS
    assert p16.dtype == A.BF16 and p16h.dtype == A.F16 and p32.dtype == A.F32
    assert torch.isfinite(p16.float()).all() and torch.isfinite(p16h.float()).all() and torch.isfinite(p32).all()
    assert p16[:65280].view(torch.int16).unique().numel() == 65280 and (p16[65280:] == 0).all()
    assert p16h[:63488].view(torch.int16).unique().numel() == 63488 and (p16h[63488:] == 0).all()
    assert float(p16.float().abs().max()) > 3.3e38
    have = set(p32.view(torch.int32).tolist())
    bits = lambda v: int(torch.tensor([v], dtype=A.F32).view(torch.int32))
    for c in (0.75179, 4.2426407, 4.75, 5.939697, 1.0 / 1.702):
        for sgn in (1.0, -1.0):
            b = bits(sgn * c)
            assert all(b + d in have for d in range(-128, 129)), c
    assert all(bits(k * 2.0 ** -149) in have for k in range(-128, 129))
    assert all(bits(s * 2.0 ** k) in have for k in range(-149, 128) for s in (1.0, -1.0))
    b = A.probes("P16").float()
    assert set(b[b.abs() <= 16].view(torch.int32).tolist()) <= have
    grid = (torch.arange(-8192, 8193, dtype=torch.float64) * 2.0 ** -9 + 2.0 ** -9 / math.pi).float()
    assert set(grid.view(torch.int32).tolist()) <= have
    # NONFINITE: each class on both lanes of a pair, every non-finite value between finite neighbours, the finite values exact in bf16 and fp16
    fin = torch.isfinite(nf)
    for cls in (nf == math.inf, nf == -math.inf, torch.isnan(nf)):
        idx = cls.nonzero().flatten()
        assert idx.numel() > 3000 and (idx % 2 == 0).any() and (idx % 2 == 1).any() and {int(i) % 8 for i in idx} == set(range(8))
    bad = (~fin).nonzero().flatten()
    assert fin[bad - 1].all() and fin[bad + 1].all()
    f = nf[fin]
    assert torch.equal(f.to(A.BF16).float(), f) and torch.equal(f.to(A.F16).float(), f)
    codes, vals, scales = A.p8()
    assert codes.numel() == 254 and vals.abs().max() == 448.0 and scales.numel() == 15 and scales[0] == 2.0 ** -10 and scales[-1] == 16.0
    if hasattr(torch, "float8_e4m3fn"):
        assert torch.equal(codes.view(torch.float8_e4m3fn).double(), vals)


def test_references_use_erfc_and_agree_with_autograd():
    z = torch.linspace(-12.0, 12.0, 4801, dtype=torch.float64, requires_grad=True)
    for kind in ("gelu", "quick"):
        (g,) = torch.autograd.grad(A.reference(kind, z).sum(), z)
        assert float((g - A.reference(kind + "_grad", z.detach())).abs().max()) < 1e-14
    # the tail is relative: GELU(-12) = -12 Phi(-12) = -2.13e-32 to 1e-13, where 1 + erf gives 0
    assert abs(float(A.reference("gelu", torch.tensor([-12.0]))[0]) / (-12.0 * 1.7764821120776e-33) - 1.0) < 1e-9


@pytest.mark.parametrize("fused", (True, False), ids=("fused", "unfused"))
def test_the_bounds_common_h_states_hold_for_the_restated_forms(fused):
    x = _union()
    z = x.double()
    ctx = A.unfused() if not fused else torch.no_grad()
    with ctx:
        got = {f: A.restated(f, x) for f in ("erf16", "gelu16", "gelu16_v2", "gelu_grad16", "phi32", "gelu32", "gelu_grad32")}
    sups = {"erf16": _sup(got["erf16"], torch.special.erf(z / math.sqrt(2.0))), "gelu16": _sup(got["gelu16"], A.reference("gelu", z)),
            "gelu16_v2": _sup(got["gelu16_v2"], A.reference("gelu", z)), "gelu_grad16": _sup(got["gelu_grad16"], A.reference("gelu_grad", z)),
            "phi32": _sup(got["phi32"], A.phi64(z))}
    ref = A.reference("gelu", z)
    rel = torch.where(ref.abs() > A.GELU32_REL_FROM, (got["gelu32"].double() - ref).abs() / ref.abs(), torch.zeros_like(ref))
    sups["gelu32 relative"] = (float(rel.max()), int(rel.argmax()))
    for k, (e, i) in sups.items():
        print(f"  {k}: supremum {e:.3e} at z = {float(z[i])!r}")
    assert sups["erf16"][0] <= A.ERF16_BOUND
    assert sups["gelu16"][0] <= A.GELU16_BOUND and sups["gelu16_v2"][0] <= A.GELU16_BOUND
    assert sups["gelu_grad16"][0] <= A.GELU_GRAD16_BOUND
    assert sups["phi32"][0] <= A.PHI32_BOUND
    assert sups["gelu32 relative"][0] <= A.GELU32_REL
    # what the statements rest on: the clamp of erf at the fit edge, and GELU' beyond its clamp
    assert 1.0 - math.erf(3.0) <= A.ERF16_BOUND and 1.5 * math.sqrt(2.0) * (1.0 - math.erf(3.0)) <= A.GELU16_BOUND
    tails = A.restated("gelu_grad16", torch.tensor([-1e30, -4.76, 4.76, 1e30]))
    assert torch.equal(tails[:2], tails[:1].expand(2)) and abs(float(tails[0])) <= A.GELU_GRAD16_BOUND and abs(float(tails[3]) - 1.0) <= A.GELU_GRAD16_BOUND


def test_gelu_grad_f32_supremum_is_the_constant_of_its_gate():
    s = A.gelu_grad32_sup()
    with A.unfused():
        z = A.probes("P32")
        s_unfused = float((A.restated("gelu_grad32", z).double() - A.reference("gelu_grad", z)).abs().max())
    print(f"  restated gg_gelu_grad_f32 against fp64 over P32: supremum {s:.4e} (unfused {s_unfused:.4e}); gate constant: that supremum + 2^-22")
    assert float(A.form_bound("gelu_grad32", torch.zeros(1))[0]) == s + 2.0 ** -22            # the gate uses the computed supremum itself
    assert 1.10e-7 <= s <= 1.18e-7                      # the figure the docstrings quote (1.14e-7): a restatement that drifts is noticed
    assert s_unfused <= s + 2.0 ** -22


@pytest.mark.parametrize("form,gate,store,pset", A.FAITHFUL, ids=lambda v: str(v).replace("torch.", ""))
def test_faithful_restatement_is_inside_its_gate_everywhere(form, gate, store, pset):
    x = A.probes(pset).float()
    A.assert_inside(A.stored(A.restated(form, x), store), x, gate, store, f"restated {form} on {pset}")


def test_faithful_restatement_has_the_required_non_finite_classes():
    x = A.probes("NONFINITE")
    for form, gate, store in (("gelu16_v2", "gelu16", A.BF16), ("gelu32", "gelu32", A.F32), ("quick16", "quick", A.BF16), ("quick32", "quick", A.F32),
                              ("gelu_grad16", "gelu_grad16", A.BF16), ("gelu_grad32", "gelu_grad32", A.F32), ("quick_grad16", "quick_grad", A.BF16),
                              ("quick_grad32", "quick_grad", A.F32)):
        A.assert_inside(A.stored(A.restated(form, x), store), x, gate, store, f"restated {form} on NONFINITE")


@pytest.mark.parametrize("defect", sorted(A.DEFECTS))
def test_every_listed_defect_is_rejected(defect):
    for form, gate, store, pset in A.DEFECTS[defect]:
        x = A.probes(pset).float()
        worst, w, bad = A.check(A.stored(A.restated(form, x, defect), store), x, gate, store)
        print(f"  {defect} in {form} / {str(store).replace('torch.', '')} on {pset}: worst err/gate {worst:.3g} at z = {float(x[w])!r}")
        assert worst > 1.0 or bad, (defect, form)


def test_quick_gelu_grad_without_its_clamp_is_nan_for_finite_arguments():
    """s + 1.702 x s (1 - s) left to right: 1.702 x is inf for |x| > 2e38 and inf * 0 is NaN.  The clamp on the product term's argument removes it and changes
    no other result: s (1 - s) is exactly 0 in f32 from |x| = 62 on (s is 1, or has underflowed to 0), far below the clamp at 1e30."""
    x = A.probes("P16").float()
    for form in ("quick_grad16", "quick_grad32"):
        y0, y1 = A.restated(form, x, "no_grad_clamp"), A.restated(form, x)
        assert int(torch.isnan(y0).sum()) > 0 and torch.isfinite(y1).all()
        keep = torch.isfinite(y0)
        assert torch.equal(y0[keep], y1[keep])
        _, _, bad = A.check(y0, x, "quick_grad", A.F32)
        assert bad
