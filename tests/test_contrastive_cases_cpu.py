"""tests/contrastive_cases.py checked without a GPU: the builders give each class its property, the conditions on the case list hold for every case of the GPU
suite, the f32 restatement of the kernel's formula passes every downstream gate, and every restated defect is rejected by one.  Nothing here runs a kernel;
`pytest -s` prints the tables.  The downstream stage takes the f32 yardstick's forward tensors in place of the tensors a call returned.

Which case catches which defect (``CATCHES``; the defective f32 result is fed to the gate as if it were the kernel's):

* ``lse_ulp``         ``cluster`` at B = 2 and 5, ``aligned`` and ``dup`` at B >= 64, ls = 4.6052: an ulp of a logit of 100 is 7.6e-6, the loss and the softmax terms
                      carry it (``cluster`` B = 2: loss 1.2e-5 against a gate of 2.4e-7; ``aligned`` B = 64: d_logit_scale 9.4e-7 against 2.4e-7)
* ``col_from_rows``   every class but a symmetric S (shown invisible on one)
* ``first_256``       B = 257: ``aligned`` loses the diagonal term of row 256, ``plain`` one term in 257
* ``identity_256``    B = 257 and 513
* ``dls_no_g``        d_loss_scale 0.5 and 1/8 (shown invisible at 1)
* ``no_projection``   every class
"""
import functools
import math

import pytest
import torch

from tests import contrastive_cases as CC


@functools.lru_cache(maxsize=None)
def _stage(kind, B, P, ls, g):
    """The yardstick's forward tensors and, on them, the downstream reference and yardstick.  Computed once; do not modify."""
    img, txt = CC.inputs(kind, B, P)
    fy = CC.forward(img, txt, ls, CC.F32)
    S, I, T = (fy[k] for k in ("logits_per_text", "image_embeds", "text_embeds"))
    return img, txt, S, I, T, CC.downstream(S, I, T, img, txt, ls, g, CC.F64), CC.downstream(S, I, T, img, txt, ls, g, CC.F32)


def _gate(kind, B, P, ls, g, got, label):
    img, txt, S, I, T, ref, yard = _stage(kind, B, P, ls, g)
    return CC.check_downstream(S, I, T, img, txt, ls, g, got, CC.case_name(kind, B, P, ls, g), label, ref=ref, yard=yard)[0]


def test_every_class_has_its_property():
    B, P = 64, 64
    cos = {}
    for kind in CC.KINDS:
        img, txt = CC.inputs(kind, B, P)
        assert img.dtype == txt.dtype == torch.float32 and img.shape == txt.shape == (B, P)
        cos[kind] = CC.forward(img, txt, 0.0)["logits_per_text"]          # e^0: the cosines
    old = torch.Generator().manual_seed(B * 1000 + P)                      # the draw of tests/test_gpu_clip_text.py::test_contrastive_head_against_fp64
    assert torch.equal(CC.inputs("plain", B, P)[0], torch.randn(B, P, generator=old) * 3) and torch.equal(CC.inputs("plain", B, P)[1], torch.randn(B, P, generator=old) * 0.5)
    assert float(cos["plain"].abs().max()) < 0.6
    assert float(cos["cluster"].min()) > 0.9 and float(cos["cluster"].max() - cos["cluster"].min()) < 0.1
    # cos(u, u + 2 n) is 1 / sqrt(5) on the diagonal, N(0, 1 / P) elsewhere: the diagonal wins most rows and columns at B = P = 64
    assert abs(float(cos["aligned"].diagonal().mean()) - 5 ** -0.5) < 0.05
    assert int((cos["aligned"].argmax(1) == torch.arange(B)).sum()) >= 0.8 * B and int((cos["aligned"].argmax(0) == torch.arange(B)).sum()) >= 0.8 * B
    assert int((cos["anti"].argmin(1) == torch.arange(B)).sum()) >= 0.8 * B and torch.equal(cos["anti"], -cos["aligned"])
    assert abs(float(cos["one_exact"][0, 0]) - 1.0) < 1e-15 and float(cos["one_exact"][1:, 1:].abs().max()) < 0.6
    d = cos["dup"]
    assert torch.equal(d[0], d[1]) and torch.equal(d[:, 0], d[:, 1]) and d[0, 0] == d[0, 1] == d[0].max()
    # scaled: exact powers of two, the cosines are those of the twin to the last fp64 bit
    for kind in CC.KINDS:
        (img, txt), (simg, stxt) = CC.inputs(kind, 5, 64), CC.inputs(kind, 5, 64, scaled=True)
        sc = CC.row_scales(5)
        assert torch.equal(simg, img * sc) and torch.equal(stxt * sc, txt) and torch.equal(simg / sc, img)
        assert float(sc[0]) == 2.0 ** 40 and float(sc[1]) == 2.0 ** -40
        assert float(simg.abs().max()) ** 2 * 64 < 3e38
        assert torch.equal(CC.forward(simg, stxt, 4.6052)["logits_per_text"], CC.forward(img, txt, 4.6052)["logits_per_text"])
    for kind in CC.EDGE_KINDS:
        img, txt = CC.inputs(kind, 5, 64)
        f = CC.forward(img, txt, 2.6592)
        assert bool(torch.isnan(f["image_embeds"][1]).all()) and bool(torch.isfinite(f["image_embeds"][[0, 2, 3, 4]]).all())
        assert bool(torch.isnan(f["logits_per_text"][:, 1]).all()) and bool(torch.isfinite(f["logits_per_text"][:, [0, 2, 3, 4]]).all())
        r = CC.downstream(f["logits_per_text"], f["image_embeds"], f["text_embeds"], img, txt, 2.6592, 1.0)
        assert all(bool(torch.isnan(r[k]).all()) for k in CC.DOWNSTREAM_TENSORS)
    assert CC.inputs("plain", 3, 64, Bt=7)[0].shape == (3, 64) and CC.inputs("plain", 3, 64, Bt=7)[1].shape == (7, 64)


def test_case_list_covers_what_it_must_and_leaves_out_only_the_named_cases():
    cases = CC.gpu_suite_cases()
    assert len(cases) == len(set(cases))
    full = {(k, B, P, ls) for k in CC.KINDS for B, P in CC.shapes() for ls in CC.LOGIT_SCALES}
    gone = full - set(cases)
    assert all((k in ("aligned", "dup") and B <= 5 and ls == 4.6052) or (k == "dup" and B == 2) for k, B, P, ls in gone)
    assert {B for B, P in CC.shapes() if P == 64} == set(CC.SWEEP_B) and {P for B, P in CC.shapes() if B == 257} == set(CC.SWEEP_P) == {P for B, P in CC.shapes() if B == 5}
    for k in ("cluster", "aligned"):
        assert (k, 257, 64, 4.6052) in cases and (k, 64, 64, 4.6052) in cases


def test_conditions_hold_and_the_fixed_formula_passes_on_every_case_of_the_gpu_suite():
    """fp64 loss >= 1e-3, every yardstick figure <= 1e-5, every reference gradient non-zero; formula_f32 inside every downstream gate at d_loss_scale 0.5."""
    print()
    worst = {}
    g = 0.5
    for kind, B, P, ls in CC.gpu_suite_cases():
        name = CC.case_name(kind, B, P, ls)
        img, txt, S, I, T, ref, yard = _stage(kind, B, P, ls, g)
        f64 = CC.forward(img, txt, ls, CC.F64)
        y = {k: CC.figure(CC._np(v), CC._np(f64[k])) for k, v in (("image_embeds", I), ("text_embeds", T), ("logits_per_text", S))}
        y.update(CC.downstream_figures(yard, ref))
        assert float(ref["loss"]) >= CC.LOSS_MIN, (name, float(ref["loss"]))
        assert all(v <= CC.Y_CAP for v in y.values()), (name, y)
        assert all(float(ref[k].abs().max()) > 0.0 for k in ("d_img", "d_txt")) and float(ref["dls_abs"]) > 0.0, name
        for k, v in y.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert not _gate(kind, B, P, ls, g, CC.formula_f32(S, I, T, img, txt, ls, g), "fixed formula"), name
        assert not _gate(kind, B, P, ls, g, yard, "yardstick"), name
    print("[yardstick] worst: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("g", [1.0, 0.125])
def test_the_fixed_formula_passes_at_the_other_loss_scales(g):
    for kind in CC.KINDS:
        for B, P, ls in ((64, 64, 4.6052), (257, 64, 4.6052), (5, 68, 2.6592)):
            img, txt, S, I, T, ref, yard = _stage(kind, B, P, ls, g)
            assert not _gate(kind, B, P, ls, g, CC.formula_f32(S, I, T, img, txt, ls, g), "fixed formula"), (kind, B, P, ls, g)


# defect -> [(kind, B, P, ls, d_loss_scale)], every one a case of the GPU suite
CATCHES = {
    "lse_ulp": [("cluster", 2, 64, 4.6052, 0.5), ("cluster", 5, 64, 4.6052, 0.5), ("aligned", 64, 64, 4.6052, 0.5), ("aligned", 257, 64, 4.6052, 0.5),
                ("dup", 64, 64, 4.6052, 1.0)],
    "col_from_rows": [("plain", 5, 64, 2.6592, 0.5), ("aligned", 64, 64, 4.6052, 1.0), ("cluster", 257, 64, 0.0, 0.125)],
    "first_256": [("aligned", 257, 64, 4.6052, 0.5), ("plain", 257, 64, 2.6592, 1.0), ("cluster", 513, 64, 0.0, 0.5)],
    "identity_256": [("plain", 257, 64, 2.6592, 0.5), ("aligned", 257, 768, 4.6052, 1.0), ("anti", 513, 64, 0.0, 0.125)],
    "dls_no_g": [("plain", 5, 64, 2.6592, 0.5), ("cluster", 64, 64, 4.6052, 0.125), ("aligned", 257, 64, 4.6052, 0.5)],
    "no_projection": [("plain", 2, 64, 2.6592, 0.5), ("cluster", 5, 4, 4.6052, 1.0), ("aligned", 256, 64, 4.6052, 0.125), ("dup", 64, 64, 0.0, 0.5)],
}


@pytest.mark.parametrize("defect", CC.DEFECTS)
def test_every_defect_is_rejected_by_a_downstream_gate(defect):
    print()
    suite = set(CC.gpu_suite_cases())
    for kind, B, P, ls, g in CATCHES[defect]:
        assert (kind, B, P, ls) in suite and g in CC.LOSS_SCALES
        img, txt, S, I, T, ref, yard = _stage(kind, B, P, ls, g)
        misses = _gate(kind, B, P, ls, g, CC.formula_f32(S, I, T, img, txt, ls, g, defect=defect), defect)
        print(f"[defect] {defect} {CC.case_name(kind, B, P, ls, g)}: misses {[(n, f'{e:.1e}', f'{g_:.1e}') for n, e, g_ in misses]}")
        assert misses, (defect, kind, B, P, ls, g)
        assert not _gate(kind, B, P, ls, g, CC.formula_f32(S, I, T, img, txt, ls, g), "sound"), (kind, B, P, ls, g)
    if defect == "dls_no_g":            # invisible at d_loss_scale 1
        img, txt, S, I, T, ref, yard = _stage("plain", 5, 64, 2.6592, 1.0)
        assert not _gate("plain", 5, 64, 2.6592, 1.0, CC.formula_f32(S, I, T, img, txt, 2.6592, 1.0, defect=defect), defect)
    if defect == "col_from_rows":       # invisible on a symmetric S: the same rows on both sides
        img, _ = CC.inputs("plain", 5, 64)
        f = CC.forward(img, img, 2.6592, CC.F32)
        S = (f["logits_per_text"] + f["logits_per_text"].t()) / 2
        ref, yard = (CC.downstream(S, f["image_embeds"], f["text_embeds"], img, img, 2.6592, 0.5, dt) for dt in (CC.F64, CC.F32))
        got = CC.formula_f32(S, f["image_embeds"], f["text_embeds"], img, img, 2.6592, 0.5, defect=defect)
        assert not CC.check_downstream(S, f["image_embeds"], f["text_embeds"], img, img, 2.6592, 0.5, got, "symmetric", defect, ref=ref, yard=yard)[0]
    if defect == "first_256":           # B = 256 cannot see it
        img, txt, S, I, T, ref, yard = _stage("aligned", 256, 64, 4.6052, 0.5)
        assert not _gate("aligned", 256, 64, 4.6052, 0.5, CC.formula_f32(S, I, T, img, txt, 4.6052, 0.5, defect=defect), defect)


def test_figures_treat_non_finite_results_as_the_reference_does():
    nan, one = torch.tensor(math.nan), torch.tensor(1.0)
    assert CC.dls_figure(nan, nan, nan) == 0.0 and CC.dls_figure(one, nan, nan) == math.inf and CC.dls_figure(nan, one, one) == math.inf
    assert CC.dls_figure(one, one, one) == 0.0 and CC.dls_figure(torch.tensor(1.5), one, torch.tensor(2.0)) == 0.25
    img, txt = CC.inputs("nan_row", 5, 64)
    f = CC.forward(img, txt, 2.6592, CC.F32)
    assert not CC.check_forward(img, txt, 2.6592, f, "nan_row yardstick")
    finite = dict(f, image_embeds=torch.nan_to_num(f["image_embeds"]))
    assert [m[0] for m in CC.check_forward(img, txt, 2.6592, finite, "nan_row made finite")] == ["image_embeds"]
    assert not CC.check_forward(img, txt, 2.6592, finite, "nan_row rows", rows=[0, 2, 3, 4])
