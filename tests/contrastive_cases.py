"""Inputs for the CLIP contrastive head (gg_clip_contrastive, csrc/contrastive.hip) away from the untrained state, their fp64 references and the yardsticks the
tests gate against.  Plain torch on the CPU: no GPU, no libgg.  The pattern is that of tests/geo_cases.py.

Inputs (``inputs(kind, B, P)``): a torch.Generator seeded B * 1000 + P draws u = randn(B, P), n = randn(B, P), c = randn(1, P) in this order.

* ``plain``      img = 3 u, txt = 0.5 n: unrelated rows, every cosine about 1 / sqrt(P), loss about log B -- the draw of the older tests, the control
* ``cluster``    img = 3 (c + 0.15 u), txt = 0.5 (c + 0.15 u + 0.1 n): every cosine high, every logit within a few units of e^ls
* ``aligned``    img = 3 u, txt = 0.5 (u + a n), a = 2: the trained state, the diagonal wins.  Two noise levels differ (``aligned_noise``), each because a = 2 breaks a
                 condition below: at P = 768 a = 7.7 (the other cosines shrink to 1 / sqrt(768); with a = 2 the loss at ls = 4.6052 underflows to 3e-13; 7.7 keeps
                 the diagonal cosine times sqrt(P) where it is at P = 64), and ``dup`` at B = 3 has a = 3 (with a = 2 torch's f32 gradients are 1.1e-5 off)
* ``anti``       ``aligned`` with txt negated: the label is the smallest logit of its row, row losses reach about 2 e^ls
* ``one_exact``  ``plain`` with txt[0] = 0.125 img[0]: one cosine is exactly 1, one logit e^ls
* ``dup``        ``aligned`` with rows 0 and 1 equal on both sides: tied maxima, two equal columns
* ``scaled=True``  any of these with row r of img times 2^(+40, -40, +40, ...) and row r of txt times 2^(-40, +40, ...): exact in f32, and a power of two commutes
                 with every operation of the normalise kernels, so every normalised output must keep its bits
* ``nan_row`` / ``zero_row``  ``plain`` with img[1] all NaN / all 0 (0 / 0: the row of image_embeds is NaN in fp64 too)

logit_scale is one of ``LOGIT_SCALES`` (0, ln 14.28, the ceiling ln 100), d_loss_scale one of ``LOSS_SCALES`` (powers of two).  Every reference sees the
f32-rounded logit_scale and d_loss_scale the C call is given.

References, fp64, from f32 tensors widened first:

* forward (``forward``): img_n, txt_n, logits_per_text as tests/test_gpu_clip_text.py::contrastive_ref writes them.
* downstream (``downstream``): a function of the tensors the call RETURNED -- S = logits_per_text, I = image_embeds, T = text_embeds, f32, widened:
  loss* = (CE(S) + CE(S^T)) / 2 against the diagonal, dS* from autograd of d_loss_scale x loss*, d_logit_scale* = sum dS* o S, dT = e^ls dS* I,
  dI = e^ls dS*^T T, d_txt* = (dT - T (T . dT)) / |txt| and d_img* alike with the fp64 norms of the inputs: what include/gg_clip_text.h states.  The f32 rounding
  of the logits themselves (an ulp of 100 at the ceiling, as large as the defect the cases are after) is thereby out of the comparison.

Yardstick: the same statements in torch f32 on the CPU (``forward`` / ``downstream`` with dtype float32: F.cross_entropy + autograd on the f32 S, f32 matmuls and
norms).  Never the kernel.

Error figure: e(T) = max |got - ref| / max |ref| (tests/geo_cases.py::figure: where the reference is not finite the result must not be either, and the reverse,
otherwise e = inf).  d_logit_scale is a scalar with heavy cancellation: |got - ref| / sum |dS* o S|.  Gate: e <= 4 max(y, 2^-24), y the yardstick's figure on the
same case.

Conditions on the case list (tests/test_contrastive_cases_cpu.py asserts them for every case of the GPU suite): the fp64 loss is >= 1e-3, every yardstick
figure is <= 1e-5, every reference gradient has max |ref| > 0.  Left out for breaking them: ``aligned`` and ``dup`` at B <= 5 with ls = 4.6052 (the loss
underflows to about 1e-8, torch's own f32 is off by 13 %), ``dup`` at B = 2 (the reference gradients vanish).

``formula_f32``: the kernel's statements in f32 on the CPU -- row / column maxima and log(sum) kept apart (the sum of the f32 exponentials and its log in double),
softmax terms exp((s - max) - logsum), on the diagonal expm1 + expm1 in place of exp + exp - 2, row loss (logsum_r - (s_rr - max_r)) + (logsum_c - (s_rr - max_c)).  tests/test_contrastive_cases_cpu.py holds it inside every downstream gate and shows each of
``DEFECTS`` (restated kernel bugs applied to it) rejected:

* ``lse_ulp``         lse = max + log(sum) in f32, stored as one float, softmax exp(s - lse), row loss lse_r + lse_c - 2 s_rr: the kernel before this module existed
* ``col_from_rows``   the column maxima and log-sums taken from the rows (invisible on a symmetric S)
* ``first_256``       the maxima and sums cover only the first 256 columns / rows
* ``identity_256``    the -2 [r == c] term missing for r >= 256
* ``dls_no_g``        d_loss_scale missing from d_logit_scale
* ``no_projection``   the n (n . dn) term missing from the normalisation backward

Largest measured figures on an MI355X (tests/test_gpu_contrastive_conditioning.py, `pytest -s`): the largest kernel figure e / the yardstick's y on that case, and the
largest e / gate over all cases:
  forward:     image_embeds 5.3e-08 / 1.3e-07 (0.20 of its gate)   text_embeds 5.2e-08 / 9.3e-08 (0.19)   logits_per_text 1.1e-07 / 2.8e-07 (0.25)
  downstream:  loss 2.9e-07 / 7.6e-06 (0.33)   d_logit_scale 2.1e-07 / 5.6e-06 (0.37)   d_img 4.1e-06 / 3.5e-06 (0.57)   d_txt 3.9e-06 / 3.6e-06 (0.54)
  largest yardstick figure of any case: image_embeds 1.5e-07, text_embeds 1.6e-07, logits_per_text 6.3e-07, loss 7.6e-06, d_logit_scale 5.6e-06, d_img 3.5e-06, d_txt 4.3e-06
The kernels as they were before this module (lse = max + logf(sum) in one float, rows times the rounded reciprocal norm, cosines as an f32 chain on the matrix
pipe): 56 of the 115 tests fail; loss 1.6e-05 against a gate of 2.4e-07 (``cluster`` B = 2, ls = 4.6052), d_logit_scale 9.6e-07 against 2.4e-07 and d_img 1.3e-06
against 3.9e-07 (``aligned`` B = 64, ls = 4.6052), d_txt 7.4e-05 against 1.3e-05 (``aligned`` B = 2, ls = 2.6592), logits_per_text 3.9e-07 against 2.4e-07 (``plain`` B = 2).
With the maxima and log-sums merely kept apart, in f32, ``aligned`` B = 5 at ls = 2.6592 still missed (loss 3.7e-07, d_logit_scale 4.0e-07 against 2.4e-07: where the
label wins, the sum is 1 + a little and rounds to an ulp of 1; on the diagonal two softmax terms near 1 are subtracted from 2): hence the double sum and expm1.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.geo_cases import figure

F32, F64 = torch.float32, torch.float64
FLOOR, FACTOR = 2.0 ** -24, 4.0
LOSS_MIN, Y_CAP = 1e-3, 1e-5
KINDS = ("plain", "cluster", "aligned", "anti", "one_exact", "dup")
EDGE_KINDS = ("nan_row", "zero_row")
LOGIT_SCALES = (0.0, 2.6592, 4.6052)
LOSS_SCALES = (1.0, 0.5, 0.125)
DEFECTS = ("lse_ulp", "col_from_rows", "first_256", "identity_256", "dls_no_g", "no_projection")
FORWARD_TENSORS = ("image_embeds", "text_embeds", "logits_per_text")
DOWNSTREAM_TENSORS = ("loss", "d_logit_scale", "d_img", "d_txt")
SWEEP_B, SWEEP_P, P_AT_B = (2, 3, 4, 5, 64, 255, 256, 257, 513), (4, 64, 68, 768), (5, 257)
RECT_SHAPES = ((3, 7), (7, 3), (1, 5), (257, 2))
NOISE_P768, NOISE_DUP_B3 = 7.7, 3.0


def f32r(x):
    """The value a float parameter or a device f32 scalar of the C call carries."""
    return float(np.float32(x))


def row_scales(B):
    """(B, 1) f32: what ``scaled`` multiplies row r of img by (txt: its inverse)."""
    return torch.tensor([2.0 ** 40 if r % 2 == 0 else 2.0 ** -40 for r in range(B)], dtype=F32).reshape(-1, 1)


def aligned_noise(kind, B, P):
    """a of txt = 0.5 (u + a n).  2 but where that breaks a condition on the case list (module docstring)."""
    if P == 768:
        return NOISE_P768
    if kind == "dup" and B == 3:
        return NOISE_DUP_B3
    return 2.0


@functools.lru_cache(maxsize=None)
def inputs(kind, B, P, scaled=False, Bt=None):
    """(img (B, P), txt (Bt or B, P)) f32.  Computed once; do not modify.  ``Bt``: a rectangular pair (forward only), the first rows of the draw for max(B, Bt)."""
    n_rows = B if Bt is None else max(B, Bt)
    g = torch.Generator().manual_seed(n_rows * 1000 + P)
    u, n, c = torch.randn(n_rows, P, generator=g), torch.randn(n_rows, P, generator=g), torch.randn(1, P, generator=g)
    if kind in ("plain", "one_exact", "nan_row", "zero_row"):
        img, txt = u * 3, n * 0.5
    elif kind == "cluster":
        img, txt = (c + 0.15 * u) * 3, (c + 0.15 * u + 0.1 * n) * 0.5
    elif kind in ("aligned", "anti", "dup"):
        img, txt = u * 3, (u + aligned_noise(kind, B, P) * n) * 0.5
    else:
        raise ValueError(kind)
    if kind == "anti":
        txt = -txt
    if kind == "one_exact":
        txt[0] = 0.125 * img[0]
    if kind == "dup":
        img[1], txt[1] = img[0], txt[0]
    if kind == "nan_row":
        img[1] = math.nan
    if kind == "zero_row":
        img[1] = 0.0
    if scaled:
        img, txt = img * row_scales(n_rows), txt / row_scales(n_rows)
    if Bt is not None:
        img, txt = img[:B], txt[:Bt]
    return img.contiguous(), txt.contiguous()


def forward(img, txt, ls, dtype=F64):
    """image_embeds, text_embeds, logits_per_text in ``dtype`` (fp64: the reference; f32: the yardstick)."""
    i, t = img.to(dtype), txt.to(dtype)
    i_n, t_n = i / i.norm(dim=-1, keepdim=True), t / t.norm(dim=-1, keepdim=True)
    lpt = torch.tensor(f32r(ls), dtype=dtype).exp() * t_n @ i_n.t()
    return dict(image_embeds=i_n, text_embeds=t_n, logits_per_text=lpt)


def clip_loss(S):
    """(CE(S) + CE(S^T)) / 2 against the diagonal, in S's own type."""
    tgt = torch.arange(S.shape[0])
    return (F.cross_entropy(S, tgt) + F.cross_entropy(S.t(), tgt)) / 2


def downstream(S, I, T, img, txt, ls, g, dtype=F64):
    """loss, d_logit_scale, d_img, d_txt (and dls_abs = sum |dS o S|) from the returned S [B][B], I, T and the inputs' norms, in ``dtype``."""
    S_ = S.to(dtype).clone().requires_grad_()
    loss = clip_loss(S_)
    (loss * torch.tensor(f32r(g), dtype=dtype)).backward()
    dS, S_ = S_.grad, S_.detach()
    sc = torch.tensor(f32r(ls), dtype=dtype).exp()
    I_, T_ = I.to(dtype), T.to(dtype)
    dT, dI = sc * dS @ I_, sc * dS.t() @ T_
    nt, ni = txt.to(dtype).norm(dim=-1, keepdim=True), img.to(dtype).norm(dim=-1, keepdim=True)
    return dict(loss=loss.detach(), d_logit_scale=(dS * S_).sum(), dls_abs=(dS * S_).abs().sum(),
                d_txt=(dT - T_ * (T_ * dT).sum(-1, keepdim=True)) / nt, d_img=(dI - I_ * (I_ * dI).sum(-1, keepdim=True)) / ni)


def formula_f32(S, I, T, img, txt, ls, g, defect=None):
    """The kernel's statements (csrc/contrastive.hip) in f32 on the CPU; ``defect``: one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    S, I, T, img, txt = (x.to(F32) for x in (S, I, T, img, txt))
    B = S.shape[0]
    n = 256 if defect == "first_256" else B
    mr, mc = S[:, :n].max(1).values, S[:n, :].max(0).values
    lr, lc = (S[:, :n] - mr[:, None]).exp().double().sum(1).log().float(), (S[:n, :] - mc[None, :]).exp().double().sum(0).log().float()
    if defect == "col_from_rows":
        mc, lc = mr, lr
    d = S.diagonal()
    eye = torch.eye(B, dtype=torch.bool)
    if defect == "identity_256":
        eye[256:] = False
    if defect == "lse_ulp":
        lse_r, lse_c = mr + (S - mr[:, None]).exp().sum(1).log(), mc + (S - mc[None, :]).exp().sum(0).log()
        core = (S - lse_r[:, None]).exp() + (S - lse_c[None, :]).exp() - 2.0 * eye.float()
        rowloss = lse_r + lse_c - 2.0 * d
    else:
        ar, ac = (S - mr[:, None]) - lr[:, None], (S - mc[None, :]) - lc[None, :]
        core = torch.where(eye, torch.expm1(ar) + torch.expm1(ac), ar.exp() + ac.exp())
        rowloss = (lr - (d - mr)) + (lc - (d - mc))
    gf = torch.tensor(f32r(g), dtype=F32)
    dS = core * (gf / (2.0 * B))
    dls = (dS * S).sum(1).double().sum().float()
    if defect == "dls_no_g":
        dls = dls / gf
    G = torch.tensor(f32r(ls), dtype=F32).exp() * dS
    dT, dI = G @ I, G.t() @ T
    inv_t, inv_i = 1.0 / (txt * txt).sum(-1, keepdim=True).sqrt(), 1.0 / (img * img).sum(-1, keepdim=True).sqrt()
    keep = 0.0 if defect == "no_projection" else 1.0
    return dict(loss=(rowloss.double().sum() / (2.0 * B)).float(), d_logit_scale=dls,
                d_txt=(dT - keep * T * (T * dT).sum(-1, keepdim=True)) * inv_t, d_img=(dI - keep * I * (I * dI).sum(-1, keepdim=True)) * inv_i)


# ------------------------------------------------------------------------------------------- figures and gates
def _np(x):
    return np.asarray(x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64)


def dls_figure(got, ref, scale):
    got, ref, scale = float(_np(got)), float(_np(ref)), float(_np(scale))
    if not math.isfinite(ref) or not math.isfinite(got):
        return 0.0 if (not math.isfinite(ref) and not math.isfinite(got)) else math.inf
    err = abs(got - ref)
    return 0.0 if err == 0.0 else (math.inf if scale == 0.0 else err / scale)


def _gate_all(names, fig, label, name, collect):
    bad, cells = [], []
    for k in names:
        e, y = fig(k)
        gate = FACTOR * max(y, FLOOR)
        ok = e <= gate
        cells.append(f"{k} {e:.1e}/{y:.1e} (gate {gate:.1e})" + ("" if ok else " MISS"))
        if collect is not None and e > collect.get(k, (-1.0, 0.0))[0]:
            collect[k] = (e, y)
        if not ok:
            bad.append((k, e, gate))
    print(f"\n[{label} {name}] kernel/yardstick: " + "  ".join(cells))
    return bad


def check_forward(img, txt, ls, got, name, label="forward", collect=None, rows=None):
    """Misses [(tensor, e, gate)] of image_embeds, text_embeds, logits_per_text (absent ones are skipped).  ``rows``: compare only these rows of image_embeds."""
    ref, yard = forward(img, txt, ls, F64), forward(img, txt, ls, F32)

    def fig(k):
        sel = (lambda x: _np(x)[rows]) if rows is not None and k == "image_embeds" else _np
        return figure(sel(got[k]), sel(ref[k])), figure(sel(yard[k]), sel(ref[k]))
    return _gate_all([k for k in FORWARD_TENSORS if got.get(k) is not None], fig, label, name, collect)


def downstream_figures(out, ref):
    """{tensor: e} of a result dict against a downstream reference."""
    f = {k: figure(_np(out[k]), _np(ref[k])) for k in ("loss", "d_img", "d_txt") if out.get(k) is not None}
    if out.get("d_logit_scale") is not None:
        f["d_logit_scale"] = dls_figure(out["d_logit_scale"], ref["d_logit_scale"], ref["dls_abs"])
    return f


def check_downstream(S, I, T, img, txt, ls, g, got, name, label="downstream", collect=None, ref=None, yard=None):
    """Misses of loss, d_logit_scale, d_img, d_txt against the downstream reference of the RETURNED S, I, T.  Returns (misses, {tensor: gate})."""
    ref = downstream(S, I, T, img, txt, ls, g, F64) if ref is None else ref
    yard = downstream(S, I, T, img, txt, ls, g, F32) if yard is None else yard
    e, y = downstream_figures(got, ref), downstream_figures(yard, ref)
    gates = {k: FACTOR * max(y[k], FLOOR) for k in y}
    return _gate_all([k for k in DOWNSTREAM_TENSORS if k in e], lambda k: (e[k], y[k]), label, name, collect), gates


# ------------------------------------------------------------------------------------------- the cases of tests/test_gpu_contrastive_conditioning.py
def shapes():
    """Every B at P = 64, every P at B = 5 and 257."""
    return [(B, 64) for B in SWEEP_B] + [(B, P) for B in P_AT_B for P in SWEEP_P if P != 64]


def left_out(kind, B, ls):
    """The downstream cases that break a condition on the case list (module docstring); their forward stage is still checked."""
    return (kind in ("aligned", "dup") and B <= 5 and ls == 4.6052) or (kind == "dup" and B == 2)


def case_name(kind, B, P, ls, g=None, scaled=False):
    return f"{'scaled ' if scaled else ''}{kind} B={B} P={P} ls={ls:g}" + ("" if g is None else f" g={g:g}")


def gpu_suite_cases():
    """Every downstream case the GPU suite runs: (kind, B, P, ls)."""
    return [(kind, B, P, ls) for kind in KINDS for B, P in shapes() for ls in LOGIT_SCALES if not left_out(kind, B, ls)]
