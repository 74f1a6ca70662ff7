"""gg_clip_contrastive away from the untrained state, against fp64 -- the cases, references, error figure and gate of tests/contrastive_cases.py
(e <= 4 max(yardstick, 2^-24); tests/test_contrastive_cases_cpu.py shows on the CPU that the downstream gates reject six restated kernel bugs, the kernel's
earlier log-sum-exp among them).  Every figure is printed next to its yardstick and gate (`pytest -s`); the largest are recorded in the docstring of
tests/contrastive_cases.py.  Everything goes through the C ABI (_lib.ContrastiveArgs): optional outputs can be NULL, img / txt are column slices of wider
buffers (ldi, ldt > P).

Two stages.  The forward stage (image_embeds, text_embeds, logits_per_text) is compared with the fp64 forward of the inputs.  The downstream stage (loss,
d_logit_scale, d_img, d_txt) is compared with the fp64 function of the tensors the call RETURNED: the f32 rounding of the logits themselves, an ulp of 100 at
the ceiling of logit_scale, is as large as the error the stage is gated on and would hide it.  The whole call is held by a bound that follows from the two:
the L1 norm of d loss / d S is at most 2, so |loss - loss64| <= gate(loss) |loss64| + 2 max |S - S64|.

Shapes, as read from csrc/contrastive.hip: B = 2 .. 5 around the contraction padding to 4 (L.Ki, L.Kt), B = 255, 256, 257, 513 around the 256-thread loops of
lse_kernel / ds_kernel / loss_final_kernel, P = 4, 64, 68, 768 around the 64-lane loops of the normalise kernels."""
import ctypes as C

import pytest
import torch

from tests import contrastive_cases as CC

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
MEASURED = {}
OUTPUTS = ("image_embeds", "text_embeds", "logits_per_text", "logits_per_image", "loss", "d_logit_scale", "d_img", "d_txt")
EXACT = ("image_embeds", "text_embeds", "logits_per_text", "logits_per_image", "loss", "d_logit_scale")


@pytest.fixture(scope="module")
def L():
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    yield _lib
    print("\n[measured] largest kernel/yardstick pairs: " + "  ".join(f"{k} {e:.1e}/{y:.1e}" for k, (e, y) in sorted(MEASURED.items())))


def _slice(x, pad, off):
    """x as columns off .. off + P of a wider device buffer."""
    wide = torch.full((x.shape[0], x.shape[1] + pad), 3.0, device="cuda")
    wide[:, off:off + x.shape[1]] = x.cuda()
    return wide, wide[:, off:off + x.shape[1]]


def _call(L, img, txt, ls, g=1.0, want_loss=True, null=()):
    """One gg_clip_contrastive call; CPU tensors by name of every output requested (``null``: outputs passed as NULL)."""
    (Bi, P), Bt = img.shape, txt.shape[0]
    wi, vi = _slice(img, 12, 4)
    wt, vt = _slice(txt, 8, 8)
    lst = torch.tensor([ls], dtype=torch.float32, device="cuda")
    shapes = dict(image_embeds=(Bi, P), text_embeds=(Bt, P), logits_per_text=(Bt, Bi), logits_per_image=(Bi, Bt))
    if want_loss:
        shapes.update(loss=(1,), d_logit_scale=(1,), d_img=(Bi, P), d_txt=(Bt, P))
    out = {k: torch.full(s, SENTINEL, device="cuda") for k, s in shapes.items() if k not in null}
    nscr = L.lib().gg_clip_contrastive_scratch_floats(Bi, Bt, P)
    assert nscr > 0
    scratch = torch.full((nscr,), SENTINEL, device="cuda")
    a = L.ContrastiveArgs()
    a.img, a.ldi, a.txt, a.ldt, a.Bi, a.Bt, a.P, a.logit_scale = vi.data_ptr(), wi.stride(0), vt.data_ptr(), wt.stride(0), Bi, Bt, P, L.ptr(lst)
    a.img_n, a.txt_n, a.logits_per_text, a.logits_per_image = (L.ptr(out.get(k)) for k in ("image_embeds", "text_embeds", "logits_per_text", "logits_per_image"))
    a.want_loss, a.d_loss_scale, a.scratch = int(want_loss), g, L.ptr(scratch)
    if want_loss:
        a.loss, a.d_logit_scale, a.d_img, a.d_txt = (L.ptr(out.get(k)) for k in ("loss", "d_logit_scale", "d_img", "d_txt"))
    L.check(L.lib().gg_clip_contrastive(C.byref(a), L.stream()), "gg_clip_contrastive")
    torch.cuda.synchronize()
    assert bool((wi[:, :4] == 3.0).all()) and bool((wi[:, 4 + P:] == 3.0).all()) and bool((wt[:, :8] == 3.0).all())
    return {k: (v.cpu().reshape(()) if v.numel() == 1 and len(shapes[k]) == 1 else v.cpu()) for k, v in out.items()}


def _same_bits(a, b, keys=None):
    """Names of the outputs of two calls that differ in any bit."""
    return [k for k in (a if keys is None else keys) if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]


def _twice(L, *args, **kw):
    """Every case is called twice and must return the same bits."""
    r, r2 = _call(L, *args, **kw), _call(L, *args, **kw)
    assert not _same_bits(r, r2), ("two calls differ", _same_bits(r, r2))
    return r


def _transposed(r):
    return torch.equal(r["logits_per_image"].view(torch.int32), r["logits_per_text"].t().contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------- the two stages and the whole call
@pytest.mark.parametrize("B,P", CC.shapes())
@pytest.mark.parametrize("kind", CC.KINDS)
def test_forward_and_downstream_stage(L, kind, B, P):
    """Each logit_scale and each d_loss_scale: the forward stage against fp64 of the inputs, the downstream stage against fp64 of the returned tensors, the
    derived whole-call bound on the loss, logits_per_image the exact transpose, two calls the same bits."""
    img, txt = CC.inputs(kind, B, P)
    bad = []
    for ls in CC.LOGIT_SCALES:
        f64 = CC.forward(img, txt, ls, CC.F64)
        loss64 = float(CC.clip_loss(f64["logits_per_text"]))
        first = None
        for g in CC.LOSS_SCALES:
            name = CC.case_name(kind, B, P, ls, g)
            r = _twice(L, img, txt, ls, g)
            assert _transposed(r), name
            if first is None:
                first = r
                bad += [(name,) + m for m in CC.check_forward(img, txt, ls, r, CC.case_name(kind, B, P, ls), collect=MEASURED)]
            assert not _same_bits(first, r, CC.FORWARD_TENSORS + ("loss",)), name           # d_loss_scale touches the gradients alone
            if CC.left_out(kind, B, ls):
                continue
            S, I, T = r["logits_per_text"], r["image_embeds"], r["text_embeds"]
            misses, gates = CC.check_downstream(S, I, T, img, txt, ls, g, r, name, collect=MEASURED)
            bad += [(name,) + m for m in misses]
            e2e, bound = abs(float(r["loss"]) - loss64), gates["loss"] * abs(loss64) + 2.0 * float((S.double() - f64["logits_per_text"]).abs().max())
            print(f"[whole call {name}] |loss - loss64| {e2e:.2e}, bound {bound:.2e}")
            if not e2e <= bound:
                bad.append((name, "whole-call loss", e2e, bound))
    assert not bad, bad


# ------------------------------------------------------------------------------------------- scale invariance
@pytest.mark.parametrize("B,P", [(5, 64), (257, 68)])
@pytest.mark.parametrize("kind", CC.KINDS)
def test_row_scales_of_two_to_the_forty_change_no_bit(L, kind, B, P):
    """Row r of img times 2^(+-40), of txt times 2^(-+40): a power of two commutes with every operation of the normalise kernels (2^80 |x|^2 P stays in range), so
    the normalised rows, both logit matrices, the loss and d_logit_scale keep their bits, and d_img / d_txt are the twin's rows times the inverse factor."""
    sc = CC.row_scales(B)
    for ls in (2.6592, 4.6052):
        twin = _twice(L, *CC.inputs(kind, B, P), ls, 0.5)
        r = _twice(L, *CC.inputs(kind, B, P, scaled=True), ls, 0.5)
        assert not _same_bits(twin, r, EXACT), (kind, B, P, ls, _same_bits(twin, r, EXACT))
        assert torch.equal(r["d_img"], twin["d_img"] / sc) and torch.equal(r["d_txt"], twin["d_txt"] * sc), (kind, B, P, ls)
        assert float(twin["d_img"].abs().max()) > 0.0 and bool(torch.isfinite(r["d_img"]).all()) and bool(torch.isfinite(r["d_txt"]).all())


# ------------------------------------------------------------------------------------------- optional outputs
NULLS = (("d_img",), ("d_txt",), ("d_img", "d_txt"), ("d_logit_scale",), ("logits_per_image",))


@pytest.mark.parametrize("B,P", [(5, 64), (6, 4), (257, 68)])
def test_every_optional_output_alone(L, B, P):
    """d_img, d_txt, both, d_logit_scale, logits_per_image passed as NULL one at a time: what is still requested keeps the bits of the full call (without a
    gradient the transposed copies and the contraction padding are not built: the launch sizes change)."""
    img, txt = CC.inputs("aligned", B, P)
    full = _twice(L, img, txt, 2.6592, 0.5)
    for null in NULLS:
        r = _twice(L, img, txt, 2.6592, 0.5, null=null)
        assert set(r) == set(OUTPUTS) - set(null)
        assert not _same_bits(full, r, r.keys()), (null, _same_bits(full, r, r.keys()))


# ------------------------------------------------------------------------------------------- rectangular forwards
@pytest.mark.parametrize("Bi,Bt", CC.RECT_SHAPES)
def test_rectangular_forward(L, Bi, Bt):
    bad = []
    for kind in ("plain", "cluster", "one_exact"):
        for P in (64, 68):
            for ls in CC.LOGIT_SCALES:
                img, txt = CC.inputs(kind, Bi, P, Bt=Bt)
                r = _twice(L, img, txt, ls, want_loss=False)
                assert r["logits_per_text"].shape == (Bt, Bi) and _transposed(r)
                bad += CC.check_forward(img, txt, ls, r, f"{kind} Bi={Bi} Bt={Bt} P={P} ls={ls:g}", "rectangular", collect=MEASURED)
    assert not bad, bad


# ------------------------------------------------------------------------------------------- NaN and zero rows
@pytest.mark.parametrize("B,P", [(5, 64), (257, 68)])
@pytest.mark.parametrize("kind", CC.EDGE_KINDS)
def test_a_nan_or_zero_image_row(L, kind, B, P):
    """img[1] all NaN or all 0: the loss is not finite, the other rows of image_embeds are finite and within the gate, and every output is non-finite exactly
    where the fp64 reference is."""
    img, txt = CC.inputs(kind, B, P)
    ls, g, name = 2.6592, 0.5, CC.case_name(kind, B, P, 2.6592, 0.5)
    r = _twice(L, img, txt, ls, g)
    others = [i for i in range(B) if i != 1]
    assert not bool(torch.isfinite(r["loss"])) and bool(torch.isfinite(r["image_embeds"][others]).all()) and bool(torch.isfinite(r["text_embeds"]).all())
    assert not CC.check_forward(img, txt, ls, r, name, "edge rows", rows=others)
    assert not CC.check_forward(img, txt, ls, r, name, "edge pattern") and _transposed(r)
    assert not CC.check_downstream(r["logits_per_text"], r["image_embeds"], r["text_embeds"], img, txt, ls, g, r, name, "edge downstream")[0]
    ref = CC.forward(img, txt, ls)
    for k in CC.FORWARD_TENSORS:
        assert torch.equal(torch.isfinite(r[k]), torch.isfinite(ref[k])), k
    assert all(not bool(torch.isfinite(r[k]).any()) for k in CC.DOWNSTREAM_TENSORS)


@pytest.mark.parametrize("kind", CC.EDGE_KINDS)
def test_a_nan_or_zero_image_row_writes_nothing_outside_the_outputs(kind):
    """The same call in guarded buffers (tests/guards.py), scratch of exactly gg_clip_contrastive_scratch_floats: bands, row padding and inputs unchanged under
    both fills, the outputs the same bits under both."""
    from tests.test_gpu_guards import run_guarded
    B, P = 5, 64
    img, txt = CC.inputs(kind, B, P)
    ref = CC.forward(img, txt, 2.6592)

    def call(S, L):
        a = L.ContrastiveArgs()
        ii, ti, li = S.inp("img", img, ld=P + 12, col_off=4), S.inp("txt", txt, ld=P + 8, col_off=8), S.inp("logit_scale", torch.tensor([2.6592]))
        a.img, a.ldi, a.txt, a.ldt, a.Bi, a.Bt, a.P, a.logit_scale = ii.ptr, ii.ld, ti.ptr, ti.ld, B, B, P, li.ptr
        shapes = dict(img_n=(B, P), txt_n=(B, P), logits_per_text=(B, B), logits_per_image=(B, B), loss=(1, 1), d_logit_scale=(1, 1), d_img=(B, P), d_txt=(B, P))
        outs = {k: S.out(k, *s, torch.float32, written=k == "txt_n") for k, s in shapes.items()}           # the others hold NaN by right
        for k, o in outs.items():
            setattr(a, k, o.ptr)
        a.want_loss, a.d_loss_scale = 1, 0.5
        a.scratch = S.scratch("scratch", 4 * L.lib().gg_clip_contrastive_scratch_floats(B, B, P), row_bytes=4 * max(P, B)).ptr
        L.check(L.lib().gg_clip_contrastive(C.byref(a), L.stream()), "gg_clip_contrastive")

        def check(val):
            assert torch.equal(torch.isfinite(val["img_n"]), torch.isfinite(ref["image_embeds"])) and not bool(torch.isfinite(val["loss"]).any())
            assert torch.equal(torch.isfinite(val["logits_per_text"]), torch.isfinite(ref["logits_per_text"]))
        return outs, check
    run_guarded(call)
