"""gg_cls_head (csrc/cls_head.hip, include/gg_cls.h) against torch fp64 ``log_softmax`` / ``F.cross_entropy`` on the CPU, inside guard bands.

Gates.  preds and rank must EQUAL the fp64 result (the rows are tie-free, asserted).  For the loss rows, the mean loss and dlogits the gate is not a constant:
torch's own f32 ``F.cross_entropy`` (CPU) is measured against fp64 on the same inputs (max |error| over the tensor) and the kernel is allowed 4 x that --
its reduction order differs, its arithmetic does not.  On rows of one to six classes torch's f32 result can equal the rounded fp64 result by luck
(measured error exactly 0); no f32 result can be asked to be closer than its own rounding, so the measured error is floored at half an f32 ulp of the
tensor's largest reference magnitude (2^-24 max|ref|) before the factor 4.  bf16 dlogits get 2^-8 |ref| per element on top (one bf16 rounding is 2^-9).
Every figure is printed next to its gate.

Every tensor the call is given lives between guard bands (tests/guards.py) under two fills; the logical outputs of the two runs must be bit-identical
(the same call twice, and no dependence on bytes outside the inputs)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import guards as G

pytestmark = pytest.mark.gpu
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64

# the issue's shapes, then every size at which the launch takes another kernel (64 | 65, 256 | 257, 1024 | 1025 classes; 4 rows per workgroup)
SHAPES = [(1, 1), (3, 2), (2, 5), (2, 6), (64, 65), (65, 63), (5, 211), (3, 1000), (2, 4097), (1, 65536),
          (5, 64), (6, 256), (7, 257), (3, 1024), (3, 1025)]


def _L():
    from geoguessr_ai_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _case(N, Cn):
    """Tie-free logits ~ N(0, 3) (row 0 shifted by +80, the last row of N >= 2 by -80), labels, and the fp64 results; computed once, never modified."""
    g = torch.Generator().manual_seed(1000 * N + Cn)
    rows = []
    for n in range(N):
        shift = 80.0 if n == 0 else (-80.0 if n == N - 1 else 0.0)
        v = torch.unique(torch.randn(max(3 * Cn, 16), generator=g) * 3.0 + shift)      # distinct AFTER the shift (f32 spacing at 80 is 7.6e-6)
        assert v.numel() >= Cn
        rows.append(v[torch.randperm(v.numel(), generator=g)[:Cn]])
    logits = torch.stack(rows).contiguous()
    for r in logits:
        assert torch.unique(r).numel() == Cn                                          # tie-free rows
    labels = torch.randint(0, Cn, (N,), generator=g)
    labels[0] = int(logits[0].argmax())                                               # one certain top-1 hit
    z64 = logits.double()
    rows64 = F.cross_entropy(z64, labels, reduction="none")
    soft64 = torch.softmax(z64, 1)
    soft64[torch.arange(N), labels] -= 1.0
    zl = z64.gather(1, labels.view(-1, 1))
    rank = (z64 > zl).sum(1).to(I32)
    # torch's own f32 error on the same inputs
    rows32 = F.cross_entropy(logits, labels, reduction="none")
    mean32 = F.cross_entropy(logits, labels)
    zg = logits.clone().requires_grad_(True)
    F.cross_entropy(zg, labels, reduction="sum").backward()
    err = dict(rows=float((rows32.double() - rows64).abs().max()), mean=float((mean32.double() - rows64.mean()).abs()),
               dl=float((zg.grad.double() - soft64).abs().max()))
    return dict(logits=logits, labels=labels, rows=rows64, mean=rows64.mean(), dl=soft64, rank=rank, preds=z64.argmax(1), err=err)


def _gate(measured, ref):
    return 4.0 * max(measured, 2.0 ** -24 * float(ref.abs().max()))


def _call(fill, logits, labels, *, dl_dtype=F32, gs=1.0, ldl=None, ldd=None, upstream=None, finite=True, edit=None):
    """One guarded call.  Returns (rc, guard set, outputs by name)."""
    L = _L()
    N, Cn = logits.shape
    ldd = Cn if ldd is None else ldd
    gset = G.GuardSet(fill)
    gl = gset.inp("logits", logits, ld=ldl)
    glab = gset.inp("labels", labels)
    gup = gset.inp("upstream", upstream) if upstream is not None else None
    o = dict(loss_rows=gset.out("loss_rows", 1, N, F32, written=finite), loss=gset.out("loss", 1, 1, F32, written=finite),
             dlogits=gset.out("dlogits", N, ldd, dl_dtype, written=finite), rank=gset.out("rank", 1, N, I32), preds=gset.out("preds", 1, N, I64))
    a = L.ClsHeadArgs()
    a.logits, a.ldl, a.N, a.C, a.labels, a.grad_scale = gl.ptr, gl.ld, N, Cn, glab.ptr, gs
    a.upstream = gup.ptr if gup is not None else None
    a.loss_rows, a.loss, a.dlogits, a.ldd, a.dlogits_f32 = o["loss_rows"].ptr, o["loss"].ptr, o["dlogits"].ptr, ldd, int(dl_dtype == F32)
    a.rank, a.preds = o["rank"].ptr, o["preds"].ptr
    if edit is not None:
        edit(a)
    rc = L.lib().gg_cls_head(C.byref(a), L.stream())
    torch.cuda.synchronize()
    return rc, gset, o


def _check(N, Cn, dl_dtype, gs, ldl=None, ldd=None, upstream=None):
    c = _case(N, Cn)
    up = None if upstream is None else torch.tensor([upstream], dtype=F32)
    runs = []
    for fill in ("nan", "finite"):
        rc, gset, o = _call(fill, c["logits"], c["labels"], dl_dtype=dl_dtype, gs=gs, ldl=ldl, ldd=ldd, upstream=up)
        assert rc == 0, _L().lib().gg_last_error()
        gset.check()
        runs.append({k: v.view.clone() for k, v in o.items()})
    for k in runs[0]:
        G.assert_bit_identical(runs[0][k], runs[1][k], f"gg_cls_head {k} N={N} C={Cn}")
    r = {k: v.cpu() for k, v in runs[0].items()}
    assert torch.equal(r["preds"].view(-1), c["preds"]) and torch.equal(r["rank"].view(-1), c["rank"])
    scale = gs * (1.0 if upstream is None else upstream)
    dl_ref = c["dl"] * scale
    e_rows = float((r["loss_rows"].view(-1).double() - c["rows"]).abs().max())
    e_mean = float((r["loss"].view(()).double() - c["mean"]).abs())
    dl = r["dlogits"].double()
    d = (dl[:, :Cn] - dl_ref).abs()
    g_rows, g_mean, g_dl = _gate(c["err"]["rows"], c["rows"]), _gate(c["err"]["mean"], c["mean"]), _gate(c["err"]["dl"] * abs(scale), dl_ref)
    slack = (2.0 ** -8) * dl_ref.abs() if dl_dtype == BF16 else torch.zeros_like(dl_ref)
    print(f"\n[cls_head N={N} C={Cn} {str(dl_dtype)[6:]} scale={scale:.4g}] loss rows err {e_rows:.3e} (torch f32 {c['err']['rows']:.3e}, gate {g_rows:.3e}) | "
          f"mean err {e_mean:.3e} (torch f32 {c['err']['mean']:.3e}, gate {g_mean:.3e}) | dlogits err {float((d - slack).max()):.3e} beyond the bf16 term "
          f"(torch f32 {c['err']['dl'] * abs(scale):.3e}, gate {g_dl:.3e})")
    assert e_rows <= g_rows and e_mean <= g_mean
    assert bool((d <= g_dl + slack).all()), float((d - slack).max())
    assert float(dl[:, Cn:].abs().sum()) == 0.0 and not bool(torch.isnan(dl).any())        # pad columns exactly zero
    return r


@pytest.mark.parametrize("dl_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,Cn", SHAPES)
def test_cls_head_matches_fp64(N, Cn, dl_dtype):
    _check(N, Cn, dl_dtype, 1.0)
    _check(N, Cn, dl_dtype, 1.0 / N)


@pytest.mark.parametrize("dl_dtype", [F32, BF16], ids=["f32", "bf16"])
def test_cls_head_padded_rows_and_upstream_scalar(dl_dtype):
    _check(5, 211, dl_dtype, 1.0 / 5, ldl=211 + 3)                    # logits as a column slice of a wider buffer
    _check(5, 211, dl_dtype, 1.0 / 5, ldd=211 + 5)                    # padded gradient rows: columns C..ldd written as zero
    _check(2, 4097, dl_dtype, 1.0, ldl=4097 + 3, ldd=4097 + 5)        # the looping kernel
    _check(3, 2, dl_dtype, 1.0 / 3, ldl=5, ldd=7)
    _check(7, 257, dl_dtype, 1.0 / 7, upstream=0.37)                  # the incoming gradient of the loss, multiplied in on the device
    _check(2, 4097, dl_dtype, 0.5, upstream=-2.5)


@pytest.mark.parametrize("N,Cn", [(5, 211), (6, 64), (3, 4097)])
def test_cls_head_out_of_range_label_poisons_only_its_row(N, Cn):
    c = _case(N, Cn)
    labels = c["labels"].clone()
    labels[1], labels[N - 1] = Cn, -1                                 # one past the end, negative
    bad = torch.zeros(N, dtype=torch.bool)
    bad[1] = bad[N - 1] = True
    outs = []
    for fill in ("nan", "finite"):
        rc, gset, o = _call(fill, c["logits"], labels, gs=1.0 / N, ldd=Cn + 5, finite=False)
        assert rc == 0
        gset.check()
        outs.append({k: v.view.clone().cpu() for k, v in o.items()})
    r = outs[0]
    for k in ("rank", "preds"):
        G.assert_bit_identical(outs[0][k], outs[1][k], k)
    rows, dl, rank = r["loss_rows"].view(-1), r["dlogits"], r["rank"].view(-1)
    assert bool(torch.isnan(rows[bad]).all()) and bool(torch.isnan(r["loss"]).all()) and bool(torch.isnan(dl[bad][:, :Cn]).all())
    assert rank[bad].tolist() == [Cn, Cn] and torch.equal(r["preds"].view(-1), c["preds"])
    assert float(dl[:, Cn:].abs().sum()) == 0.0
    ok = ~bad
    assert torch.equal(rank[ok], c["rank"][ok])
    assert float((rows[ok].double() - c["rows"][ok]).abs().max()) <= _gate(c["err"]["rows"], c["rows"])
    assert float((dl[ok][:, :Cn].double() - c["dl"][ok] / N).abs().max()) <= _gate(c["err"]["dl"] / N, c["dl"] / N)


def test_cls_head_bad_arguments_write_nothing():
    L = _L()
    c = _case(5, 211)
    host_f = torch.zeros(5 * 211, dtype=F32)
    host_i = torch.zeros(5, dtype=I64)

    def setter(**kw):
        def edit(a):
            for k, v in kw.items():
                setattr(a, k, v)
        return edit
    cases = [("N == 0", setter(N=0), b"N=0"), ("C < 1", setter(C=0), b"C=0"), ("negative C", setter(C=-3), b"C=-3"), ("ldl < C", setter(ldl=210), b"ldl=210 < C=211"),
             ("ldd < C", setter(ldd=100), b"ldd=100 < C=211"), ("NULL logits", setter(logits=None), b"null logits"), ("NULL labels", setter(labels=None), b"null logits / labels"),
             ("loss without loss_rows", setter(loss_rows=None), b"loss_rows"),
             ("host logits", setter(logits=host_f.data_ptr()), b"logits is"), ("host labels", setter(labels=host_i.data_ptr()), b"labels is"),
             ("host dlogits", setter(dlogits=host_f.data_ptr()), b"dlogits is"), ("host rank", setter(rank=host_i.data_ptr()), b"rank is")]
    for what, edit, msg in cases:
        rc, gset, o = _call("finite", c["logits"], c["labels"], edit=edit)
        err = L.lib().gg_last_error()
        assert rc != 0 and msg in err, (what, rc, err)
        for t in gset.tensors:                                        # nothing launched: not one byte of any buffer changed
            assert not any(t.regions().values()), (what, t.name, t.regions())
    assert float(host_f.abs().sum()) == 0.0 and int(host_i.abs().sum()) == 0
    with pytest.raises(L.GgError):                                    # the tensor-level wrapper refuses a host tensor by message
        from geoguessr_ai_amd import ops
        ops.cls_head(c["logits"], c["labels"].cuda())


def test_cls_head_profiler_record_and_wrapper():
    """ops.cls_head returns what the raw call does; the launch carries a head-category GG_PROF record with its algorithmic bytes."""
    L = _L()
    from geoguessr_ai_amd import ops
    lib = L.lib()
    c = _case(5, 211)
    lib.gg_prof_reset(); lib.gg_prof_enable(1)
    r = ops.cls_head(c["logits"].cuda(), c["labels"].cuda(), want_dlogits=True)
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    cat, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    recs = []
    for i in range(lib.gg_prof_count()):
        L.check(lib.gg_prof_record(i, C.byref(cat), C.byref(ms), C.byref(fl), C.byref(by)), "gg_prof_record")
        recs.append((cat.value, by.value))
    lib.gg_prof_reset()
    ldd = 216
    assert recs == [(4, 5 * 211 * 4.0 + 5 * 8.0 + 5 * ldd * 4.0 + 5 * (4.0 + 4.0 + 8.0))], recs        # GG_CAT_HEAD
    assert r["dlogits"].shape == (5, ldd) and torch.equal(r["rank"].cpu(), c["rank"]) and torch.equal(r["preds"].cpu(), c["preds"])
    assert abs(float(r["loss"]) - float(c["mean"])) <= _gate(c["err"]["mean"], c["mean"])
