"""gg_geo_head, gg_haversine_matrix, gg_adamw_step and gg_grad_sq_norm at their edges, against fp64 -- the cases, references, error figure and gate of
tests/geo_cases.py (e <= 4 max(yardstick, half an ulp of the compared type); tests/test_geo_cases_cpu.py shows on the CPU that the gates reject six restated
kernel bugs).  Every figure is printed next to its yardstick (`pytest -s`); the largest are recorded in the docstring of tests/geo_cases.py.

Head dispatch, as read from gg_geo_head: ceil(K / 256) <= 4 -> geo_head_kernel<4> (K <= 1024), <= 16 -> <16> (K <= 4096), <= 50 -> <50> (K <= 12800), else <64>
(K <= 16384); beyond that the call is refused.  The sweep sits on both sides of every boundary and on K = 1, 5, 255, 256, 257 inside the first kernel.
mean_f32_kernel strides over the loss rows in steps of 256 (batch cases N = 257, 1000); haversine_matrix_kernel grid-strides beyond 16384 x 256 elements
(400 x 12647); adamw_kernel beyond 8192 x 256 x 4 floats (n = 8388608 + 4099: grid stride and scalar tail in one call); the gradient norm takes 1024 blocks x 4096
elements (n = 4194304 + 4099).

Index results are exact: top-k indices (the kernel compares the f32 logits themselves, so every rank is decided, ties towards the lower index), preds, llh
(a gather), and ``nearest`` under the 0.25 km rule of geo_cases.nearest_rule."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import geo_cases as GC

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
MEASURED = {}


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as o
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    yield o
    print("\n[measured] largest kernel/yardstick pairs: " + "  ".join(f"{k} {e:.1e}/{y:.1e}" for k, (e, y) in sorted(MEASURED.items())))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _head(ops, c, mode, dl="f32", logits=None, labels=True, want_nearest=True, labels_clf=None, **over):
    """One ops.geo_head call on the case's inputs; numpy results by name, dlogits cut to [N, K] with the pad columns under "pad"."""
    kw = dict(c["kw"], **over)
    z = c["logits"] if logits is None else logits
    lab = _dev(c["labels"]) if labels is True else (None if labels is None else _dev(labels))
    clf = _dev(c["ref"]["labels_clf"] if labels_clf is None else labels_clf) if mode == 2 else None
    r = ops.geo_head(_dev(z), _dev(c["cent"]), labels=lab, labels_clf=clf, mode=mode, want_dlogits=mode != 0, dlogits_f32=dl == "f32",
                     want_nearest=want_nearest and lab is not None, **kw)
    torch.cuda.synchronize()
    got = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy() for k, v in r.items()}
    if "dlogits" in got:
        assert r["dlogits"].dtype == (torch.float32 if dl == "f32" else torch.bfloat16)
        got["pad"], got["dlogits"] = got["dlogits"][:, c["K"]:], got["dlogits"][:, :c["K"]]
    got["loss"] = got["loss"].reshape(())
    return got


def _assert_head(c, got, mode, dl, label):
    bad = GC.check(c, got if mode else dict(got, loss_rows=None, loss=None), mode, dl, label=label, collect=MEASURED)
    bad += GC.exact_misses(c, got)
    if "nearest" in got:
        bad += GC.nearest_misses(c, got["nearest"])
    if "pad" in got:
        assert not got["pad"].any(), "dlogits columns K..ldd must be zero"
    assert not bad, (c["name"], mode, dl, bad)


# ------------------------------------------------------------------------------------------- the head
@pytest.mark.parametrize("K", GC.SWEEP_K)
def test_dispatch_sweep(ops, K):
    """Every kernel width and both sides of every dispatch boundary: N = 8, one label class per row, modes 0, 1, 2, dlogits f32 and bf16; every output against
    fp64, the pad columns K..ldd zero."""
    c = GC.sweep_case(K)
    _assert_head(c, _head(ops, c, 0), 0, "f32", "sweep")
    for mode in (1, 2):
        for dl in ("f32", "bf16"):
            _assert_head(c, _head(ops, c, mode, dl), mode, dl, f"sweep {dl}")


def _raw_head(c, K, num_candidates, N=None):
    """gg_geo_head through ctypes on sentinel-filled outputs: (return code, message, {name: output tensor})."""
    from geoguessr_ai_amd import _lib as L
    N = c["N"] if N is None else N
    ld = (K + 7) // 8 * 8
    logits = torch.zeros(N, K, device="cuda")
    cent = torch.zeros(K, 2, device="cuda")
    out = dict(loss_rows=torch.full((N,), SENTINEL, device="cuda"), loss=torch.full((1,), SENTINEL, device="cuda"),
               dlogits=torch.full((N, ld), SENTINEL, device="cuda"), preds=torch.full((N,), -7, dtype=torch.int64, device="cuda"),
               llh=torch.full((N, 2), SENTINEL, device="cuda"), topk_vals=torch.full((N, num_candidates), SENTINEL, device="cuda"),
               topk_idx=torch.full((N, num_candidates), -7, dtype=torch.int64, device="cuda"), nearest=torch.full((N,), -7, dtype=torch.int64, device="cuda"))
    a = L.GeoHeadArgs()
    a.logits, a.ldl, a.N, a.K = L.ptr(logits), K, N, K
    a.labels, a.centroids, a.mode, a.smoothing_km, a.grad_scale = L.ptr(_dev(c["labels"][:N])), L.ptr(cent), 1, 65.0, 1.0 / N
    a.loss_rows, a.loss, a.dlogits, a.ldd, a.dlogits_f32 = L.ptr(out["loss_rows"]), L.ptr(out["loss"]), L.ptr(out["dlogits"]), ld, 1
    a.preds, a.llh, a.topk_vals, a.topk_idx, a.num_candidates, a.nearest = (L.ptr(out["preds"]), L.ptr(out["llh"]), L.ptr(out["topk_vals"]), L.ptr(out["topk_idx"]),
                                                                            num_candidates, L.ptr(out["nearest"]))
    rc = L.lib().gg_geo_head(C.byref(a), L.stream())
    torch.cuda.synchronize()
    return rc, L.lib().gg_last_error().decode(errors="replace"), out


def _untouched(out):
    return all(bool((t == (SENTINEL if t.is_floating_point() else -7)).all()) for t in out.values())


def test_k_beyond_the_widest_kernel_is_refused_and_writes_nothing(ops):
    from geoguessr_ai_amd import _lib as L
    c = GC.sweep_case(5)
    rc, msg, out = _raw_head(c, 16385, 5)
    assert rc != 0 and "16385" in msg and _untouched(out), (rc, msg)
    with pytest.raises(L.GgError, match="unsupported"):
        ops.geo_head(torch.zeros(2, 16385, device="cuda"), torch.zeros(16385, 2, device="cuda"))


def test_more_candidates_than_classes_is_refused_and_writes_nothing(ops):
    from geoguessr_ai_amd import _lib as L
    c = GC.sweep_case(5)
    rc, msg, out = _raw_head(c, 4, 5)
    assert rc != 0 and "num_candidates=5" in msg and "K=4" in msg and _untouched(out), (rc, msg)
    with pytest.raises(L.GgError, match="num_candidates"):
        ops.geo_head(torch.zeros(2, 3, device="cuda"), torch.zeros(3, 2, device="cuda"), num_candidates=4)
    rc, msg, out = _raw_head(c, 5, 5)          # K == num_candidates is served
    assert rc == 0 and out["topk_idx"].cpu().tolist() == [[0, 1, 2, 3, 4]] * c["N"], (rc, msg)


@pytest.mark.parametrize("logit_cls", GC.LOGIT_CLASSES)
@pytest.mark.parametrize("K", GC.COND_K)
def test_conditioning(ops, K, logit_cls):
    """Every label class (one per row) x every logit class, soft CE and hard CE on the fp64 nearest centroid, dlogits f32 and bf16.  On ``masked`` the soft loss
    is non-finite in fp64 and f32 alike and must be here; on ``ties`` the ranks resolve to the lower index (exact_misses)."""
    c = GC.cond_case(K, logit_cls)
    for mode in (1, 2):
        for dl in ("f32", "bf16"):
            got = _head(ops, c, mode, dl)
            _assert_head(c, got, mode, dl, f"cond {dl}")
            if logit_cls == "masked" and mode == 1:
                assert not np.isfinite(got["loss_rows"]).any() and not np.isfinite(got["loss"])
    if logit_cls == "ties":
        got = _head(ops, c, 0, num_candidates=7)
        assert (got["topk_idx"] == np.asarray(GC.TIE_AT + GC.TIE_NEXT)).all()


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_nan_logits_rank_first_and_stay_in_their_row(ops, mode):
    """Row 2 all NaN, row 5 one NaN at column 700: NaN ranks above every number, lower index first (torch.topk / argmax).  The all-NaN row gives preds 0,
    topk_idx 0..4, llh = centroids[0]; both rows have NaN probabilities and (modes 1, 2) NaN loss rows, mean loss and gradient rows; every other row is gated
    against fp64 as usual.  No index leaves [0, K)."""
    K = 1025
    c = GC.cond_case(K, "plain")
    z = c["logits"].copy()
    z[2] = np.nan
    z[5, 700] = np.nan
    got = _head(ops, c, mode, logits=z)
    nan_rows, ref = [2, 5], c["ref"]
    assert got["topk_idx"].min() >= 0 and got["topk_idx"].max() < K and got["preds"].min() >= 0 and got["preds"].max() < K
    assert got["topk_idx"][2].tolist() == [0, 1, 2, 3, 4] and got["preds"][2] == 0 and (got["llh"][2] == c["cent"][0]).all()
    rest = [int(j) for j in GC.rank_order(c["logits"][5:6])[0] if j != 700][:4]
    assert got["topk_idx"][5].tolist() == [700] + rest and got["preds"][5] == 700 and (got["llh"][5] == c["cent"][700]).all()
    assert np.isnan(got["topk_vals"][nan_rows]).all()
    if mode:
        assert np.isnan(got["loss_rows"][nan_rows]).all() and np.isnan(got["loss"]) and np.isnan(got["dlogits"][nan_rows]).all()
        assert not got["pad"].any()
    # the other rows: the NaN rows take the reference's values, the mean is checked on the row losses
    patched = dict(got)
    for name, rname in GC.tensors_of(mode).items():
        if name == "loss":
            patched[name] = None
            continue
        patched[name] = got[name].copy()
        patched[name][nan_rows] = ref[rname][nan_rows]
    for name in ("topk_idx", "preds", "llh"):
        patched[name] = got[name].copy()
        patched[name][nan_rows] = ref[name][nan_rows]
    _assert_head(c, patched, mode, "f32", "nan rows")


def test_fewer_finite_logits_than_candidates(ops):
    """A row with two finite logits among K = 5 and five candidates: the -inf entries rank after them by index, each once (a stable sort; a retired winner must not
    come back as the lowest-index -inf)."""
    c = GC.sweep_case(5)
    z = c["logits"].copy()
    z[:, [0, 2, 4]] = -np.inf
    z[3] = -np.inf
    a = GC.adhoc_case(z, c["labels"], c["cent"], "K=5 mostly -inf", num_candidates=5)
    got = _head(ops, a, 0)
    assert got["topk_idx"][3].tolist() == [0, 1, 2, 3, 4]
    assert sorted(got["topk_idx"][0].tolist()) == [0, 1, 2, 3, 4] and got["topk_idx"][0].tolist()[2:] == [0, 2, 4]
    assert not GC.exact_misses(a, got), GC.exact_misses(a, got)


def test_signed_zeros_tie_and_infinities_rank_at_the_ends(ops):
    """-0 == +0 (the lower index wins whichever sign it has), +inf ranks above every number and below NaN, -inf last -- the order of a stable sort on the values."""
    c = GC.sweep_case(257)
    z = -np.abs(c["logits"]) - 1.0
    z[0, 9], z[0, 3] = 0.0, -0.0
    z[1, 9], z[1, 3] = -0.0, 0.0
    z[2, 200], z[2, 256], z[2, 0] = np.inf, np.nan, -np.inf
    got = _head(ops, c, 0, logits=z.astype(np.float32))
    assert got["topk_idx"][0, :2].tolist() == [3, 9] and got["topk_idx"][1, :2].tolist() == [3, 9]
    assert got["topk_idx"][2, :2].tolist() == [256, 200] and 0 not in got["topk_idx"][2]
    assert np.array_equal(got["topk_idx"], GC.rank_order(z.astype(np.float32))[:, :5]) and np.array_equal(got["preds"], got["topk_idx"][:, 0])


@pytest.mark.parametrize("i", range(len(GC.PARAM_CASES)))
def test_parameters(ops, i):
    """smoothing_km 10 and 300, grad_scale 0.37 (1 / N is every other case's), num_candidates 1 and 16 -- on peaked logits."""
    c = GC.param_case(i)
    for mode in (1, 2):
        for dl in ("f32", "bf16"):
            _assert_head(c, _head(ops, c, mode, dl), mode, dl, f"param {dl}")


def test_smoothing_falls_back_to_65_km_and_mode_0_needs_no_labels(ops):
    c = GC.param_case(3)       # peaked, 65 km, one candidate
    for s in (0.0, -3.0):
        _assert_head(c, _head(ops, c, 1, smoothing_km=s), 1, "f32", f"smoothing {s}")
    got = _head(ops, c, 0, labels=None)
    assert "nearest" not in got and float(got["loss"]) == 0.0
    _assert_head(c, got, 0, "f32", "mode 0, no labels")
    got = _head(ops, c, 0, want_nearest=True)
    assert "nearest" in got
    _assert_head(c, got, 0, "f32", "mode 0, labels and nearest")


@pytest.mark.parametrize("N", GC.BATCH_N)
def test_batch(ops, N):
    """N = 1, 257, 1000 at K = 300: the mean loss against the fp64 mean of the fp64 row losses (the strided mean_f32_kernel), and every row as usual."""
    c = GC.batch_case(N)
    for mode in (1, 2):
        _assert_head(c, _head(ops, c, mode), mode, "f32", "batch")


def test_nan_label_row_is_pinned(ops):
    """include/gg.h: a label with a NaN coordinate has no nearest centroid -- nearest = 2147483647, soft targets all 0, loss row 0, gradient row 0; a hard CE on that
    index is NaN.  The other rows are as without it."""
    c = GC.cond_case(1025, "plain")
    lab = c["labels"].copy()
    lab[4, 0] = np.nan
    got = _head(ops, c, 1, labels=lab)
    assert got["nearest"][4] == 2147483647 and got["loss_rows"][4] == 0.0 and not got["dlogits"][4].any() and not got["pad"].any()
    keep = [n for n in range(c["N"]) if n != 4]
    assert (got["nearest"][keep] == _head(ops, c, 1)["nearest"][keep]).all()
    patched = dict(got, loss=None, loss_rows=got["loss_rows"].copy(), dlogits=got["dlogits"].copy(), nearest=got["nearest"].copy())
    patched["loss_rows"][4], patched["dlogits"][4], patched["nearest"][4] = c["ref"]["loss_rows"][4], c["ref"]["dlogits"][4], c["ref"]["nearest"][4]
    _assert_head(c, patched, 1, "f32", "nan label")
    hard = _head(ops, c, 2, labels_clf=got["nearest"])
    assert np.isnan(hard["loss_rows"][4]) and np.isnan(hard["loss"]) and np.isnan(hard["dlogits"][4]).all() and np.isfinite(hard["dlogits"][keep]).all()


# ------------------------------------------------------------------------------------------- haversine matrix
@pytest.mark.parametrize("name", list(GC.haversine_pairs()))
def test_haversine_pairs(ops, name):
    """Each pair in a call of its own, so its figure is relative to its own distance.  The gate is the same everywhere; where the oracle is NaN (it has no clamp)
    it says nothing and the floor alone applies."""
    x, y = GC.haversine_pairs()[name]
    got = ops.haversine_matrix(_dev(x), _dev(y)).cpu().numpy()
    if name == "nan_coordinate":
        assert np.isnan(got).all()
    else:
        assert np.isfinite(got).all()
    if name == "identical":
        assert got[0, 0] == 0.0
    if name == "antipode":      # the documented clamp: finite and at most pi R, to the gate's four half-ulps (f32(pi) alone exceeds pi by 2.8e-8)
        assert got[0, 0] <= np.pi * GC.R_KM * (1 + GC.FACTOR * GC.FLOOR["f32"])
    assert not GC.haversine_check(x, y, got, name, collect=MEASURED if name in ("pole_to_pole", "1m_origin") else None)


def test_haversine_matrix_beyond_one_grid(ops):
    """N K = 400 x 12647 > 16384 x 256: the grid-stride loop repeats.  Labels cycle through every class."""
    cent = GC.centroids(12647)
    x = GC.make_labels(cent, GC.label_classes("each", 400), 400)
    got = ops.haversine_matrix(_dev(x), _dev(cent)).cpu().numpy()
    assert got.shape == (400, 12647) and np.isfinite(got).all() and got.max() <= np.pi * GC.R_KM * (1 + GC.FACTOR * GC.FLOOR["f32"])
    assert not GC.haversine_check(x, cent, got, "400 x 12647", collect=MEASURED)


# ------------------------------------------------------------------------------------------- AdamW
def _adamw_run(ops, c, pad=0):
    """The case's step sequence through ops.adamw_step on buffers with ``pad`` guard floats after the range; f32 arrays p, m, v and the guards."""
    n = c["n"]
    ext = lambda a: torch.cat([torch.from_numpy(a), torch.full((pad,), SENTINEL)]).cuda()
    p, m, v = ext(c["p0"]), ext(c["m0"]), ext(c["v0"])
    h = c["hyper"]
    for s, g in zip(c["steps"], c["grads"]):
        ops.adamw_step(p[:n], _dev(g), m[:n], v[:n], s, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], c["scale"])
    torch.cuda.synchronize()
    for t in (p, m, v):
        assert bool((t[n:] == SENTINEL).all()), "wrote past the range"
    return dict(p=p[:n].cpu().numpy(), m=m[:n].cpu().numpy(), v=v[:n].cpu().numpy())


@pytest.mark.parametrize("n", GC.ADAMW_SIZES[:-1])
def test_adamw_sizes_and_hyper_parameters(ops, n):
    """Steps 1..3 at every small size x (betas, eps, weight decay) x grad_scale; p, m, v and the update p - p0 after the sequence."""
    for hyper in range(len(GC.ADAMW_HYPER)):
        for scale in GC.ADAMW_SCALES:
            c = GC.adamw_case(n, hyper, scale)
            bad = GC.adamw_check(c, _adamw_run(ops, c, pad=5), collect=MEASURED)
            assert not bad, (c["name"], bad)


@pytest.mark.parametrize("scale", GC.ADAMW_SCALES)
@pytest.mark.parametrize("hyper", range(len(GC.ADAMW_HYPER)))
def test_adamw_beyond_one_grid(ops, hyper, scale):
    """n = 8388608 + 4099 > 8192 x 256 x 4: the grid-stride loop takes a second turn and the scalar tail follows it, in one call; every hyper-parameter set x
    every grad_scale, like the small sizes."""
    c = GC.adamw_case(GC.ADAMW_SIZES[-1], hyper, scale)
    bad = GC.adamw_check(c, _adamw_run(ops, c, pad=5), "large", collect=MEASURED)
    assert not bad, (c["name"], bad)


@pytest.mark.parametrize("step", (1000, 100000))
def test_adamw_late_steps(ops, step):
    """One step at a late step count from non-zero m and v: the bias corrections 1 - beta^step (computed in double, passed as float)."""
    for hyper in range(len(GC.ADAMW_HYPER)):
        c = GC.adamw_case(4099, hyper, 1.0 / 8.0, steps=(step,), seeded_state=True)
        bad = GC.adamw_check(c, _adamw_run(ops, c, pad=5), f"step {step}", collect=MEASURED)
        assert not bad, (c["name"], bad)


@pytest.mark.parametrize("grad_cls", GC.GRAD_CLASSES)
def test_adamw_gradient_classes(ops, grad_cls):
    """n = 4099.  ``zero``: m = v = 0, p changes by the decay only (fp64 gate).  ``mixed`` (1e-6 .. 1e3, both signs): fp64 gate.  ``tiny`` (1e-30: g^2 underflows
    f32, v stays 0) and ``huge`` (1e20: g^2 alone overflows f32; (1 - beta2) g g taken left to right stays finite, as torch's addcmul does): the f32 range is the
    point, fp64 does not have it, so torch.optim.AdamW's f32 result is the expected value -- within 4 half-ulps, non-finite elements identical."""
    c = GC.adamw_case(4099, grad_cls=grad_cls)
    got = _adamw_run(ops, c, pad=5)
    range_cls = grad_cls in ("tiny", "huge")
    bad = GC.adamw_check(c, got, grad_cls, against_yardstick=range_cls, collect=MEASURED)
    assert not bad, (c["name"], bad)
    if grad_cls == "zero":
        assert not got["m"].any() and not got["v"].any()
    if grad_cls == "tiny":
        assert not got["v"].any() and (got["m"] != 0).all()
    if grad_cls == "huge":
        assert np.isfinite(got["v"]).all() and np.isfinite(got["p"]).all()


def test_adamw_refuses_an_unaligned_range_and_writes_nothing(ops):
    from geoguessr_ai_amd import _lib as L
    n = 1024
    bufs = [torch.full((n + 4,), SENTINEL, device="cuda") for _ in range(4)]
    for off in range(4):        # each of params, grads, exp_avg, exp_avg_sq in turn starts 4 bytes off
        views = [b[1:n + 1] if i == off else b[:n] for i, b in enumerate(bufs)]
        with pytest.raises(L.GgError, match="16-byte aligned"):
            ops.adamw_step(views[0], views[1], views[2], views[3], 1, 1e-3)
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)


# ------------------------------------------------------------------------------------------- gradient norm
def test_grad_sq_norm_beyond_one_grid(ops):
    """n = 4194304 + 4099 > 1024 x 4096, values from 1e-8 to 1e4 with both signs, with and without ``accumulate``.  The kernel squares and adds in double: only the
    order differs from the fp64 sum, so rtol 1e-12; the two-stage sum is deterministic, so two calls give the same bits."""
    from geoguessr_ai_amd import _lib as L
    n = 4194304 + 4099
    rng = np.random.default_rng(11)
    g = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-8, 4, n)).astype(np.float32)
    want = float(np.sum(g.astype(np.float64) ** 2))
    gd = _dev(g)
    scratch = torch.empty((L.lib().gg_grad_sq_norm_scratch_doubles(n),), dtype=torch.float64, device="cuda")
    outs = []
    for accumulate, init in ((0, 123.0), (0, 123.0), (1, 2.5), (1, 2.5)):
        out = torch.full((1,), init, dtype=torch.float64, device="cuda")
        L.check(L.lib().gg_grad_sq_norm(L.ptr(gd), n, L.ptr(scratch), L.ptr(out), accumulate, L.stream()), "gg_grad_sq_norm")
        outs.append(float(out.cpu()))
    print(f"\n[grad_sq_norm] fp64 {want!r}  kernel {outs[0]!r}  rel {abs(outs[0] - want) / want:.1e}")
    assert outs[0] == outs[1] and outs[2] == outs[3]
    assert abs(outs[0] - want) <= 1e-12 * want and abs(outs[2] - (want + 2.5)) <= 1e-12 * want
