"""tests/geo_cases.py checked without a GPU: the builders give each class its property, the fp64 reference agrees with oracle.geo_ref (f32) on every case of
the GPU suite, the nearest-index cap holds, every defect is rejected by its gate, and the fp64 AdamW reference is torch.optim.AdamW in float64.  Nothing here
runs a kernel; `pytest -s` prints the tables.

Which case catches which defect (``CATCHES``; each defective fp64 result is fed to the gate as if it were the kernel's):

* ``dup_high``           any case with a duplicated nearest coordinate (``on_centroid`` rows): the nearest rule demands the lower index
* ``padded_column``      ``shift-``: every real logit is near -1e4, the phantom column of logit 0 takes the whole softmax
* ``wave_dmin``          every case of K >= 256: three of the four waves measure their distances from another centroid
* ``hard_no_minus_one``  every mode-2 case
* ``topk_thread_once``   ``ties``: indices 7 and 263 share a thread, and 773, 517, 261, 5 do
* ``mean_256``           the batch cases of N = 257 and 1000
"""
import numpy as np
import pytest
import torch

from oracle import geo_ref as G
from tests import geo_cases as GC

# Bounds on the yardstick's own error (oracle.geo_ref in f32 against the fp64 reference), held on every case of the GPU suite.  Measured with this module: row
# losses 2e-7 .. 2.8e-6, dlogits 1.5e-6 .. 9.3e-6 (the largest at 10 km smoothing), top-k probabilities <= 3.8e-7.  Distances up to 0.9 pi R differ by at most
# 0.008 km (bound: twice that); nearer the antipode asin loses its conditioning (1.7 km at 20035.8 km), which the 0.25 km nearest rule never meets.
Y_LOSS, Y_DLOGITS, DIST_KM = 3e-6, 1.9e-5, 0.016


def test_centroid_table_keeps_its_duplicates():
    c = GC.centroids(12647)
    first, dup = GC.first_index(c)
    assert len(np.unique(first)) == 6823 and int(dup.sum()) == 2 * 5824
    assert np.array_equal(np.sort(c.view(np.uint64).reshape(-1)), np.sort(np.load(GC.GOLDEN).view(np.uint64).reshape(-1)))
    big = GC.centroids(16384)
    assert big.shape == (16384, 2) and np.array_equal(big[:12647], c) and np.abs(big[:, 1]).max() <= 90 and np.abs(big[:, 0]).max() <= 180
    assert np.array_equal(GC.centroids(1025), c[:1025])


def test_every_label_class_has_its_property():
    for K in (1025, 12647):
        c = GC.cond_case(K, "plain")
        d, cent = c["ref"]["dist"], c["cent"]
        first, dup = GC.first_index(cent)
        row = {cls: i for i, cls in enumerate(c["classes"])}
        assert set(row) == set(GC.LABEL_CLASSES)
        k = int(np.argmin(d[row["on_centroid"]]))
        assert d[row["on_centroid"], k] == 0.0 and dup[k] and int((d[row["on_centroid"]] == 0.0).sum()) >= 2
        k = int(np.argmin(d[row["on_unique"]]))
        assert d[row["on_unique"], k] == 0.0 and not dup[k] and int((d[row["on_unique"]] == 0.0).sum()) == 1
        two = np.sort(np.unique(d[row["midpoint"]]))[:2]
        assert two[1] - two[0] < GC.NEAR_KM and not c["near_rule"][row["midpoint"]][0]
        assert np.ptp(d[row["north_pole"]] - GC.R_KM * np.deg2rad(90.0 - cent[:, 1].astype(np.float64))) < 1e-6           # a pole's distance is the co-latitude
        assert np.ptp(d[row["south_pole"]] - GC.R_KM * np.deg2rad(90.0 + cent[:, 1].astype(np.float64))) < 1e-6
        for cls in ("dateline+", "dateline-"):      # the nearest centroid is nearer than the same one measured without wrapping the longitude
            i = row[cls]
            assert d[i].min() < 2000.0
        assert d[row["ocean"]].min() > 1500.0
        assert 0.005 < d[row["offset"]].min() < 0.02
        soft = c["ref"]["soft"][row["ocean"]]
        assert soft.max() > 0.25 and (soft > 1e-6).mean() < 0.02           # a handful of targets hold the row, the rest is below f32's reach of the largest
    K = 12647
    c = GC.cond_case(K, "plain")
    cross = [cls for cls in ("dateline+", "dateline-") if np.sign(c["cent"][int(np.argmin(c["ref"]["dist"][list(c["classes"]).index(cls)])), 0]) != np.sign(GC.FIXED[cls][0])]
    print("\nnearest centroid across the antimeridian for:", cross)


def test_every_logit_class_has_its_property():
    K, N = 1025, 10
    z = {cls: GC.make_logits(N, K, cls, 5) for cls in GC.LOGIT_CLASSES}
    assert all(v.dtype == np.float32 and v.shape == (N, K) for v in z.values())
    assert z["peaked"].std() > 25 and abs(z["shift+"].mean() - 1e4) < 1 and abs(z["shift-"].mean() + 1e4) < 1
    m = np.isneginf(z["masked"])
    assert m[:, K - 300:].all() and 0.25 < m[:, :K - 300].mean() < 0.42 and np.isfinite(z["masked"][~m]).all()
    assert m[:, 768:1024].all()          # register 3 of every thread (columns 768 + tid) holds only -inf
    order = GC.rank_order(z["ties"])
    assert (order[:, :7] == np.asarray(GC.TIE_AT + GC.TIE_NEXT)).all()
    assert (z["ties"][:, GC.TIE_AT[0]][:, None] == z["ties"][:, list(GC.TIE_AT)]).all()
    assert {k % 256 for k in GC.TIE_NEXT} == {5} and GC.TIE_AT[0] % 256 == GC.TIE_AT[2] % 256 and GC.TIE_AT[0] // 64 != GC.TIE_AT[1] // 64
    nan = z["plain"].copy(); nan[0, 700] = np.nan; nan[1] = np.nan
    o = GC.rank_order(nan)
    assert o[0, 0] == 700 and (o[1, :16] == np.arange(16)).all()
    t = torch.from_numpy(z["plain"])
    assert np.array_equal(GC.rank_order(z["plain"])[:, :5], torch.sort(t, dim=-1, descending=True, stable=True).indices[:, :5].numpy())


def test_fp64_reference_restates_the_oracle():
    """In f32 arithmetic the written-out formula IS oracle.geo_ref: soft_ce / hard_ce / head_forward give the yardstick's tensors bit for bit at the oracle's own
    constants (65 km, 1 / N), so the fp64 reference and the yardstick differ by precision alone."""
    c = GC.cond_case(1025, "plain")
    y = GC.yardstick(c)
    loss, dl, soft, d = G.soft_ce(c["logits"], c["labels"], c["cent"])
    assert np.array_equal(d, y["dist"]) and np.array_equal(soft, y["soft"]) and np.float32(loss) == y["loss"]
    np.testing.assert_allclose(y["dlogits"], dl, rtol=3e-7, atol=0)                # (x / n against x * f32(1 / n))
    hl, hdl = G.hard_ce(c["logits"], c["ref"]["labels_clf"])
    assert np.float32(hl) == y["hard_loss"]
    np.testing.assert_allclose(y["hard_dlogits"], hdl, rtol=3e-7, atol=0)
    assert np.array_equal(G.nearest_centroid(c["labels"], c["cent"]), y["nearest"])
    lp = G.log_softmax(c["logits"])
    assert np.array_equal(np.argsort(-lp, axis=-1, kind="stable")[:, :5], c["ref"]["topk_idx"])


def test_fp64_reference_agrees_with_the_f32_oracle_on_every_case_of_the_gpu_suite():
    print()
    worst = {}
    for c in GC.gpu_suite_cases():
        y, ref = GC.yardstick(c), c["ref"]
        f = {n: GC.figure(y[n], ref[n], n == "topk_vals") for n in ("loss_rows", "loss", "dlogits", "hard_rows", "hard_loss", "hard_dlogits", "topk_vals")}
        dist = float(np.abs(y["dist"].astype(np.float64) - ref["dist"]).max())
        print(f"[yardstick] {c['name']:60s} " + "  ".join(f"{n} {v:.1e}" for n, v in f.items()) + f"  dist {dist:.3f} km")
        # near a row's minimum -- all the nearest rule rests on -- and everywhere else up to 0.9 pi R; beyond, the overall figure is printed above
        assert float(np.abs(y["dist"].astype(np.float64) - ref["dist"])[ref["dist"] <= 0.9 * np.pi * GC.R_KM].max()) <= DIST_KM, (c["name"], dist)
        assert f["loss_rows"] <= Y_LOSS and f["hard_rows"] <= Y_LOSS and f["loss"] <= Y_LOSS and f["hard_loss"] <= Y_LOSS, (c["name"], f)
        assert f["dlogits"] <= Y_DLOGITS and f["hard_dlogits"] <= Y_DLOGITS, (c["name"], f)
        assert f["topk_vals"] <= Y_LOSS, (c["name"], f)
        for n, v in f.items():
            worst[n] = max(worst.get(n, 0.0), v)
        # the yardstick passes its own gate, trivially; and the bf16 yardstick is within the bf16 floor of the f32 one
        assert not GC.check(c, {k: y[k2] for k, k2 in GC.tensors_of(1).items()}, 1, label="yardstick")
    print("[yardstick] worst: " + "  ".join(f"{n} {v:.1e}" for n, v in worst.items()))


def test_masked_soft_loss_is_not_finite_in_either_precision():
    for K in GC.COND_K:
        c = GC.cond_case(K, "masked")
        assert not np.isfinite(c["ref"]["loss_rows"]).any() and not np.isfinite(GC.yardstick(c)["loss_rows"]).any()
        assert np.isfinite(c["ref"]["dlogits"]).all() and np.isfinite(GC.yardstick(c)["dlogits"]).all()
        assert np.isfinite(c["ref"]["hard_rows"]).sum() >= 1


def test_nearest_index_cap_and_the_oracles_own_argmin():
    print()
    for c in GC.gpu_suite_cases():
        loose = GC.loose_rows(c)
        print(f"[nearest] {c['name']:60s} rows under the 0.25 km rule: {loose} of {c['N']}")
        assert loose * 8 <= max(c["N"], 8), (c["name"], loose)
        assert not GC.nearest_misses(c, GC.yardstick(c)["nearest"]), (c["name"], GC.nearest_misses(c, GC.yardstick(c)["nearest"]))
        assert not GC.nearest_misses(c, c["ref"]["nearest"])
    c = GC.cond_case(12647, "plain")
    first, dup = GC.first_index(c["cent"])
    strict_dup = [n for n, (strict, a) in enumerate(c["near_rule"]) if strict and dup[next(iter(a))]]
    assert strict_dup, "no row whose nearest coordinate is duplicated: the lower-index rule would not be exercised"


CATCHES = {
    "dup_high": [("cond", 12647, "plain", 1), ("sweep", 1025, None, 1)],
    "padded_column": [("cond", 1025, "shift-", 1), ("cond", 1025, "shift-", 2), ("cond", 12647, "shift-", 1)],
    "wave_dmin": [("cond", 1025, "plain", 1), ("cond", 12647, "peaked", 1), ("sweep", 257, None, 1)],
    "hard_no_minus_one": [("cond", 1025, "plain", 2), ("sweep", 5, None, 2), ("sweep", 16384, None, 2)],
    "topk_thread_once": [("cond", 1025, "ties", 0), ("cond", 12647, "ties", 0)],
    "mean_256": [("batch", 257, None, 1), ("batch", 1000, None, 2)],
}


def _catch_case(kind, a, b):
    return GC.cond_case(a, b) if kind == "cond" else GC.sweep_case(a) if kind == "sweep" else GC.batch_case(a)


@pytest.mark.parametrize("defect", GC.DEFECTS)
def test_every_defect_is_rejected_by_its_gate(defect):
    print()
    for kind, a, b, mode in CATCHES[defect]:
        c = _catch_case(kind, a, b)
        bad = GC.reference(c["logits"], c["labels"], c["cent"], labels_clf=c["ref"]["labels_clf"], defect=defect, **c["kw"])
        got = {k: bad[k2] for k, k2 in GC.tensors_of(mode).items()}
        for dtype in ("f32", "bf16"):
            g = dict(got)
            if dtype == "bf16" and g.get("dlogits") is not None:
                g["dlogits"] = GC.to_bf16(g["dlogits"])
            misses = GC.check(c, g, mode, dtype, label=defect)
            idx = GC.exact_misses(c, bad) + GC.nearest_misses(c, bad["nearest"])
            print(f"[defect] {defect} {c['name']} mode {mode} {dtype}: gate misses {[(n, f'{e:.1e}', f'{g_:.1e}') for n, e, g_ in misses]}, index misses {idx}")
            if defect in ("dup_high", "topk_thread_once"):
                assert idx, (defect, c["name"])
            else:
                assert misses and max(e / g_ for _, e, g_ in misses) >= 10.0, (defect, c["name"], mode, dtype, misses)
        # ... and the sound reference passes the same gates
        good = {k: c["ref"][k2] for k, k2 in GC.tensors_of(mode).items()}
        assert not GC.check(c, good, mode, "f32", label="sound") and not GC.exact_misses(c, c["ref"])
    if defect == "padded_column":       # shift+ cannot see it: its weight is e^-1e4
        c = GC.cond_case(1025, "shift+")
        bad = GC.reference(c["logits"], c["labels"], c["cent"], labels_clf=c["ref"]["labels_clf"], defect=defect, **c["kw"])
        assert not GC.check(c, {k: bad[k2] for k, k2 in GC.tensors_of(1).items()}, 1, label=defect)


def test_haversine_pairs_and_their_yardstick():
    print()
    for name, (x, y) in GC.haversine_pairs().items():
        ref = GC.haversine64(x, y)[0, 0]
        print(f"[haversine pair] {name:16s} fp64 {ref:.9f} km")
        with np.errstate(all="ignore"):
            yard = G.haversine_matrix(x, y.T.copy())
        assert not GC.haversine_check(x, y, np.asarray([[ref]]), name)
        if name == "nan_coordinate":
            assert np.isnan(ref) and np.isnan(yard[0, 0]) and GC.haversine_check(x, y, np.asarray([[np.pi * GC.R_KM]]), name)      # pi R for a NaN is rejected
        if name == "identical":
            assert ref == 0.0 and yard[0, 0] == 0.0
        if name.startswith("1m"):
            assert 0.0005 < ref < 0.005
        if name == "pole_to_pole":
            assert abs(ref - np.pi * GC.R_KM) < 1e-6
        if name == "antimeridian":
            assert ref < 0.25
        if name == "near_antipodal":
            assert 0.9 < np.pi * GC.R_KM - ref < 1.1
        if name == "antipode":
            assert abs(ref - np.pi * GC.R_KM) < 1e-6


@pytest.mark.parametrize("hyper", range(len(GC.ADAMW_HYPER)))
def test_fp64_adamw_reference_is_torch_adamw_in_float64(hyper):
    for seeded, steps in ((False, (1, 2, 3)), (True, (1000,)), (True, (100000,))):
        c = GC.adamw_case(1023, hyper, 0.013, steps=steps, seeded_state=seeded)
        h = c["hyper"]
        tp = torch.nn.Parameter(torch.from_numpy(c["p0"]).double())
        opt = torch.optim.AdamW([tp], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"], foreach=False)
        for i, (s, g) in enumerate(zip(steps, c["grads"])):
            if i == 0 and seeded:
                opt.state[tp] = dict(step=torch.tensor(float(s - 1)), exp_avg=torch.from_numpy(c["m0"]).double(), exp_avg_sq=torch.from_numpy(c["v0"]).double())
            tp.grad = torch.from_numpy(g).double() * c["scale"]
            opt.step()
        st = opt.state[tp]
        assert int(st["step"]) == steps[-1]
        for name, t in (("p", tp.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            assert GC.figure(t.numpy(), c["ref"][name]) < 1e-13, (name, steps)
        # the f32 yardstick is f32-close to it, and passes its own gate
        assert not GC.adamw_check(c, {k: c["yard"][k] for k in ("p", "m", "v")}, "yardstick")
        for name in ("p", "m", "v"):
            assert GC.figure(c["yard"][name], c["ref"][name]) < 1e-6, (name, steps)


def test_adamw_range_classes_are_about_the_f32_range():
    tiny, huge = GC.adamw_case(4099, grad_cls="tiny"), GC.adamw_case(4099, grad_cls="huge")
    assert (tiny["yard"]["v"] == 0).all() and (tiny["ref"]["v"] > 0).all()             # g^2 underflows f32, not fp64
    # g^2 alone overflows f32; torch (addcmul: value * g first) and the kernel ((1 - beta2) * g * g, left to right) keep v finite at 3e37 -- the f32 result is the
    # expected value, and an implementation that squares first gets inf and is rejected
    with np.errstate(over="ignore"):
        assert np.isinf(huge["grads"][0] * huge["grads"][0]).all()
    assert np.isfinite(huge["yard"]["v"]).all() and huge["yard"]["v"].min() > 1e37 and np.isfinite(huge["yard"]["p"]).all()
    squared_first = dict(huge["yard"], v=np.full_like(huge["yard"]["v"], np.inf))
    assert GC.adamw_check(huge, squared_first, "squares first", against_yardstick=True)
    assert not GC.adamw_check(huge, huge["yard"], "yardstick", against_yardstick=True)
    zero = GC.adamw_case(4099, grad_cls="zero")
    assert (zero["yard"]["m"] == 0).all() and (zero["yard"]["v"] == 0).all() and (zero["ref"]["m"] == 0).all()
    assert GC.figure(zero["ref"]["p"], zero["p0"].astype(np.float64) * (1 - zero["hyper"]["lr"] * zero["hyper"]["wd"]) ** 3) < 1e-15
    mixed = GC.adamw_case(4099, grad_cls="mixed")
    a = np.abs(mixed["grads"][0])
    assert a.min() < 1e-5 and a.max() > 1e2 and (mixed["grads"][0] < 0).any() and (mixed["grads"][0] > 0).any()
