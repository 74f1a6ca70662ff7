"""Edge-case inputs for the geocell head (gg_geo_head), the haversine matrix and AdamW, their fp64 references and the yardsticks the tests gate against.
Plain numpy / torch on the CPU: no GPU, no libgg.  The pattern is that of tests/attention_cases.py.

A head case is made by ``case(K, N, label_cls, logit_cls, smoothing_km, grad_scale, num_candidates)`` and computed once (lru_cache; never modify what it
returns).  It holds the f32 inputs, the fp64 reference of BOTH loss modes (``ref``: soft CE = mode 1, hard CE on the fp64 nearest centroid = mode 2) and of
the predictions, and on first use the yardstick's tensors.  Mode and the dlogits type are arguments of ``check``: they select what is compared and how the
yardstick is rounded.

Centroids: the first K rows of a fixed permutation of tests/golden/centroids_12647x2_f32.npy (6823 distinct coordinates among 12647 rows: the duplicates
stay in), beyond 12647 rows seeded uniform lon / lat.

Label classes (``LABEL_CLASSES``; ``label_cls`` names one for every row, or ``"each"``: row i has class i mod 10, ``"sweep"``: the eight of ``SWEEP_LABELS``):

* ``on_centroid``  exactly a centroid that has a duplicate among the K rows (d_min = 0 twice, bit-identically: the lower index must win)
* ``on_unique``    exactly a centroid without a duplicate
* ``midpoint``     the fp64 midpoint (in lon / lat) of a centroid and its nearest neighbour at another coordinate, rounded to f32: two candidates within metres
* ``north_pole``   (0, 90)    ``south_pole``  (12.5, -90): cos(lat) = 6e-17 in fp64, -4e-8 in f32
* ``dateline+/-``  (+-179.99, -16.5): the nearest centroids lie across the antimeridian
* ``ocean``        (-140, -50): thousands of km from every centroid, the soft target is nearly one-hot and most of the row underflows
* ``offset``       a centroid plus 1e-4 degrees (11 m): sin^2 of a 1e-6 rad difference
* ``plain``        a centroid plus up to 0.5 degrees, latitude clipped to +-89.5: the draw of the older tests, the control

Logit classes (``LOGIT_CLASSES``): ``plain`` N(0, 1); ``peaked`` N(0, 1) x 30; ``shift+/-`` plain +- 1e4 (rounded to f32: every reference sees the rounded
values); ``masked`` -inf on a random third of the row and on the last 300 columns (whole waves hold only -inf in their last registers); ``ties`` the row maximum at indices 7, 71
and 263 (same wave, another wave, the same thread's next register) and the next four largest values at 773, 517, 261, 5 in that order (all = 5 mod 256: one
thread owns them).  A -inf logit under a positive soft target makes the soft-CE row loss +inf in fp64 and NaN in f32 (0 x -inf where the target underflows):
on ``masked`` the soft loss is required to be non-finite, nothing more; its gradient is finite and gated like any other.

fp64 reference (``reference``): models/utils.py:20-57 and models/super_guessr.py:333-383 as oracle/geo_ref.py cites them, every operand widened to float64
first (a is clamped to 1 before asin, the kernels' documented clamp): distances, first argmin, soft targets with nan_to_num and the 1e-12 clamp, row losses
and their mean, dlogits x grad_scale, the ranking (NaN first, then the larger value, then the lower index: torch.topk / a stable argsort), probabilities, llh,
hard-CE rows and gradient.

Error figure: ``e(T) = max |got - ref64| / max |ref64|`` over the finite elements of ref64 (0 / 0 = 0); where ref64 is not finite ``got`` must not be
either, and where it is ``got`` must be: otherwise e = inf.  top-k probabilities are ranked per row, so their figure is the largest per-row
``max |got - ref| / ref[row, 0]``.  Gate: ``e <= 4 max(y, floor)``, floor 2^-24 for f32 results and 2^-9 for bf16 dlogits, y the same figure of the
yardstick on the same case -- the rule of tests/attention_cases.py and tests/test_gpu_cls_head.py.  The yardstick is never the kernel: it is oracle.geo_ref
in f32 (haversine_matrix, log_softmax and, at 65 km, smooth_labels; another smoothing constant is the same line with that constant), for bf16 dlogits
rounded to bf16 once.

Nearest-centroid rule (``nearest_rule``): g = fp64 gap between the nearest centroid and the nearest one at a DIFFERENT coordinate.  g >= 0.25 km (twice the
0.058 km, the largest f32 distance error against fp64 on the 12647-row table, rounded up): ``nearest`` is the lowest index of the nearest coordinate -- the fp64 first argmin.
g < 0.25 km: the lowest index of any coordinate within 0.25 km of the minimum.  At most one row in eight of a case may be of the second kind
(tests/test_geo_cases_cpu.py asserts it for every case of the GPU suite, and that oracle.geo_ref's own argmin obeys the rule).

Defects (``DEFECTS``): CPU restatements of kernel bugs applied to the fp64 formula; tests/test_geo_cases_cpu.py shows each rejected.

AdamW (``adamw_case``): reference oracle.geo_ref.adamw_step on float64 arrays, yardstick torch.optim.AdamW on f32 CPU tensors, figures on p, m, v and on the
update dp = p_after - p_before (p alone hides an error of the update behind |p|).  The C entry point takes its hyper-parameters as float: all three see the
f32-rounded lr, betas, eps, weight decay and grad_scale (1 - f32(0.999) differs from 1e-3 by 1.3e-5: not an error of the kernel's arithmetic).

Largest measured figures on an MI355X, kernel e / yardstick y (tests/test_gpu_geo_conditioning.py, `pytest -s`):
  head (sweep, conditioning, parameters, batch):  loss_rows 2.7e-06 / 2.8e-06   loss 2.4e-07 / 2.4e-07   dlogits f32 9.2e-06 / 9.3e-06   dlogits bf16 2.6e-03 / 2.6e-03
                                                  topk_vals 1.8e-07 / 1.8e-07 (computed in double from the f32 sum; with the fast f32 exponential one row of the
                                                  N = 1 batch case was at 3.5e-07 against a yardstick of 6.6e-08: outside 4 x 2^-24)
  haversine:  identical 0 / 0   1 m at the origin 6.9e-08 / 6.9e-08   4 m at 59.91 N 5.3e-03 / 5.3e-03   pole to pole 2.6e-08 / 2.6e-08
              antimeridian 1.2e-03 / 1.2e-03   1 km short of antipodal 1.7e-04 / 5.0e-05   400 x 12647 1.5e-05 / 2.0e-05
  AdamW:      p 1.5e-07 / 1.5e-07   m 1.6e-07 / 1.6e-07   v 1.9e-07 / 1.9e-07   dp 4.5e-04 / 4.5e-04 (zero gradients: the update is the decay's last bit)
  gradient norm (n = 4198403): relative difference from the fp64 sum 3.9e-16
"""
import functools
import math
import os
import zlib

import numpy as np

from oracle import geo_ref as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "centroids_12647x2_f32.npy")
F32, F64 = np.float32, np.float64
FLOOR = {"f32": 2.0 ** -24, "bf16": 2.0 ** -9}
FACTOR = 4.0
NEAR_KM = 0.25
R_KM = G.EARTH_RADIUS_M / 1000.0
LABEL_CLASSES = ("on_centroid", "on_unique", "midpoint", "north_pole", "south_pole", "dateline+", "dateline-", "ocean", "offset", "plain")
SWEEP_LABELS = ("on_centroid", "on_unique", "midpoint", "north_pole", "dateline+", "ocean", "offset", "plain")
LOGIT_CLASSES = ("plain", "peaked", "shift+", "shift-", "masked", "ties")
DEFECTS = ("dup_high", "padded_column", "wave_dmin", "hard_no_minus_one", "topk_thread_once", "mean_256")
TIE_AT, TIE_NEXT = (7, 71, 263), (773, 517, 261, 5)
FIXED = {"north_pole": (0.0, 90.0), "south_pole": (12.5, -90.0), "dateline+": (179.99, -16.5), "dateline-": (-179.99, -16.5), "ocean": (-140.0, -50.0)}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def _table():
    t = np.load(GOLDEN)
    return np.ascontiguousarray(t[np.random.default_rng(12647).permutation(len(t))])


@functools.lru_cache(maxsize=None)
def centroids(K):
    """(K, 2) f32 lon, lat: the first K rows of the permuted golden table, then seeded uniform rows.  Do not modify."""
    t = _table()
    if K <= len(t):
        return np.ascontiguousarray(t[:K])
    rng = np.random.default_rng(K)
    extra = np.stack([rng.uniform(-180, 180, K - len(t)), rng.uniform(-90, 90, K - len(t))], 1).astype(F32)
    return np.ascontiguousarray(np.concatenate([t, extra]))


def first_index(cent):
    """(K,) lowest index that has the same (bit-identical) coordinate, and (K,) whether the coordinate occurs more than once."""
    keys = np.ascontiguousarray(cent).view(np.uint64).reshape(-1)
    _, first, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    return first[inverse], counts[inverse] > 1


def haversine64(x, cent):
    """(N, K) km in fp64 from f32 (lon, lat) degrees; a clamped to 1."""
    xr, cr = np.deg2rad(x.astype(F64)), np.deg2rad(cent.astype(F64))
    dlon, dlat = xr[:, None, 0] - cr[None, :, 0], xr[:, None, 1] - cr[None, :, 1]
    a = np.sin(dlat / 2) ** 2 + np.cos(xr[:, None, 1]) * np.cos(cr[None, :, 1]) * np.sin(dlon / 2) ** 2
    with np.errstate(invalid="ignore"):
        return R_KM * 2 * np.arcsin(np.sqrt(np.minimum(a, 1.0)))


def label_classes(label_cls, N):
    if label_cls == "each":
        return tuple(LABEL_CLASSES[i % len(LABEL_CLASSES)] for i in range(N))
    if label_cls == "sweep":
        return tuple(SWEEP_LABELS[i % len(SWEEP_LABELS)] for i in range(N))
    assert label_cls in LABEL_CLASSES, label_cls
    return (label_cls,) * N


def make_labels(cent, classes, seed):
    """(N, 2) f32 labels, one class per row.  Where the K rows hold no duplicate (small K) ``on_centroid`` is a centroid all the same."""
    rng = np.random.default_rng(seed)
    K = len(cent)
    first, dup = first_index(cent)
    out = np.zeros((len(classes), 2), F32)
    for i, cls in enumerate(classes):
        pick = int(rng.integers(0, K))
        if cls in FIXED:
            out[i] = FIXED[cls]
        elif cls == "on_centroid":
            pool = np.flatnonzero(dup)
            out[i] = cent[pool[pick % len(pool)]] if len(pool) else cent[pick]
        elif cls == "on_unique":
            pool = np.flatnonzero(~dup)
            out[i] = cent[pool[pick % len(pool)]] if len(pool) else cent[pick]
        elif cls == "midpoint":
            d = haversine64(cent[pick:pick + 1], cent)[0]
            d[first == first[pick]] = np.inf
            other = int(np.argmin(d)) if np.isfinite(d).any() else pick
            out[i] = ((cent[pick].astype(F64) + cent[other].astype(F64)) / 2).astype(F32)
        elif cls == "offset":
            out[i] = (cent[pick].astype(F64) + 1e-4).astype(F32)
        elif cls == "plain":
            out[i] = (cent[pick] + rng.uniform(-0.5, 0.5, 2)).astype(F32)
        else:
            raise ValueError(cls)
        out[i, 1] = np.clip(out[i, 1], -89.5, 89.5) if cls in ("plain", "offset") else out[i, 1]
    return out


def make_logits(N, K, cls, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((N, K))
    if cls == "plain":
        pass
    elif cls == "peaked":
        z *= 30.0
    elif cls in ("shift+", "shift-"):
        z += 1e4 if cls == "shift+" else -1e4
    elif cls == "masked":
        assert K > 600
        z[rng.random((N, K)) < 1.0 / 3.0] = -np.inf
        z[:, K - 300:] = -np.inf
    elif cls == "ties":
        assert K > max(TIE_NEXT + TIE_AT)
        top = np.ceil(z.max(-1)) + 3.0
        for j in TIE_AT:
            z[:, j] = top
        for r, j in enumerate(TIE_NEXT):
            z[:, j] = top - 0.5 * (r + 1)
    else:
        raise ValueError(cls)
    return z.astype(F32)


def rank_order(z):
    """(N, K) indices in ranking order: NaN first, then the larger value, then the lower index."""
    nan = np.isnan(z)
    key = np.where(nan, 0.0, -z.astype(F64))
    return np.stack([np.lexsort((np.arange(z.shape[1]), key[n], ~nan[n])) for n in range(z.shape[0])])


def _log_softmax64(z):
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def reference(logits, labels, cent, smoothing_km=65.0, grad_scale=None, num_candidates=5, labels_clf=None, defect=None):
    """Everything gg_geo_head returns, in fp64 (see the module docstring).  ``labels_clf`` defaults to the reference's own nearest index.  ``defect``: one of DEFECTS."""
    N, K = logits.shape
    gs = 1.0 / N if grad_scale is None else float(F32(grad_scale))
    s = float(F32(smoothing_km)) if smoothing_km > 0 else 65.0
    z = logits.astype(F64)
    first, _ = first_index(cent)
    r = {}
    with np.errstate(all="ignore"):
        d = haversine64(labels, cent)
        near = first[np.argmin(d, -1)]
        r["dist"], r["nearest"] = d, near.astype(np.int64)
        if defect == "dup_high":                                    # the last of the bit-identical minima instead of the first
            r["nearest"] = np.asarray([np.flatnonzero(first == f).max() for f in near], np.int64)
        dmin = d.min(-1, keepdims=True)
        if defect == "wave_dmin":                                   # column k lives in thread k mod 256, wave (k mod 256) // 64: the minimum of the wave's own columns
            wave = (np.arange(K) % 256) // 64
            dmin = np.stack([np.where(wave == w, d, np.inf).min(-1) for w in range(4)], -1)[:, wave]
        soft = np.nan_to_num(np.exp(-(d - dmin) / s), nan=0.0, posinf=0.0, neginf=0.0)
        soft = soft / np.maximum(soft.sum(-1, keepdims=True), 1e-12)
        lp = _log_softmax64(z)
        if defect == "padded_column":                               # one column k >= K of logit 0 in the sum
            lse = z - lp
            lp = z - np.logaddexp(lse, 0.0)
        p = np.exp(lp)
        r["soft"] = soft
        r["loss_rows"] = -(soft * lp).sum(-1)
        r["dlogits"] = (p * soft.sum(-1, keepdims=True) - soft) * gs
        lab = r["nearest"] if labels_clf is None else np.asarray(labels_clf, np.int64)
        r["labels_clf"] = lab
        r["hard_rows"] = -lp[np.arange(N), lab]
        hd = p.copy()
        if defect != "hard_no_minus_one":
            hd[np.arange(N), lab] -= 1.0
        r["hard_dlogits"] = hd * gs
        mean = (lambda v: v[:256].sum() / N) if defect == "mean_256" else (lambda v: v.mean())
        r["loss"], r["hard_loss"] = mean(r["loss_rows"]), mean(r["hard_rows"])
        order = rank_order(logits)
        if defect == "topk_thread_once":                            # a thread offers its own best once and is not asked again: the top-k of the 256 thread maxima
            order = np.stack([np.asarray([j for j in order[n] if j == order[n][np.flatnonzero(order[n] % 256 == j % 256)[0]]]) for n in range(N)])
        idx = order[:, :num_candidates]
        r["topk_idx"] = idx.astype(np.int64)
        r["topk_vals"] = np.take_along_axis(p, idx, -1)
        r["preds"] = idx[:, 0].astype(np.int64)
        r["llh"] = cent[idx[:, 0]]
    return r


def yardstick_tensors(logits, labels, cent, smoothing_km=65.0, grad_scale=None, num_candidates=5, labels_clf=None):
    """The same tensors from oracle.geo_ref in f32 (its haversine_matrix, smooth_labels, log_softmax; soft_ce's and hard_ce's lines with grad_scale in place of
    1 / n and per-row losses kept)."""
    N, K = logits.shape
    gs = F32(1.0 / N if grad_scale is None else grad_scale)
    s = F32(smoothing_km) if smoothing_km > 0 else F32(65.0)
    with np.errstate(all="ignore"):
        d = G.haversine_matrix(labels.astype(F32), cent.T.astype(F32))
        if s == F32(G.LABEL_SMOOTHING_CONSTANT):
            soft = G.smooth_labels(d)
        else:
            soft = np.nan_to_num(np.exp(-(d - d.min(axis=-1, keepdims=True)) / s), nan=0.0, posinf=0.0, neginf=0.0)
        soft = soft / np.maximum(soft.sum(axis=-1, keepdims=True), F32(1e-12))
        lp = G.log_softmax(logits.astype(F32))
        p = np.exp(lp)
        r = dict(dist=d, nearest=d.argmin(axis=-1).astype(np.int64), soft=soft)
        r["loss_rows"] = -(soft * lp).sum(axis=-1)
        r["loss"] = r["loss_rows"].mean()
        r["dlogits"] = (p * soft.sum(axis=-1, keepdims=True) - soft) * gs
        lab = np.asarray(labels_clf, np.int64)
        r["hard_rows"] = -lp[np.arange(N), lab]
        r["hard_loss"] = r["hard_rows"].mean()
        hd = p.copy()
        hd[np.arange(N), lab] -= 1
        r["hard_dlogits"] = hd * gs
        idx = rank_order(logits)[:, :num_candidates]
        r["topk_vals"] = np.take_along_axis(p, idx, -1)
    assert all(v.dtype == F32 for k, v in r.items() if k != "nearest"), {k: v.dtype for k, v in r.items()}
    return r


# ------------------------------------------------------------------------------------------- figures and gates
def figure(got, ref, per_row_top=False):
    """e(T), see the module docstring.  ``per_row_top``: ranked rows, each normalised by its own first reference value."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    if (np.isfinite(got) != fin).any():
        return math.inf
    if not fin.any():
        return 0.0
    diff = np.where(fin, np.abs(got - np.where(fin, ref, 0.0)), 0.0)
    if per_row_top:
        top = np.abs(ref[:, :1])
        with np.errstate(all="ignore"):
            q = np.where(diff == 0.0, 0.0, diff / top)
        return float(np.nanmax(q))
    err, mag = float(diff.max()), float(np.abs(ref[fin]).max())
    return 0.0 if err == 0.0 else (math.inf if mag == 0.0 else err / mag)


def to_bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).to(torch.bfloat16).float().numpy()


def tensors_of(mode):
    """The gated tensors of a mode: {name in ``got``: name in the reference}."""
    t = {"topk_vals": "topk_vals"}
    if mode == 1:
        t.update(loss_rows="loss_rows", loss="loss", dlogits="dlogits")
    if mode == 2:
        t.update(loss_rows="hard_rows", loss="hard_loss", dlogits="hard_dlogits")
    return t


def nearest_rule(d64, cent):
    """Per row (strict, allowed): ``strict`` -- the gap to the nearest other coordinate is >= NEAR_KM and ``allowed`` is the one index the fp64 first argmin gives;
    otherwise ``allowed`` holds the lowest index of every coordinate within NEAR_KM of the minimum."""
    first, _ = first_index(cent)
    rules = []
    for row in d64:
        k0 = first[int(np.argmin(row))]
        dmin = row.min()
        others = row[first != k0]
        gap = (others.min() - dmin) if len(others) else math.inf
        if gap >= NEAR_KM:
            rules.append((True, {int(k0)}))
        else:
            rules.append((False, {int(f) for f in first[row <= dmin + NEAR_KM]}))
    return rules


def nearest_misses(c, near):
    """Rows whose ``nearest`` breaks the rule: [(row, got, allowed)]."""
    near = np.asarray(near).reshape(-1)
    return [(n, int(near[n]), sorted(a)) for n, (_, a) in enumerate(c["near_rule"]) if int(near[n]) not in a]


def loose_rows(c):
    return sum(1 for strict, _ in c["near_rule"] if not strict)


@functools.lru_cache(maxsize=None)
def case(K, N, label_cls="each", logit_cls="plain", smoothing_km=65.0, grad_scale=None, num_candidates=5):
    """Inputs, the fp64 reference and the nearest rule.  Computed once; do not modify."""
    assert logit_cls in LOGIT_CLASSES
    cent = centroids(K)
    classes = label_classes(label_cls, N)
    labels = make_labels(cent, classes, _seed("labels", K, N, label_cls))
    logits = make_logits(N, K, logit_cls, _seed("logits", K, N, logit_cls))
    kw = dict(smoothing_km=smoothing_km, grad_scale=grad_scale, num_candidates=num_candidates)
    c = dict(K=K, N=N, label_cls=label_cls, logit_cls=logit_cls, classes=classes, cent=cent, labels=labels, logits=logits, kw=kw,
             name=f"K={K} N={N} {label_cls}/{logit_cls} s={smoothing_km:g} gs={'1/N' if grad_scale is None else grad_scale} nc={num_candidates}")
    c["ref"] = reference(logits, labels, cent, **kw)
    c["near_rule"] = nearest_rule(c["ref"]["dist"], cent)
    return c


def adhoc_case(logits, labels, cent, name, **kw):
    """A case around inputs made elsewhere (f32 arrays)."""
    kw = dict(dict(smoothing_km=65.0, grad_scale=None, num_candidates=5), **kw)
    c = dict(K=logits.shape[1], N=logits.shape[0], cent=cent, labels=labels, logits=logits, kw=kw, name=name)
    c["ref"] = reference(logits, labels, cent, **kw)
    c["near_rule"] = nearest_rule(c["ref"]["dist"], cent)
    return c


def yardstick(c):
    if "yard" not in c:
        c["yard"] = yardstick_tensors(c["logits"], c["labels"], c["cent"], labels_clf=c["ref"]["labels_clf"], **c["kw"])
    return c["yard"]


def check(c, got, mode, dlogits="f32", label="", ref=None, collect=None):
    """Print every figure next to its yardstick and return the misses [(tensor, e, gate)].  ``got``: numpy arrays by the kernel's names (loss_rows, loss, dlogits
    [N, K], topk_vals; absent ones are skipped).  ``ref``: another reference dict in place of the case's (the CPU test passes the yardstick's own or a defective one
    as ``got``)."""
    ref, yard = c["ref"] if ref is None else ref, yardstick(c)
    bad, cells = [], []
    for name, rname in tensors_of(mode).items():
        if got.get(name) is None:
            continue
        y_t, kind = yard[rname], "f32"
        if name == "dlogits" and dlogits == "bf16":
            y_t, kind = to_bf16(y_t), "bf16"
        top = name == "topk_vals"
        e, y = figure(got[name], ref[rname], top), figure(y_t, c["ref"][rname], top)
        gate = FACTOR * max(y, FLOOR[kind])
        ok = e <= gate
        cells.append(f"{name} {e:.1e}/{y:.1e}" + ("" if ok else f" MISS(gate {gate:.1e})"))
        if collect is not None:
            key = name + ("_bf16" if kind == "bf16" else "")
            if e > collect.get(key, (-1.0, 0.0))[0]:
                collect[key] = (e, y)
        if not ok:
            bad.append((name, e, gate))
    print(f"\n[{label} mode {mode} {c['name']}] kernel/yardstick: " + "  ".join(cells))
    return bad


def exact_misses(c, got):
    """The index results, which are exact: topk_idx, preds, llh (a gather of f32 centroids)."""
    ref, bad = c["ref"], []
    for name in ("topk_idx", "preds", "llh"):
        if got.get(name) is not None and not np.array_equal(np.asarray(got[name]), ref[name]):
            rows = np.flatnonzero((np.asarray(got[name]).reshape(c["N"], -1) != ref[name].reshape(c["N"], -1)).any(-1))
            bad.append((name, rows.tolist()[:8]))
    return bad


# ------------------------------------------------------------------------------------------- the cases of tests/test_gpu_geo_conditioning.py
SWEEP_K = (1, 5, 255, 256, 257, 1024, 1025, 4096, 4097, 12800, 12801, 16384)
COND_K = (1025, 12647)
PARAM_CASES = [dict(smoothing_km=10.0), dict(smoothing_km=300.0), dict(grad_scale=0.37), dict(num_candidates=1), dict(num_candidates=16)]
BATCH_N, BATCH_K = (1, 257, 1000), 300


def sweep_case(K):
    return case(K, 8, "sweep", "plain", num_candidates=min(5, K))


def cond_case(K, logit_cls):
    return case(K, len(LABEL_CLASSES), "each", logit_cls)


def param_case(i):
    return case(1025, len(LABEL_CLASSES), "each", "peaked", **PARAM_CASES[i])


def batch_case(N):
    return case(BATCH_K, N, "each", "plain")


def gpu_suite_cases():
    """Every head case the GPU suite runs."""
    cs = [sweep_case(K) for K in SWEEP_K] + [cond_case(K, z) for K in COND_K for z in LOGIT_CLASSES]
    return cs + [param_case(i) for i in range(len(PARAM_CASES))] + [batch_case(N) for N in BATCH_N]


# ------------------------------------------------------------------------------------------- haversine pairs
def haversine_pairs():
    """{name: (x (1, 2) f32, y (1, 2) f32)}; every reference sees the f32 values."""
    a = np.asarray([[10.75, 59.91]], F32)
    one_m = 1.0 / 111319.49            # degrees of latitude in a metre
    p = {
        "identical": (a, a.copy()),
        "1m_origin": (np.asarray([[0.0, 0.0]], F32), np.asarray([[0.0, one_m]], F32)),
        "4m_oslo": (a, np.asarray([[10.75, 59.91 + 4 * one_m]], F32)),      # four metres: one ulp of 59.91 degrees is 0.4 m
        "pole_to_pole": (np.asarray([[0.0, 90.0]], F32), np.asarray([[12.5, -90.0]], F32)),
        "antimeridian": (np.asarray([[179.999, -16.5]], F32), np.asarray([[-179.999, -16.5]], F32)),
        "near_antipodal": (np.asarray([[30.0, 20.0]], F32), np.asarray([[-150.0, -20.0 + 1.0 / 111.31949]], F32)),
        "antipode": (np.asarray([[0.0, 0.0]], F32), np.asarray([[180.0, 0.0]], F32)),
        "nan_coordinate": (np.asarray([[np.nan, 10.0]], F32), np.asarray([[20.0, 30.0]], F32)),      # NaN in, NaN out (include/gg.h), never the clamp's pi R
    }
    return p


def haversine_check(x, cent, got, label, collect=None):
    """Gate a (N, K) f32 distance matrix: [(tensor, e, gate)] misses."""
    ref = haversine64(x, cent)
    with np.errstate(all="ignore"):
        yard = G.haversine_matrix(x.astype(F32), cent.T.astype(F32))
    yard = np.where(np.isfinite(yard), yard, ref)       # the oracle has no clamp: where an exact antipode makes it NaN it says nothing (the kernel must be finite there all the same)
    e, y = figure(got, ref), figure(yard, ref)
    gate = FACTOR * max(y, FLOOR["f32"])
    print(f"\n[haversine {label}] kernel/yardstick: dist {e:.1e}/{y:.1e}" + ("" if e <= gate else f" MISS(gate {gate:.1e})"))
    if collect is not None and e > collect.get("dist", (-1.0, 0.0))[0]:
        collect["dist"] = (e, y)
    return [] if e <= gate else [("dist", e, gate)]


# ------------------------------------------------------------------------------------------- AdamW
ADAMW_HYPER = (((0.9, 0.999), 1e-8, 0.01), ((0.9, 0.98), 1e-6, 0.1), ((0.5, 0.9), 1e-8, 0.0))
ADAMW_SCALES = (1.0, 1.0 / 8.0, 0.013)
ADAMW_SIZES = (1, 2, 3, 4, 5, 1023, 8388608 + 4099)
ADAMW_LR = 1e-2
GRAD_CLASSES = ("zero", "tiny", "huge", "mixed")


def f32r(x):
    """The value a float parameter of the C entry point carries."""
    return float(F32(x))


def adamw_grads(n, cls, seed):
    rng = np.random.default_rng(seed)
    if cls == "normal":
        return (rng.standard_normal(n) * 0.1).astype(F32)
    if cls == "zero":
        return np.zeros(n, F32)
    if cls == "tiny":
        return np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(F32) * F32(1e-30)
    if cls == "huge":
        return np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(F32) * F32(1e20)
    if cls == "mixed":
        return (np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 3, n)).astype(F32)
    raise ValueError(cls)


def adamw_case(n, hyper=0, scale=1.0, steps=(1, 2, 3), grad_cls="normal", seeded_state=False, lr=ADAMW_LR):
    """p0, m0, v0, one gradient per step (all f32), the fp64 reference and the f32 torch yardstick after the whole sequence: dicts of p, m, v, dp."""
    import torch
    (b1, b2), eps, wd = ADAMW_HYPER[hyper]
    rng = np.random.default_rng(_seed("adamw", n, hyper, scale, steps, grad_cls))
    p0 = (rng.standard_normal(n) * 0.1).astype(F32)
    m0 = (rng.standard_normal(n) * 0.01).astype(F32) if seeded_state else np.zeros(n, F32)
    v0 = (rng.random(n) * 1e-3).astype(F32) if seeded_state else np.zeros(n, F32)
    grads = [adamw_grads(n, grad_cls, _seed("g", n, s, grad_cls)) for s in steps]
    h = dict(lr=f32r(lr), beta1=f32r(b1), beta2=f32r(b2), eps=f32r(eps), wd=f32r(wd))
    gs = f32r(scale)
    p, m, v = p0.astype(F64), m0.astype(F64), v0.astype(F64)
    with np.errstate(all="ignore"):
        for s, g in zip(steps, grads):
            p, m, v = G.adamw_step(p, g.astype(F64) * gs, m, v, s, **h)
    ref = dict(p=p, m=m, v=v, dp=p - p0.astype(F64))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.AdamW([tp], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"], foreach=False)
        for i, (s, g) in enumerate(zip(steps, grads)):
            if i == 0 and (seeded_state or s != 1):
                opt.state[tp] = dict(step=torch.tensor(float(s - 1)), exp_avg=torch.from_numpy(m0.copy()), exp_avg_sq=torch.from_numpy(v0.copy()))
            tp.grad = torch.from_numpy(g) * torch.tensor(gs, dtype=torch.float32)
            opt.step()
        st = opt.state[tp]
        yard = dict(p=tp.detach().numpy().copy(), m=st["exp_avg"].numpy().copy(), v=st["exp_avg_sq"].numpy().copy())
    finally:
        torch.set_num_threads(threads)
    yard["dp"] = yard["p"].astype(F64) - p0.astype(F64)
    return dict(n=n, p0=p0, m0=m0, v0=v0, grads=grads, steps=tuple(steps), hyper=h, scale=gs, ref=ref, yard=yard,
                name=f"n={n} betas=({b1},{b2}) eps={eps} wd={wd} gs={scale:.3g} steps={tuple(steps)} {grad_cls}")


def adamw_check(c, got, label="", against_yardstick=False, collect=None):
    """Misses of p, m, v, dp (``got``: f32 arrays p, m, v).  ``against_yardstick``: the f32 result is the expected value (gradient classes whose point is the f32
    range: g^2 under- or overflows, fp64 does not); the gate is then 4 floors, and non-finite elements must agree exactly."""
    got = dict(got, dp=got["p"].astype(F64) - c["p0"].astype(F64))
    bad, cells = [], []
    for name in ("p", "m", "v") if against_yardstick else ("p", "m", "v", "dp"):      # (dp against an f32 expected value would compare p's own last bit with the decay)
        if against_yardstick:
            e, y = figure(got[name], c["yard"][name]), 0.0
            exact = np.array_equal(np.asarray(got[name], F64)[~np.isfinite(c["yard"][name])], np.asarray(c["yard"][name], F64)[~np.isfinite(c["yard"][name])])
            e = e if exact else math.inf
        else:
            e, y = figure(got[name], c["ref"][name]), figure(c["yard"][name], c["ref"][name])
        gate = FACTOR * max(y, FLOOR["f32"])
        cells.append(f"{name} {e:.1e}/{y:.1e}" + ("" if e <= gate else f" MISS(gate {gate:.1e})"))
        if collect is not None and not against_yardstick and e > collect.get("adamw_" + name, (-1.0, 0.0))[0]:
            collect["adamw_" + name] = (e, y)
        if not e <= gate:
            bad.append((name, e, gate))
    print(f"\n[adamw {label} {c['name']}] kernel/{'f32 torch as expected value' if against_yardstick else 'yardstick'}: " + "  ".join(cells))
    return bad
