"""tests/attention_cases.py checked without a GPU: the layouts, the formula, the property each input class is built for, the size of the f32 yardstick on
every case the GPU suite runs, and that the gates reject defective references.  Nothing here runs a kernel; `pytest -s` prints the two tables.

Which class catches which defect (every defect is a CPU restatement applied to the fp64 formula; its error must exceed the gate of the case by >= 10 x on the
classes named here, ``CATCHES``, at every shape where the defect exists at all):

* ``phantom_key``      (a padded / out-of-window key of score 0 and v = 0 in the sum): ``shift-`` -- all real scores are near -32, the phantom key takes the whole
                       row, error 1.0 on out, dq, dk, dv.  ``shift+`` cannot see it (its weight is e^-32: asserted below the gate), and on the ``plain`` and
                       ``late`` draws of a 14 x 14 window at bf16 storage it is at 1.5 x and 0.9 x the gate: not a reliable catch, and the reason the older
                       tests with their fixed 2e-2 let it pass.
* ``mask_off_by_one``  (causal: key i + 1 admitted): ``masked_spike`` -- the admitted key has score 64 against the diagonal's 32.
* ``tile_max``         (a per-tile maximum without rescale): ``late`` -- its staircase makes the running maximum grow in every 64-key tile; no defect exists on a
                       single tile (49 tokens).
* ``bias_index``       (the gather index off by one): ``bias_spike`` -- the +24 entry lands on another key.
* ``neighbour_lse``    (the backward recomputes P with the next row's lse; forward untouched): ``late`` and ``early`` -- the spike rows' lse differs from their
                       neighbours' by about 30."""
import pytest
import torch

from tests import attention_cases as A

F64 = torch.float64
SHAPES = {      # the three (N, hd) of the issue's measurement, and a causal one
    "7x7 hd32": dict(layout="tinyvit", N=49, hd=32, ws=7, map_hw=14, windows=8),
    "14x14 hd32": dict(layout="tinyvit", N=196, hd=32, ws=14, map_hw=14, windows=2),
    "200 hd64": dict(layout="clip", N=200, hd=64),
    "causal 77 hd64": dict(layout="clip", N=77, hd=64, causal=True),
}
CATCHES = {"phantom_key": ("shift-",), "mask_off_by_one": ("masked_spike",), "tile_max": ("late",), "bias_index": ("bias_spike",), "neighbour_lse": ("late", "early")}


def _case(shape, cls, storage="f32"):
    s = SHAPES[shape]
    return A.case(s["layout"], s["N"], s["hd"], 2, s.get("windows", 2), s.get("ws", 0), s.get("causal", False), storage, cls, s.get("map_hw", 0))


def _probs(c):
    s = A._scores(c["q"], c["k"], None if c["table"] is None else c["table"].double()[:, c["bidx"]], c["scale"], c["causal"])
    return s, torch.softmax(s, -1)


def test_gather_index_is_the_oracles():
    from oracle.tinyvit_ref import attention_bias_idxs
    for ws in (7, 10, 12):
        assert torch.equal(A.bias_idxs(ws), attention_bias_idxs(ws))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_flat_layouts_round_trip_and_match_the_older_tests_reference(shape):
    """The flat qkv / dout buffers are what the kernels' older tests feed them: the view / permute reference of tests/test_gpu_kernels.py::_attn_ref on the flat buffer
    gives the canonical reference's output, and canon_* invert the flattening."""
    c = _case(shape, "plain")
    W, H, N, D, ws = c["windows"], c["heads"], c["N"], c["hd"], c["ws"]
    qkv = c["qkv"].double()
    if c["layout"] == "tinyvit":
        B, Hm = W // (c["map_hw"] // ws) ** 2, c["map_hw"]
        x = qkv.view(B, Hm // ws, ws, Hm // ws, ws, H, 3 * D).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, H, N, 3 * D)
        q, k, v = x.split([D, D, D], -1)
        s = q @ k.transpose(-1, -2) * D ** -0.5 + c["table"].double()[:, A.bias_idxs(ws)][None]
        o = (s.softmax(-1) @ v).view(B, Hm // ws, Hm // ws, H, ws, ws, D).permute(0, 1, 4, 2, 5, 3, 6).reshape(W * N, H * D)
    else:
        x = qkv.view(W, N, 3, H, D).permute(2, 0, 3, 1, 4)
        s = x[0] @ x[1].transpose(-1, -2) * D ** -0.5
        if c["causal"]:
            s = s.masked_fill(torch.triu(torch.ones(N, N, dtype=torch.bool), 1), float("-inf"))
        o = (s.softmax(-1) @ x[2]).permute(0, 2, 1, 3).reshape(W * N, H * D)
    assert float((A.canon_out(c, o) - c["ref"]["out"]).abs().max()) < 1e-12
    dq, dk, dv = A.canon_dqkv(c, c["qkv"])
    assert torch.equal(dq, c["q"]) and torch.equal(dk, c["k"]) and torch.equal(dv, c["v"])
    assert torch.equal(A.canon_out(c, c["dout"]), c["dout_c"])
    lse_flat = torch.zeros(W * N, H, dtype=F64)
    lse_flat[c["idx"].reshape(-1)] = c["ref"]["lse"].permute(0, 2, 1).reshape(W * N, H)
    assert torch.equal(A.canon_lse(c, lse_flat), c["ref"]["lse"])


@pytest.mark.parametrize("shape,cls", [(n, c) for n, s in SHAPES.items() for c in A.classes_for(bool(s.get("ws")), s.get("causal", False))])
def test_written_out_formula_is_autograds(shape, cls):
    """attention_math (forward, recompute-from-lse backward, bias scatter) in fp64 == torch.softmax / logsumexp / autograd in fp64."""
    c = _case(shape, cls)
    auto = A.attention_autograd(c["q"], c["k"], c["v"], c["dout_c"], None if c["table"] is None else c["table"].double(), c["bidx"], c["scale"], c["causal"], F64)
    for name, e in A.errors(c, auto).items():
        assert e["all"] < 1e-11, (name, e)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_class_has_its_property(shape):
    s = SHAPES[shape]
    N, causal = s["N"], s.get("causal", False)
    for cls in A.classes_for(bool(s.get("ws")), causal):
        for storage in ("f32", "bf16"):
            c = _case(shape, cls, storage)
            sc, p = _probs(c)
            info = c["info"]
            if cls in ("late", "early", "masked_spike"):
                assert info["spike_q"], cls
                for i in info["spike_q"]:
                    assert float(p[:, :, i, info["dominant"][i]].min()) >= 0.99, (cls, storage, i)
            if cls == "late":
                assert set(info["dominant"].values()) == {N - 1} and info["stairs"][-1] == (N - 1, 1.0)      # the last key: the last, ragged 16-key tile
                tiles = sorted({key // 64 for key, _ in info["stairs"]})
                assert len(tiles) == min((N + 63) // 64, 4)
                if tiles[0] > 0:
                    tiles = [tiles[0] - 1] + tiles
                for i in info["spike_q"]:      # the running maximum after each 64-key tile strictly grows
                    run = [sc[:, :, i, :min(N, 64 * (t + 1))].amax(-1) for t in tiles]
                    assert all(bool((hi_ > lo_).all()) for lo_, hi_ in zip(run, run[1:])), (storage, i)
            if cls == "early":
                assert set(info["dominant"].values()) == {2}
            if cls in ("shift+", "shift-"):
                centre = 32.0 if cls == "shift+" else -32.0
                fin = sc[torch.isfinite(sc)]
                assert float((fin - centre).abs().max()) <= 8.0, (cls, storage, float(fin.min()), float(fin.max()))
            if cls == "bias_spike":
                hi, lo = info["spike_bias"]
                ws = c["ws"]
                assert float(c["table"].max()) == 24.0 and float(c["table"].min()) == -24.0
                for h in range(c["heads"]):
                    rows = [0, ws - 1, N - ws, N - 1] if h % 2 == 0 else list(range(ws)) + list(range(N - ws, N))
                    for i in rows:
                        j = int((c["bidx"][i] == hi[h]).nonzero().view(-1)[0])
                        assert int((c["bidx"][i] == hi[h]).sum()) == 1                       # one key at that offset: chosen by the gather index alone
                        assert float(p[:, h, i, j].min()) >= 0.99, (h, i, j)
            if cls == "masked_spike":
                raw = c["q"] @ c["k"].transpose(-1, -2) * c["scale"]                         # before the mask
                for i, j in info["masked"].items():
                    assert bool((raw[:, :, i].argmax(-1) == j).all()) and float(raw[:, :, i, j].min()) > 60.0
                    assert float(p[:, :, i, j].max()) == 0.0


def test_f32_yardstick_is_bounded_on_every_case_of_the_gpu_suite():
    """torch's f32 softmax / logsumexp / autograd against fp64 on every f32-storage case of tests/test_gpu_attention_conditioning.py: y(T) <= 1e-5 on all six
    tensors (whole-tensor figure), so no gate is looser than 4e-5 -- within a factor two of the fixed 2e-5 of the older tests.  The rows-of-interest figures
    are printed next to them (a saturated row's dq is noise against ROWS_MIN: not bounded by 1e-5, see attention_cases.ROWS_MIN)."""
    worst = {}
    print()
    for r in A.ROUTES:
        if r["storage"] != "f32":
            continue
        for cls in A.classes_for(r["bias"], r["causal"]):
            c = A.route_case(r, cls)
            _, per = A.yardstick(c, parts=True)
            y = per["f32"]
            print(f"[yardstick f32] {r['name']:24s} {cls:12s} " + "  ".join(
                f"{n} {v['all']:.1e}" + ("" if v["rows"] is None else f" (rows {v['rows']:.1e})") for n, v in y.items()))
            for n, v in y.items():
                assert v["all"] <= 1e-5, (r["name"], cls, n, v)
                worst[cls] = max(worst.get(cls, 0.0), v["all"])
    print("[yardstick f32] worst whole-tensor figure per class: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def _defect_ratio(c, defect, rounded_bias=False):
    """max over tensors and figures of (error of the defective fp64 formula) / gate, and the tensor that has it."""
    bad = A._math(c, defect=defect)
    e, g = A.errors(c, bad), A.gates(c, rounded_bias)
    best = max(((e[n][w] / g[n][w], n) for n in e for w in ("all", "rows") if e[n][w] is not None))
    return best


def test_every_gate_rejects_its_defects():
    print()
    table = {}
    for shape, s in SHAPES.items():
        bias, causal = bool(s.get("ws")), s.get("causal", False)
        for defect in A.DEFECTS:
            if (defect == "mask_off_by_one" and not causal) or (defect == "bias_index" and not bias):
                continue
            for storage in ("f32", "bf16"):
                cells = []
                for cls in A.classes_for(bias, causal):
                    ratio, name = _defect_ratio(_case(shape, cls, storage), defect, rounded_bias=(storage == "bf16" and bias))
                    table[(shape, defect, storage, cls)] = ratio
                    cells.append(f"{cls} {ratio:.1e} ({name})")
                print(f"[defect / gate] {shape:14s} {defect:16s} {storage:5s} " + "  ".join(cells))
    for (shape, defect, storage, cls), ratio in table.items():
        exists = not (defect == "tile_max" and SHAPES[shape]["N"] <= 64)          # one tile has one maximum
        if cls in CATCHES[defect] and exists:
            assert ratio >= 10.0, (shape, defect, storage, cls, ratio)
    for defect, classes in CATCHES.items():          # each defect is caught somewhere at each storage
        for storage in ("f32", "bf16"):
            assert any(r >= 10.0 for (s_, d_, st_, c_), r in table.items() if d_ == defect and st_ == storage and c_ in classes), (defect, storage)
    # what the issue observed: the phantom key is invisible to shift+ everywhere, and inside the bf16 gate on the plain draw of a 14 x 14 window
    for shape in SHAPES:
        for storage in ("f32", "bf16"):
            assert table[(shape, "phantom_key", storage, "shift+")] < 1.0
    assert table[("14x14 hd32", "phantom_key", "bf16", "plain")] < 10.0 and table[("14x14 hd32", "phantom_key", "bf16", "late")] < 10.0
    assert table[("14x14 hd32", "tile_max", "f32", "late")] >= 10.0 and table[("7x7 hd32", "tile_max", "f32", "late")] < 1e-3


# whole-tensor figures of the kernels on an MI355X (tests/test_gpu_attention_conditioning.py) that torch's own f32 order does not explain
MEASURED = [("split_f32_7x7", "early", "dv", 1.3e-6), ("split_f32_14x14", "early", "dk", 7.7e-6), ("stream_f32_hd64_200", "late", "dk", 1.2e-5),
            ("causal_f32_77", "masked_spike", "dk", 5.3e-6), ("dtype3_200", "early", "dk", 9.1e-6)]


def test_documented_operation_order_reproduces_the_kernels_peaked_backward_figures():
    """On the peaked classes every f32 backward kernel is 2 .. 10 x above torch's own f32 error, all routes alike: the exponent is taken in the exp2 domain on an
    argument of magnitude 46 and P is recomputed from the stored f32 lse (attention_cases, ``f32_lse_domain`` / ``f32_split_products``).  The CPU restatement
    of that order reproduces the measured figures: each lies inside the gate it gives and within 4 x of the yardstick itself, where torch's order alone is
    below half of it (on most of them below a tenth)."""
    print()
    for route, cls, name, kernel in MEASURED:
        r = A.ROUTE[route]
        y, per = A.yardstick(A.route_case(r, cls), parts=True, split_products=r["split_products"])
        torch_only, documented = per["f32"][name]["all"], y[name]["all"]
        print(f"[documented order] {route:22s} {cls:12s} {name}: kernel {kernel:.1e}  torch f32 {torch_only:.1e}  documented order {documented:.1e}")
        assert kernel <= A.FACTOR * documented and documented <= A.FACTOR * kernel, (route, cls, name, kernel, documented)
        assert 2.0 * torch_only < kernel, (route, cls, name, kernel, torch_only)
