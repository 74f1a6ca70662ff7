"""Shapes, inputs and the CPU restatement of the fixed-order bias gradient (include/gg_attn_dbias.h, csrc/attention_dbias.hip).  Plain torch / numpy on the CPU:
no GPU, no libgg.  Operands, fp64 references and gates are those of tests/attention_cases.py (the canonical tensors of a case do not depend on the map the
windows are cut from, so the 14 x 7 map of the 7 x 7 shape -- which ``attention_cases.case`` does not draw itself -- reuses the case of the same window count
with a token index of its own).

``bin_walk`` restates which (query, key) pairs fall into which bin and in which order the kernel adds them: workgroup, wave (strip mod 4), 64-key tile, query
row, key row (issued in pairs), lane = (side, |dx|), then the eight tables in (wave, side) order.  On an integer-valued dS every order gives the same sum, so it
must equal the gather-index sum exactly; ``bin_walk`` also returns how often every pair was visited (exactly once)."""
import numpy as np
import torch

from tests import attention_cases as AC

WAVES, KT, GROUPS_MAX, REDUCE_SLICES = 4, 64, 512, 64

# name: (ws, heads, windows, map_h, map_w) -- the issue's table: 7 x 7 on a 14 x 7 map (map_h != map_w, two windows per image, two images, 49 -> 64 padded
# tokens); 12 x 12 (144 tokens, no padding); 14 x 14 (196 -> 208); 17 x 17 (odd side, beyond 256 tokens; 2 x 2 windows per image); 32 x 32 (1024 bins, key tiling)
SHAPES = {
    "7x7": (7, 2, 4, 14, 7),
    "12x12": (12, 2, 2, 12, 12),
    "14x14": (14, 2, 2, 14, 14),
    "17x17": (17, 2, 4, 34, 34),
    "32x32": (32, 2, 1, 32, 32),
}
# peaked (late / early: one key dominates, in the last ragged tile or in the first), shifted (every score +-32) and the class whose dominant key is chosen by
# the gather index alone; `plain` is the control.  1024 tokens take one class per family (their fp64 references and yardsticks are the slow part of a case).
CLASSES = {n: ("late", "shift-", "bias_spike") if n == "32x32" else AC.classes_for(True, False) for n in SHAPES}


def token_index(N, windows, ws, map_h, map_w):
    """(windows, N) row of the flat NHWC buffer for every (window, token): AC.token_index for a map that need not be square."""
    ny, nx = map_h // ws, map_w // ws
    per = ny * nx
    assert windows % per == 0
    return torch.arange(windows * N).view(windows // per, ny, ws, nx, ws).permute(0, 1, 3, 2, 4).reshape(windows, N)


def case(name, storage, cls):
    """The attention_cases case of a shape (canonical tensors, fp64 reference, yardsticks) with the flat qkv / dout of ITS map and its geometry keywords."""
    ws, heads, windows, map_h, map_w = SHAPES[name]
    N = ws * ws
    base = AC.case("tinyvit", N, 32, heads, windows, ws, False, storage, cls, map_h if map_h == map_w else max(map_h, map_w))
    if map_h == map_w:
        return base
    c = dict(base)
    c["idx"] = token_index(N, windows, ws, map_h, map_w)
    qkv = torch.zeros(windows * N, 3 * heads * 32, dtype=AC.F64)
    for x, off in ((c["q"], c["q_off"]), (c["k"], c["k_off"]), (c["v"], c["v_off"])):
        AC._flat(c, x, off, into=qkv)
    c["qkv"] = qkv.to(c["dtype"])
    c["dout"] = AC._flat(c, c["dout_c"]).to(c["dtype"])
    c["kw"] = dict(base["kw"], map_h=map_h, map_w=map_w)
    return c


def groups(num_windows):
    return min(num_windows, GROUPS_MAX)


def rows(num_windows):
    """gg_attention_dbias_rows: one partial row per window group plus the rows the second stage folds into."""
    return groups(num_windows) + REDUCE_SLICES


def bin_walk(ds, ws):
    """ds: (windows, N, N) array of ONE head.  Returns (table (ws * ws,) float64 summed in the kernel's order of adds, visits (windows, N, N) int)."""
    W, N, _ = ds.shape
    assert N == ws * ws
    G = groups(W)
    nstrip = (N + 15) // 16
    lanes = np.arange(64)
    side, adx = lanes >> 5, lanes & 31
    visits = np.zeros((W, N, N), dtype=np.int64)
    total = np.zeros(ws * ws)
    for g in range(G):
        bins = np.zeros((WAVES, 2, ws * ws))
        for w in range(g, W, G):
            for s in range(nstrip):
                wave = s % WAVES
                nq = min(16, N - 16 * s)
                for k0 in range(0, N, KT):
                    kend = min(k0 + KT, N)
                    r0, r1 = k0 // ws, (kend - 1) // ws
                    for q in range(nq):
                        t = 16 * s + q
                        ty, tx = divmod(t, ws)
                        kx = np.where(side == 1, tx + adx, tx - adx)
                        okx = (adx < ws) & (kx >= 0) & (kx < ws) & ((side == 0) | (adx > 0))
                        for ky in range(r0, r1 + 1):        # (the kernel issues rows ky, ky + 1 together: distinct |dy|, so the same adds in the same order)
                            k = ky * ws + kx
                            ok = okx & (k >= k0) & (k < kend)
                            b = abs(ty - ky) * ws + adx[ok]
                            assert len(set(zip(side[ok], b))) == int(ok.sum())      # no two lanes of an instruction on one bin of one table
                            np.add.at(bins, (wave, side[ok], b), ds[w, t, k[ok]])
                            np.add.at(visits, (w, t, k[ok]), 1)
        for wv in range(WAVES):
            for sd in range(2):
                total += bins[wv, sd]
    return total, visits
