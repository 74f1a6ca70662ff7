"""Cases of the 16-bit-MFMA window attention forward beyond 256 tokens (include/gg_attn16w.h) shared by tests/test_attention16_win_cpu.py and
tests/test_gpu_attention16_win.py; the torch restatement of the kernel's arithmetic contract is tests/attention16_cases.py::tiled_contract (with the bias).  Plain
torch on the CPU: no GPU, no libgg.

Sizes ``(ws, m, W)``: window side, map side in windows, windows.  A single key (1); an exact and a ragged 16-key sub-tile (4, 5; the latter with four windows per
image); exactly one 64-key tile over two images of four windows (8); a second, ragged tile (9); four tiles, the last size TinyViT's route does not take (16); 289
tokens, the smallest it takes, gathered from a 2 x 2 map (17); 576 and 1024 tokens, tiny_vit_21m_384 / _512 (24, 32: the limit of the bias table).  Classes: every
class of ``attention_cases.classes_for(True, False)`` -- ``bias_spike`` included --; a single key has no other key to be peaked against, so ws = 1 runs ``plain``
only."""
import math

import torch

from tests import attention_cases as AC
from tests.attention16_cases import tiled_contract          # noqa: F401  (one restatement serves both entry points: a case without a table takes its no-bias branch)

SIZES = ((1, 1, 2), (4, 1, 2), (5, 2, 4), (8, 2, 8), (9, 1, 2), (16, 1, 2), (17, 2, 4), (24, 1, 2), (32, 1, 2))
GEOM = {ws: (m, W) for ws, m, W in SIZES}
TILE = 64
HD = 32
LOG2E = 1.4426950408889634


def params():
    """[(ws, class)] of the conditioning cases."""
    return [(ws, c) for ws, _, _ in SIZES for c in AC.classes_for(True, False) if ws > 1 or c == "plain"]


def get_case(ws, cls):
    m, W = GEOM[ws]
    return AC.case("tinyvit", ws * ws, HD, heads=2, windows=W, ws=ws, storage="bf16", cls=cls, map_hw=m * ws)


def flat_qkv(q, k, v, ws, m, layout="tinyvit", pad=0):
    """Canonical (windows, heads, ws * ws, 32) q, k, v -> the bf16 (tokens, 3 * heads * 32 [+ pad]) buffer of an m x m-window map in ``layout`` ("tinyvit": per-head
    interleaved [q | k | v]; "clip": [q | k | v] column blocks), the keywords of ops.attention_flash16_win, and the (windows, N) row index.  The pad columns hold
    NaN: nothing may read them."""
    W, H, N, D = q.shape
    assert N == ws * ws and D == HD and W % (m * m) == 0
    q_off, k_off, v_off, hs = AC.columns(layout, H, D)
    idx = AC.token_index("tinyvit", N, W, ws, m * ws)
    c = dict(head_stride=hs, idx=idx)
    buf = torch.full((W * N, 3 * H * D + pad), float("nan"), dtype=torch.float64)
    for x, off in ((q, q_off), (k, k_off), (v, v_off)):
        AC._flat(c, x, off, into=buf)
    kw = dict(num_windows=W, tokens_per_window=N, num_heads=H, q_off=q_off, k_off=k_off, v_off=v_off, head_stride=hs, window_size=ws, map_h=m * ws, map_w=m * ws)
    return buf.to(torch.bfloat16), kw, idx


def canon(idx, flat, heads):
    """(tokens, heads * d) -> (windows, heads, N, d) fp64 on the CPU; (tokens, heads) -> (windows, heads, N)."""
    f = flat.detach().double().cpu()[idx]                                          # (W, N, heads * d)
    W, N = idx.shape
    if f.shape[-1] == heads:
        return f.permute(0, 2, 1).contiguous()
    return f.view(W, N, heads, -1).permute(0, 2, 1, 3).contiguous()


def half_ulp(x):
    """Bound of ONE rounding of x (fp64, normal range) to bf16 after the f32 division: tests/attention16_cases.py::half_ulp."""
    from tests.attention16_cases import half_ulp as h
    return h(x, torch.bfloat16)


def integer_case(ws, W, heads=2, seed=0):
    """Canonical q, k in {-1, 0, 1} and v in {-8 .. 8}: every product and every partial sum exact."""
    N = ws * ws
    g = torch.Generator().manual_seed(1000 * N + seed)
    q = torch.randint(-1, 2, (W, heads, N, HD), generator=g).double()
    k = torch.randint(-1, 2, (W, heads, N, HD), generator=g).double()
    v = torch.randint(-8, 9, (W, heads, N, HD), generator=g).double()
    return q, k, v


def mask_sets(ws):
    """S_h per head: the (|dy|, |dx|) entries whose bias is 0 (every other entry is -200).  (0, 0) is in both; the sets are not symmetric in (dy, dx), so a
    transposed gather is another set."""
    return [[(0, 0), (0, 1), (2, 0), (ws - 1, ws - 2)], [(0, 0), (1, 3), (0, ws - 1), (3, 0), (ws - 2, 1)]]


def mask_case(ws, W, seed=0):
    """q = 0, integer v, and per head a table that is 0 on ``mask_sets`` and -200 elsewhere: every P is exactly 1 or exactly 0 (exp2(-200 log2 e) underflows to 0 in
    f32, and the query's own key -- offset (0, 0) -- holds the maximum at 0), so out[q] is the mean of v over the keys whose offset from q is in S_h and lse the
    log of their number.  Returns q, k, v, table (heads, ws * ws) f32, mean (W, heads, N, 32) fp64, count (heads, N)."""
    N = ws * ws
    g = torch.Generator().manual_seed(3000 * N + seed)
    q = torch.zeros(W, 2, N, HD, dtype=torch.float64)
    k = torch.randint(-1, 2, (W, 2, N, HD), generator=g).double()
    v = torch.randint(-8, 9, (W, 2, N, HD), generator=g).double()
    table = torch.full((2, N), -200.0)
    for h, S in enumerate(mask_sets(ws)):
        for dy, dx in S:
            table[h, dy * ws + dx] = 0.0
    keep = (table[:, AC.bias_idxs(ws)] == 0).double()                              # (heads, N, N)
    count = keep.sum(-1)
    mean = (keep[None] @ v) / count[None, :, :, None]
    return q, k, v, table, mean, count


ONE_HOT_SCALE = 32.0
ONE_HOT_SEED = {9: 0, 17: 0, 32: 0}


def one_hot_case(ws, W=2, heads=2):
    """Keys of +-1 entries (head dim 32), query i equal to key sel(i) = (7 i + 3) mod N: its score is 32, every other key's a sum of 32 random signs.  With
    ``scale`` = 32 and a margin of 4 the other keys' P underflow to exactly 0 in f32 (4 * 32 * log2 e = 184 > 150; asserted by the caller), so out[i] must be
    v[sel(i)] bit for bit.  The seeds are ones for which the margin holds."""
    N = ws * ws
    g = torch.Generator().manual_seed(2000 * N + ONE_HOT_SEED[ws])
    k = (torch.randint(0, 2, (W, heads, N, HD), generator=g) * 2 - 1).double()
    v = torch.randint(-8, 9, (W, heads, N, HD), generator=g).double()
    sel = (7 * torch.arange(N) + 3) % N
    q = k[:, :, sel]
    s = q @ k.transpose(-1, -2)
    other = s.masked_fill(torch.nn.functional.one_hot(sel, N).bool(), -math.inf)
    margin = float(HD) - float(other.max())
    return q, k, v, sel, margin
