"""Cases of the long-sequence 16-bit-MFMA attention forward (include/gg_attn16.h) shared by tests/test_attention16_cpu.py and tests/test_gpu_attention16.py, and a
torch restatement of the kernel's arithmetic contract.  Plain torch on the CPU: no GPU, no libgg.

Sizes: a single key (1); an exact and a ragged 16-key sub-tile (16, 17); the 64-key tile edge from both sides (63, 64, 65); one live row in the last tile (257
and 577, the production length of CLIP ViT-L/14-336); a whole number of tiles (320).  Classes: every class of ``attention_cases.classes_for(False, False)``; a
single key has no other key to be peaked against, so N = 1 runs ``plain`` only."""
import math

import torch

from tests import attention_cases as AC

SIZES = (1, 16, 17, 63, 64, 65, 257, 320, 577)
STORAGES = ("f16", "bf16")
TILE = 64
LOG2E = 1.4426950408889634


def params():
    """[(storage, N, class)] of the conditioning cases."""
    return [(s, N, c) for s in STORAGES for N in SIZES for c in AC.classes_for(False, False) if N > 1 or c == "plain"]


def get_case(storage, N, cls):
    return AC.case("clip", N, 64, heads=2, windows=2, storage=storage, cls=cls)


def tiled_contract(c, tile=TILE):
    """The contract of include/gg_attn16.h in f32 arithmetic on the case's canonical (storage-rounded) q, k, v: scores with f32 accumulation scaled into the exp2
    domain, online softmax over ``tile``-key tiles with a running maximum, the row sum from the unrounded P, P rounded to the storage type per tile as the operand
    of P V, O accumulated in f32 (rescaled when the maximum moves) and rounded once after the division, lse = m ln 2 + log l.  Returns canonical out, lse."""
    st = c["dtype"]
    q, k, v = (c[n].float() for n in ("q", "k", "v"))
    sc2 = float(torch.tensor(c["scale"] * LOG2E, dtype=torch.float32))
    s = (q @ k.transpose(-1, -2)) * sc2
    N = s.shape[-1]
    m = torch.full(s.shape[:-1] + (1,), -1e30)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for t in range(0, N, tile):
        st_ = s[..., t:t + tile]
        mn = torch.maximum(m, st_.amax(-1, keepdim=True))
        alpha = torch.exp2(m - mn)
        p = torch.exp2(st_ - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(st).float() @ v[..., t:t + tile, :]
        m = mn
    out = (o / l).to(st)
    lse = (m * 0.6931471805599453 + torch.log(l)).squeeze(-1)
    return {"out": out.double(), "lse": lse.double()}


def integer_case(N, storage, heads=2, windows=2, seed=0):
    """Canonical q, k in {-1, 0, 1} and v in {-8 .. 8} (every product and every partial sum exact in either storage type), flattened to the clip layout."""
    g = torch.Generator().manual_seed(1000 * N + seed)
    q = torch.randint(-1, 2, (windows, heads, N, 64), generator=g).double()
    k = torch.randint(-1, 2, (windows, heads, N, 64), generator=g).double()
    v = torch.randint(-8, 9, (windows, heads, N, 64), generator=g).double()
    return q, k, v


def half_ulp(x, dtype):
    """Bound of ONE rounding of x (fp64, normal range) to ``dtype``: half a unit in the last place, |x| 2^-p at most (p = 11 fp16, 8 bf16), with 2^-10 of it on
    top for the f32 division in front of the rounding (a double rounding moves a result by at most the f32 ulp, 2^-13 of a bf16 / 2^-12 of an fp16 half-ulp)."""
    return x.abs() * (2.0 * AC.FLOOR[dtype]) * (1.0 + 2.0 ** -10)


def one_hot_case(N, heads=2, windows=2, seed=0):
    """Keys of +-1 entries, query i equal to key sel(i) = (7 i + 3) mod N: its score is 64, every other key's a sum of 64 random signs.  With ``scale`` = 8 the
    other keys' P underflow to exactly 0 in f32 (asserted by the caller through ``margin``), so out[i] must be v[sel(i)] bit for bit."""
    g = torch.Generator().manual_seed(2000 * N + seed)
    k = (torch.randint(0, 2, (windows, heads, N, 64), generator=g) * 2 - 1).double()
    v = torch.randint(-8, 9, (windows, heads, N, 64), generator=g).double()
    sel = (7 * torch.arange(N) + 3) % N
    q = k[:, :, sel]
    s = q @ k.transpose(-1, -2)
    other = s.masked_fill(torch.nn.functional.one_hot(sel, N).bool(), -math.inf)
    margin = 64.0 - float(other.max()) if N > 1 else math.inf
    return q, k, v, sel, margin


def flat_qkv(q, k, v, layout, dtype, pad=0):
    """(tokens, 3 * heads * 64 [+ pad]) buffer in ``layout`` ("clip": [q | k | v] column blocks; "tinyvit": per-head interleaved [q | k | v]) and the column
    keywords of the entry point.  The pad columns hold NaN: nothing may read them."""
    W, H, N, D = q.shape
    q_off, k_off, v_off, hs = AC.columns(layout, H, D)
    c = dict(head_stride=hs, idx=AC.token_index("clip", N, W, 0, 0))
    buf = torch.full((W * N, 3 * H * D + pad), float("nan"), dtype=torch.float64)
    for x, off in ((q, q_off), (k, k_off), (v, v_off)):
        AC._flat(c, x, off, into=buf)
    kw = dict(num_windows=W, tokens_per_window=N, num_heads=H, q_off=q_off, k_off=k_off, v_off=v_off, head_stride=hs)
    return buf.to(dtype), kw
