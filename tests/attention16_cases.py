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
    """The contract of include/gg_attn16.h and include/gg_attn16w.h in f32 arithmetic on the case's canonical (storage-rounded) q, k, v and its f32 table (if any):
    scores with f32 accumulation taken into the exp2 domain as acc * (scale log2 e), with a table + table[|dy| ws + |dx|] log2 e (one FMA; the table unrounded),
    online softmax over ``tile``-key tiles with a running maximum the bias has joined, the row sum from the unrounded P, P rounded to the storage type per tile as
    the operand of P V, O accumulated in f32 (rescaled when the maximum moves) and rounded once after the division, lse = m ln 2 + log l.  ``c``: a case of
    ``attention_cases.case`` or a dict with dtype, q, k, v, scale and (optional) table, bidx.  Returns canonical out, lse."""
    st = c["dtype"]
    q, k, v = (c[n].float() for n in ("q", "k", "v"))
    sc2 = float(torch.tensor(c["scale"] * LOG2E, dtype=torch.float32))
    qk = q @ k.transpose(-1, -2)
    table = c.get("table")
    if table is None:
        s = qk * sc2
    else:
        bias2 = (table.float() * torch.tensor(LOG2E, dtype=torch.float32))[:, c["bidx"]]      # (H, N, N), the f32 product the kernel stages
        s = (qk.double() * sc2 + bias2.double()).float()                                        # one rounding: an FMA
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


# ------------------------------------------------------------------------------------------- the bits of the build before the two kernels became one
# tests/golden/attention16_parent.npz (tools/make_attention16_parent_golden.py) holds out and lse of these calls from the build with one translation unit per head
# dim; the smallest shapes at which each mechanism of the kernel is live.
# linear, head dim 64, 2 sequences x 2 heads, (N, layout, row pad, lse given): 17 a ragged 16-key sub-tile and one wave partly live; 65 a second, ragged key tile,
# also interleaved with rows only 8-byte aligned; 130 a second query tile with two live rows, three key tiles
PARENT_LINEAR = ((17, "clip", 0, True), (65, "clip", 0, False), (65, "tinyvit", 4, False), (130, "clip", 0, True))
# window, head dim 32, bf16, 2 heads, (ws, map side in windows, windows, layout, row pad), each with a random f32 table and without: 5 a ragged sub-tile gathered
# across a 2 x 2 map; 9 a second ragged tile, a 16-query strip straddling a window row, also [q | k | v] with rows only 8-byte aligned; 12 a second query tile
PARENT_WINDOW = ((5, 2, 4, "tinyvit", 0), (9, 1, 2, "tinyvit", 0), (9, 1, 2, "clip", 4), (12, 1, 2, "tinyvit", 0))


def parent_bits(ops, window):
    """{name: numpy array} of the PARENT_WINDOW (``window``) or PARENT_LINEAR calls on seeded N(0, 1) inputs, run on the GPU through ``ops`` (geoguessr_ai_amd.ops):
    ``<name>_out`` the int16 view of out, ``<name>_lse`` the f32 lse where the call takes one."""
    from tests import attention16_win_cases as W16
    store = {}

    def keep(name, res, want_lse):
        out, lse = res if want_lse else (res, None)
        store[name + "_out"] = out.view(torch.int16).cpu().numpy()
        if want_lse:
            store[name + "_lse"] = lse.cpu().numpy()

    if not window:
        for storage, st in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            for N, layout, pad, want_lse in PARENT_LINEAR:
                g = torch.Generator().manual_seed(7000 + N)
                q, k, v = (torch.randn(2, 2, N, 64, generator=g).to(st).double() for _ in range(3))
                qkv, kw = flat_qkv(q, k, v, layout, st, pad=pad)
                keep(f"lin_{storage}_{N}_{layout}{pad}", ops.attention_flash16(qkv.cuda()[:, :384], **kw, want_lse=want_lse), want_lse)
        return store
    for ws, m, W, layout, pad in PARENT_WINDOW:
        g = torch.Generator().manual_seed(7100 + ws)
        q, k, v = (torch.randn(W, 2, ws * ws, 32, generator=g).to(torch.bfloat16).double() for _ in range(3))
        table = (0.5 * torch.randn(2, ws * ws, generator=g)).float().cuda()
        qkv, kw, _ = W16.flat_qkv(q, k, v, ws, m, layout=layout, pad=pad)
        for name, tab in (("bias", table), ("nobias", None)):
            keep(f"win_{ws}_{layout}{pad}_{name}", ops.attention_flash16_win(qkv.cuda()[:, :192], **kw, bias_table=tab, want_lse=True), True)
    return store
