"""Cases of the 16-bit-MFMA window attention backward beyond 256 tokens (include/gg_attn16wb.h) shared by tests/test_attention16_win_bwd_cpu.py and
tests/test_gpu_attention16_win_bwd.py, and a torch restatement of the kernel's arithmetic contract.  Plain torch on the CPU: no GPU, no libgg.

Sizes ``(ws, m, W)``: those of tests/attention16_win_cases.py -- a single key (1); an exact and a ragged 16-strip (4, 5; the latter with four windows per image);
exactly one 64 tile (8); a ragged second tile (9); 256 tokens, two whole 128 blocks (16); 289 = two blocks + 33 rows, gathered from a 2 x 2 map (17); 576 = 4.5
blocks (24); 1024, the limit of the bias table (32).  Classes: every class of ``attention_cases.classes_for(True, False)``; ws = 1 runs ``plain`` only.  Storage
is bf16, the head dim 32.

Two exact families (every expected value is bf16- / f32-representable, so the comparison is bit for bit, dbias included):

* one-hot rows (``attention16_win_cases.one_hot_case`` with an integer ``dout`` and a zero table): P is 1 on key sel(i) after its rounding to bf16 and exactly 0
  elsewhere, so dv[sel(i)] = dout[i]; delta_i = dout[i] . v[sel(i)] = dP[i][sel(i)] exactly, so dS = 0 exactly: dq = dk = 0 and dbias = 0;
* two-hot rows at ws = 8 (``two_hot_case``): P is exactly 1/2 on two keys; the closed form is in its docstring."""
import math

import torch

from tests import attention16_bwd_cases as B
from tests import attention16_win_cases as WC
from tests import attention_cases as AC

SIZES = WC.SIZES
GEOM = WC.GEOM
ONE_HOT_SIZES = (9, 17, 32)
TILE = 64
HD = 32
LOG2E = 1.4426950408889634
BF16 = torch.bfloat16
F32 = torch.float32
TENSORS = ("dq", "dk", "dv", "dbias")


def params():
    """[(ws, class)] of the conditioning cases."""
    return WC.params()


def get_case(ws, cls):
    return WC.get_case(ws, cls)          # (the forward's cases: computed once for both files)


def kw_of(c):
    return {k: v for k, v in c["kw"].items() if k != "head_dim"}


def tiled_contract_bwd(c, out, lse, tile=TILE):
    """The contract of include/gg_attn16wb.h in f32 arithmetic on canonical bf16-representable q, k, v, dout (``c``: a case of ``attention_cases.case`` or a dict
    with q, k, v, dout_c, scale and, optionally, table (heads, ws * ws) f32 and bidx), the forward's canonical ``out`` (bf16 values) and ``lse``: per ``tile``-key
    tile S with f32 accumulation, P = exp2(fma(S, scale log2 e, b2 + nl)) with b2 = table[|dy| ws + |dx|] log2 e (an f32 product; 0 without a table),
    nl = -lse log2 e (an f32 product) and b2 + nl an f32 sum -- no maximum is subtracted again --, dP = dO V^T, delta = sum_d dO O in f32, dS = P (dP - delta), P
    and dS rounded to bf16 as the operands of dV = P^T dO, dK = dS^T Q, dQ = dS K, f32 accumulators, dq and dk times ``scale`` in f32, one rounding to bf16;
    dbias[h][|dy| ws + |dx|] = the sum over windows, queries and keys of the UNROUNDED f32 dS (summed here in fp64: the kernel's order is not fixed).  Returns
    canonical dq, dk, dv (fp64 holding bf16 values) and dbias (fp64; None without a table)."""
    q, k, v, do = (c[n].to(F32) for n in ("q", "k", "v", "dout_c"))
    o = out.to(F32)
    sc2 = float(torch.tensor(c["scale"] * LOG2E, dtype=F32))
    scale = float(torch.tensor(c["scale"], dtype=F32))
    nl = (lse.to(F32) * torch.tensor(-LOG2E, dtype=F32))[..., None]                  # -lse log2 e, one f32 rounding
    table = c.get("table")
    b2 = None if table is None else (table.to(F32) * torch.tensor(LOG2E, dtype=F32))[:, c["bidx"]]      # (H, N, N)
    delta = (do * o).sum(-1, keepdim=True)
    N = q.shape[-2]
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    dsf = torch.zeros(q.shape[:-1] + (N,), dtype=torch.float64)
    for t in range(0, N, tile):
        kt, vt = k[..., t:t + tile, :], v[..., t:t + tile, :]
        s = q @ kt.transpose(-1, -2)
        add = nl if b2 is None else b2[..., t:t + tile] + nl                        # one f32 rounding
        p = torch.exp2((s.double() * sc2 + add.double()).to(F32))                   # one rounding: an FMA
        ds = p * (do @ vt.transpose(-1, -2) - delta)
        dsf[..., t:t + tile] = ds.double()
        pb, dsb = p.to(BF16).to(F32), ds.to(BF16).to(F32)
        dv[..., t:t + tile, :] = pb.transpose(-1, -2) @ do
        dk[..., t:t + tile, :] = dsb.transpose(-1, -2) @ q
        dq += dsb @ kt
    r = lambda x: x.to(BF16).double()
    dbias = None
    if table is not None:
        H, T = table.shape
        dbias = torch.zeros(H, T, dtype=torch.float64).index_add_(1, c["bidx"].reshape(-1), dsf.sum(0).reshape(H, -1))
    return {"dq": r(dq * scale), "dk": r(dk * scale), "dv": r(dv), "dbias": dbias}


def check(c, got, label, tensors=TENSORS):
    """``attention_cases.check`` on dq, dk, dv, dbias: e <= 4 max(yardstick, floor).  A single key (ws = 1) has dS = 0 in exact arithmetic, so the fp64 dq, dk and
    dbias are exactly zero and their relative figure is 0 / 0 for any kernel: there dv goes through the gate, dq and dk take
    ``attention16_bwd_cases.check``'s absolute bound, and dbias -- the sum over the windows of the unrounded dS = P (dP - delta), P = 1 -- is held to the f32
    rounding of the two sums whose difference it is: windows * 2^-24 * 32 terms * max |dout| max |v| (the two sums run in different orders)."""
    got = {n: t for n, t in got.items() if n in tensors and t is not None}
    if c["N"] > 1:
        return AC.check(c, got, label, tensors=tensors)
    bad = B.check(c, {n: got[n] for n in ("dq", "dk", "dv")}, label)
    if "dbias" in got:
        assert float(c["ref"]["dbias"].abs().max()) == 0.0
        e = float(got["dbias"].abs().max())
        bound = c["windows"] * AC.FLOOR[F32] * c["hd"] * float(c["dout_c"].abs().max()) * float(c["v"].abs().max())
        print(f"[{label}] max |dbias| {e:.1e} (reference 0; bound {bound:.1e})")
        if not e <= bound:
            bad.append(("dbias", "abs", e, bound))
    return bad


def flat_inputs(c, ws, m, layout="tinyvit", pad=0):
    """qkv (tokens, 192 + pad), dout (tokens, 64) in bf16, the keywords and the (windows, N) row index for a dict of canonical q, k, v, dout_c (2 heads) on an
    m x m-window map."""
    qkv, kw, idx = WC.flat_qkv(c["q"], c["k"], c["v"], ws, m, layout, pad=pad)
    return qkv, AC._flat(dict(idx=idx), c["dout_c"]).to(BF16), kw, idx


def flat_out(idx, x):
    """canonical (windows, heads, N, d) -> (tokens, heads * d); (windows, heads, N) -> (tokens, heads).  fp64."""
    if x.dim() == 3:
        f = torch.zeros(idx.numel(), x.shape[1], dtype=torch.float64)
        f[idx.reshape(-1)] = x.permute(0, 2, 1).reshape(-1, x.shape[1]).double()
        return f
    return AC._flat(dict(idx=idx), x.double())


def canon(idx, heads, layout, dqkv):
    """dq, dk, dv in canonical form from a flat (tokens, >= 3 * heads * 32) result in ``layout``."""
    q_off, k_off, v_off, hs = AC.columns(layout, heads, HD)
    cc = dict(idx=idx, heads=heads, hd=HD, head_stride=hs, q_off=q_off, k_off=k_off, v_off=v_off)
    return dict(zip(("dq", "dk", "dv"), AC.canon_dqkv(cc, dqkv)))


def one_hot_bwd_case(ws):
    """``attention16_win_cases.one_hot_case(ws)`` on the size's own map (``GEOM``) with an integer ``dout`` in -8 .. 8, a zero table and the expected gradients:
    dv[sel(i)] = dout[i] (sel is a bijection: gcd(7, N) = 1), dq = dk = 0, dbias = 0.  Asserts the margin premise: with ``scale`` = 32 a margin of 4 puts every
    other key's exponent 4 * 32 * log2 e = 184 > 150 below the selected one's, so its P is exactly 0 in f32."""
    m, W = GEOM[ws]
    N = ws * ws
    q, k, v, sel, margin = WC.one_hot_case(ws, W=W)
    assert math.gcd(7, N) == 1 and margin >= 4 and margin * WC.ONE_HOT_SCALE * LOG2E > 150
    g = torch.Generator().manual_seed(3000 + N)
    dout = torch.randint(-8, 9, q.shape, generator=g).double()
    dv = torch.zeros_like(v)
    dv[:, :, sel] = dout
    table = torch.zeros(2, N, dtype=F32)
    return dict(q=q, k=k, v=v, dout_c=dout, scale=WC.ONE_HOT_SCALE, dtype=BF16, sel=sel, margin=margin, N=N, ws=ws, m=m, windows=W, table=table,
                bidx=AC.bias_idxs(ws), out=v[:, :, sel],
                want={"dq": torch.zeros_like(q), "dk": torch.zeros_like(k), "dv": dv, "dbias": torch.zeros(2, N, dtype=torch.float64)})


def hadamard32():
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < 32:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


# scale 8 (lse = 256 + ln 2).  With 16 (512 + ln 2) no f32 lse within 16 ulps makes the exponent exactly -1: the product lse * -log2 e steps over the one f32
# value 32 * f32(16 log2 e) + 1 calls for, so P would be 1/2 (1 +- 4e-5) and the unrounded dS behind dbias inexact; ``_two_hot_lse`` asserts the premise
TWO_HOT_SCALE = 8.0


def _two_hot_lse(scale):
    """The f32 value nearest 32 scale + ln 2 for which the contract's P of a score-32 key is EXACTLY 1/2: fma(32, f32(scale log2 e), f32(lse * -log2 e)) = -1.  The
    products' roundings decide which neighbours qualify, so the few f32 values around it are tried; the premise is asserted."""
    sc2 = torch.tensor(scale * LOG2E, dtype=F32)
    x = torch.tensor(32.0 * scale + math.log(2.0), dtype=F32)
    cands = [x.clone()]
    up, down = x.clone(), x.clone()
    for _ in range(16):
        up = torch.nextafter(up, torch.tensor(math.inf, dtype=F32))
        down = torch.nextafter(down, torch.tensor(-math.inf, dtype=F32))
        cands += [up.clone(), down.clone()]
    for l in cands:
        nl = l * torch.tensor(-LOG2E, dtype=F32)
        if float((32.0 * sc2.double() + nl.double()).to(F32)) == -1.0:
            return float(l)
    raise AssertionError("no f32 lse near 32 scale + ln 2 gives P = 1/2 exactly: change TWO_HOT_SCALE")


def two_hot_case(ws=8, m=2, W=4, heads=2):
    """N = 64 tokens per window on a map of m x m windows.  Keys: the 64 vectors {rows of the Sylvester Hadamard matrix H32, their negatives} (pairwise scores
    32, 0 or -32); query i = k[i] + k[b(i)], b(i) = (i + 5) mod 64: its score is 32 on keys i and b(i) and at most 0 elsewhere, so with ``scale`` = 8 (margin
    256), a zero table and lse GIVEN as the f32 value at 256 + ln 2 that makes the exponent exactly -1 (``_two_hot_lse``), P is exactly 1/2 on the two and 0 on the
    rest.  v integer in -8 .. 8, dout one +-1 per row (column c_i, sign s_i).  The closed form of ``attention16_bwd_cases.two_hot_case`` with 32 in place of 64,
    all bf16-exact:
      out[i] = (v[i] + v[b]) / 2;  dP[i][j] = s_i v[j][c_i];  delta_i = s_i (v[i][c_i] + v[b][c_i]) / 2;
      dS[i][i] = s_i (v[i][c_i] - v[b][c_i]) / 4 = -dS[i][b]   (a quarter-integer of magnitude <= 4);
      dq[i] = 8 dS[i][i] (k[i] - k[b]);  dk[j] = 8 (dS[j][j] q[j] + dS[a][j] q[a]) with b(a) = j;  dv[j] = (dout[j] + dout[a]) / 2;
      dbias = index_add of dS over ``attention_cases.bias_idxs(8)``, summed over the windows: sums of quarter-integers, every partial sum exact in f32, so the
      order of the kernel's adds does not matter."""
    N = ws * ws
    assert N == 64 and W % (m * m) == 0
    g = torch.Generator().manual_seed(4000 + N)
    h = hadamard32()
    keys = torch.cat([h, -h])
    k = keys.expand(W, heads, N, HD).clone()
    b = (torch.arange(N) + 5) % N
    q = k + k[:, :, b]
    v = torch.randint(-8, 9, (W, heads, N, HD), generator=g).double()
    col = torch.randint(0, HD, (W, heads, N), generator=g)
    sign = (torch.randint(0, 2, (W, heads, N), generator=g) * 2 - 1).double()
    dout = torch.zeros_like(v).scatter_(-1, col[..., None], sign[..., None])
    s = q @ k.transpose(-1, -2)
    two = torch.zeros(N, N, dtype=torch.bool)
    two[torch.arange(N), torch.arange(N)] = True
    two[torch.arange(N), b] = True
    assert bool((s[..., two] == 32).all()) and float(s.masked_fill(two, -math.inf).max()) <= 0
    out = (v + v[:, :, b]) / 2
    vc = torch.gather(v, -1, col[..., None]).squeeze(-1)                            # v[i][c_i]
    vbc = torch.gather(v[:, :, b], -1, col[..., None]).squeeze(-1)                  # v[b(i)][c_i]
    dsa = sign * (vc - vbc) / 4                                                     # dS[i][i]; dS[i][b(i)] = -dsa
    ds = torch.zeros(W, heads, N, N, dtype=torch.float64)
    ds[..., torch.arange(N), torch.arange(N)] = dsa
    ds[..., torch.arange(N), b] = -dsa
    p = two.double() / 2
    bidx = AC.bias_idxs(ws)
    dbias = torch.zeros(heads, N, dtype=torch.float64).index_add_(1, bidx.reshape(-1), ds.sum(0).reshape(heads, -1))
    want = {"dq": TWO_HOT_SCALE * ds @ k, "dk": TWO_HOT_SCALE * ds.transpose(-1, -2) @ q, "dv": p.t() @ dout, "dbias": dbias}
    assert torch.equal(want["dq"], TWO_HOT_SCALE * dsa[..., None] * (k - k[:, :, b]))
    # premises: every expected value is bf16-exact (dbias: f32-exact with room for any order of partial sums: quarter-integers below 2^20)
    assert all(B.is_bf16(want[n]) for n in ("dq", "dk", "dv")) and B.is_bf16(out) and B.is_bf16(q)
    assert torch.equal(dbias * 4, (dbias * 4).round()) and float(ds.abs().sum(0).sum(-1).sum(-1).max()) * 4 < 2 ** 20
    lse = _two_hot_lse(TWO_HOT_SCALE)
    assert abs(lse - (32.0 * TWO_HOT_SCALE + math.log(2.0))) < 1e-3 and 32.0 * TWO_HOT_SCALE * LOG2E > 150      # (every other key's P underflows to 0)
    return dict(q=q, k=k, v=v, dout_c=dout, scale=TWO_HOT_SCALE, dtype=BF16, N=N, ws=ws, m=m, windows=W, want=want, out=out, lse=lse,
                table=torch.zeros(heads, N, dtype=F32), bidx=bidx)
