"""Cases of the long-sequence 16-bit-MFMA attention backward (include/gg_attn16b.h) shared by tests/test_attention16_bwd_cpu.py and
tests/test_gpu_attention16_bwd.py, and a torch restatement of the kernel's arithmetic contract.  Plain torch on the CPU: no GPU, no libgg.

Sizes: a single key (1); a full and a ragged 16-strip (16, 17); the 64-tile edge from both sides (63, 64, 65); a second 128-row block with one live row (129);
one live row in the last 64-row tile (257 and 577, the production length of CLIP ViT-L/14-336); whole tiles (320).  Classes: every class of
``attention_cases.classes_for(False, False)``; a single key has no other key to be peaked against, so N = 1 runs ``plain`` only.  Storage is bf16.

Two exact families (every expected value is bf16-representable, so the comparison is bit for bit):

* one-hot rows (``attention16_cases.one_hot_case`` with an integer ``dout``): P is exactly 1 on key sel(i) and 0 elsewhere, so dv[sel(i)] = dout[i] and, because
  delta_i = dout[i] . v[sel(i)] = dP[i][sel(i)], dS = 0: dq = dk = 0;
* two-hot rows (``two_hot_case``): P is exactly 1/2 on two keys; the closed form is in its docstring."""
import math

import torch

from tests import attention16_cases as A
from tests import attention_cases as AC

SIZES = (1, 16, 17, 63, 64, 65, 129, 257, 320, 577)
ONE_HOT_SIZES = (17, 65, 577)
TWO_HOT_SIZES = (17, 64, 80, 128)
TILE = 64
LOG2E = 1.4426950408889634
BF16 = torch.bfloat16


def params():
    """[(N, class)] of the conditioning cases."""
    return [(N, c) for N in SIZES for c in AC.classes_for(False, False) if N > 1 or c == "plain"]


def get_case(N, cls):
    return A.get_case("bf16", N, cls)          # (the forward's cases where the sizes coincide: computed once for both files)


def kw_of(c):
    return {k: v for k, v in c["kw"].items() if k not in ("map_h", "map_w", "head_dim", "window_size")}


def tiled_contract_bwd(c, out, lse, tile=TILE):
    """The contract of include/gg_attn16b.h in f32 arithmetic on canonical bf16-representable q, k, v, dout (``c``: a case of ``attention_cases.case`` or a dict
    with q, k, v, dout_c, scale), the forward's canonical ``out`` (bf16 values) and ``lse``: per ``tile``-key tile S with f32 accumulation,
    P = exp2(fma(S, scale log2 e, -lse log2 e)) (one rounding: no maximum is subtracted again), dP = dO V^T, delta = sum_d dO O in f32, dS = P (dP - delta), P and dS
    rounded to bf16 as the operands of dV = P^T dO, dK = dS^T Q, dQ = dS K, f32 accumulators, dq and dk times ``scale`` in f32, one rounding to bf16.  Returns
    canonical dq, dk, dv (fp64 holding bf16 values)."""
    f32 = torch.float32
    q, k, v, do = (c[n].to(f32) for n in ("q", "k", "v", "dout_c"))
    o = out.to(f32)
    sc2 = float(torch.tensor(c["scale"] * LOG2E, dtype=f32))
    scale = float(torch.tensor(c["scale"], dtype=f32))
    nl = (lse.to(f32) * torch.tensor(-LOG2E, dtype=f32))[..., None]                 # -lse log2 e, one f32 rounding
    delta = (do * o).sum(-1, keepdim=True)
    N = q.shape[-2]
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for t in range(0, N, tile):
        kt, vt = k[..., t:t + tile, :], v[..., t:t + tile, :]
        s = q @ kt.transpose(-1, -2)
        p = torch.exp2((s.double() * sc2 + nl.double()).to(f32))                    # one rounding: an FMA
        ds = p * (do @ vt.transpose(-1, -2) - delta)
        pb, dsb = p.to(BF16).to(f32), ds.to(BF16).to(f32)
        dv[..., t:t + tile, :] = pb.transpose(-1, -2) @ do
        dk[..., t:t + tile, :] = dsb.transpose(-1, -2) @ q
        dq += dsb @ kt
    r = lambda x: x.to(BF16).double()
    return {"dq": r(dq * scale), "dk": r(dk * scale), "dv": r(dv)}


def check(c, got, label):
    """``attention_cases.check`` on dq, dk, dv: e <= 4 max(yardstick, floor).  A single key (N = 1) has P = 1 and dS = P (dP - delta) = 0 in exact arithmetic, so the
    fp64 dq and dk are exactly zero and their relative figure is 0 / 0 for any kernel: there dv goes through the gate and dq, dk are held to an absolute bound,
    half a bf16 unit in the last place (2^-9) of the products whose difference they are -- scale * max |dP| * max |k| for dq, * max |q| for dk.  (f32 arithmetic leaves
    2^-24-sized residues of dP - delta, not zeros: the two sums run in different orders.)"""
    if c["N"] > 1:
        return AC.check(c, got, label, tensors=("dq", "dk", "dv"))
    bad = AC.check(c, got, label, tensors=("dv",))
    dp = float((c["dout_c"] @ c["v"].transpose(-1, -2)).abs().max())
    for name, other in (("dq", "k"), ("dk", "q")):
        assert float(c["ref"][name].abs().max()) == 0.0
        e, bound = float(got[name].abs().max()), AC.FLOOR[BF16] * c["scale"] * dp * float(c[other].abs().max())
        print(f"[{label}] max |{name}| {e:.1e} (reference 0; bound {bound:.1e})")
        if not e <= bound:
            bad.append((name, "abs", e, bound))
    return bad


def is_bf16(x):
    """Every value of ``x`` is bf16-representable."""
    return torch.equal(x.double(), x.to(BF16).double())


def one_hot_bwd_case(N):
    """``attention16_cases.one_hot_case(N)`` with an integer ``dout`` in -8 .. 8 and the expected gradients: dv[sel(i)] = dout[i] (sel is a bijection for the
    sizes used: gcd(7, N) = 1), dq = dk = 0.  Returns a dict with q, k, v, dout_c, scale (8), dtype, sel, margin, want."""
    q, k, v, sel, margin = A.one_hot_case(N)
    assert math.gcd(7, N) == 1
    g = torch.Generator().manual_seed(3000 + N)
    dout = torch.randint(-8, 9, q.shape, generator=g).double()
    dv = torch.zeros_like(v)
    dv[:, :, sel] = dout
    return dict(q=q, k=k, v=v, dout_c=dout, scale=8.0, dtype=BF16, sel=sel, margin=margin, N=N,
                want={"dq": torch.zeros_like(q), "dk": torch.zeros_like(k), "dv": dv}, out=v[:, :, sel])


def hadamard64():
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < 64:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def two_hot_case(N, heads=2, windows=2):
    """Keys: the first N of the 128 vectors {rows of the Sylvester Hadamard matrix H64, their negatives} (pairwise scores 64, 0 or -64); query i = k[i] + k[b(i)],
    b(i) = (i + 5) mod N: its score is 64 on keys i and b(i) and at most 0 elsewhere, so with ``scale`` = 8 (margin 512) P is exactly 1/2 on the two and 0 on the
    rest.  v integer in -8 .. 8, dout one +-1 per row (column c_i, sign s_i).  The closed form, all bf16-exact:
      out[i] = (v[i] + v[b]) / 2;  dP[i][j] = s_i v[j][c_i];  delta_i = s_i (v[i][c_i] + v[b][c_i]) / 2;
      dS[i][i] = s_i (v[i][c_i] - v[b][c_i]) / 4 = -dS[i][b]   (a quarter-integer of magnitude <= 4);
      dq[i] = 8 dS[i][i] (k[i] - k[b]);  dk[j] = 8 (dS[j][j] q[j] + dS[a][j] q[a]) with b(a) = j;  dv[j] = (dout[j] + dout[a]) / 2."""
    assert 6 <= N <= 128
    g = torch.Generator().manual_seed(4000 + N)
    h = hadamard64()
    keys = torch.cat([h, -h])[:N]
    k = keys.expand(windows, heads, N, 64).clone()
    b = (torch.arange(N) + 5) % N
    q = k + k[:, :, b]
    v = torch.randint(-8, 9, (windows, heads, N, 64), generator=g).double()
    col = torch.randint(0, 64, (windows, heads, N), generator=g)
    sign = (torch.randint(0, 2, (windows, heads, N), generator=g) * 2 - 1).double()
    dout = torch.zeros_like(v).scatter_(-1, col[..., None], sign[..., None])
    s = q @ k.transpose(-1, -2)
    two = torch.zeros(N, N, dtype=torch.bool)
    two[torch.arange(N), torch.arange(N)] = True
    two[torch.arange(N), b] = True
    assert bool((s[..., two] == 64).all()) and float(s.masked_fill(two, -math.inf).max()) <= 0
    out = (v + v[:, :, b]) / 2
    vc = torch.gather(v, -1, col[..., None]).squeeze(-1)                            # v[i][c_i]
    vbc = torch.gather(v[:, :, b], -1, col[..., None]).squeeze(-1)                  # v[b(i)][c_i]
    dsa = sign * (vc - vbc) / 4                                                     # dS[i][i]; dS[i][b(i)] = -dsa
    ds = torch.zeros(windows, heads, N, N, dtype=torch.float64)
    ds[..., torch.arange(N), torch.arange(N)] = dsa
    ds[..., torch.arange(N), b] = -dsa
    p = two.double() / 2
    want = {"dq": 8 * ds @ k, "dk": 8 * ds.transpose(-1, -2) @ q, "dv": p.t() @ dout}
    assert torch.equal(want["dq"], 8 * dsa[..., None] * (k - k[:, :, b]))
    return dict(q=q, k=k, v=v, dout_c=dout, scale=8.0, dtype=BF16, N=N, want=want, out=out, lse=512.0 + math.log(2.0))


def flat_inputs(c, layout="clip", pad=0):
    """qkv (tokens, 384 + pad), dout (tokens, 128) in bf16 and the column keywords for a dict of canonical q, k, v, dout_c (2 heads)."""
    qkv, kw = A.flat_qkv(c["q"], c["k"], c["v"], layout, BF16, pad=pad)
    W, H, N, D = c["q"].shape
    cc = dict(idx=AC.token_index("clip", N, W, 0, 0))
    return qkv, AC._flat(cc, c["dout_c"]).to(BF16), kw


def canon(c_or_shape, layout, dqkv):
    """dq, dk, dv in canonical form from a flat (tokens, >= 384) result in ``layout``."""
    W, H, N, D = c_or_shape
    q_off, k_off, v_off, hs = AC.columns(layout, H, D)
    cc = dict(idx=AC.token_index("clip", N, W, 0, 0), heads=H, hd=D, head_stride=hs, q_off=q_off, k_off=k_off, v_off=v_off)
    return dict(zip(("dq", "dk", "dv"), AC.canon_dqkv(cc, dqkv)))
