"""Ill-conditioned attention inputs, their fp64 references and the yardsticks the attention tests gate against.  Plain torch on the CPU: no GPU, no libgg.

A case is made by ``case(...)`` for one ``(layout, N, head_dim, heads, windows, window_size, causal, storage, cls)`` and is computed once (lru_cache; never
modify what it returns).  Layouts are the two the kernels take: ``tinyvit`` (per-head interleaved [q|k|v] columns, tokens of a map partitioned into windows, the
relative-position bias gathered through oracle.tinyvit_ref.attention_bias_idxs) and ``clip`` ([q|k|v] column blocks, tokens in order, no bias).  For bf16 / fp16
storage qkv and dout are rounded to the storage type first and every reference sees the rounded values.

Input classes (``CLASSES``; the score magnitude 32 is the one of the two older spike tests):

* ``plain``         q, k, v ~ N(0, 1), table ~ N(0, 0.5): the draw of the older tests, the control.
* ``late``          q, k scaled by 0.2; queries 5 and N-1 aligned with key N-1 (the last, ragged 16-key tile) at score 32 (``QK_SPLIT``: how the norm is shared
                    between the query and the key).  With more than one 64-key tile
                    it is a staircase as well: one key in each of the last four tiles (position 20 of the tile) is aligned with strength 0.25, 0.5, 0.75, 1
                    (key N-1 being the last step), so the running maximum of the spike rows grows tile after tile.  Every (window, head) has its own spike
                    direction: the same scores, other last bits.
* ``early``         the dominant key is key 2: every later tile underflows against it.
* ``shift+/-``      the component of every q and k along one unit vector is replaced by a common one: every score is +32 / -32 plus the plain spread.
                    Softmax does not see the shift; a kernel that subtracts at the wrong place or lets a padded / masked / out-of-window key (score 0) into
                    the sum does (``shift-``: such a key then outweighs the whole row).
* ``bias_spike``    (bias routes) q, k scaled by 0.2, table ~ N(0, 0.5) with one entry at +24 and one at -24 per head: even heads +24 at (|dy|, |dx|) =
                    (ws-1, ws-1) -- the four corner queries, each with ONE such key, the opposite corner -- and -24 at (ws-1, 0); odd heads +24 at (ws-1, 0)
                    -- the 2 ws queries of the top and bottom row, each with the key of the same column in the other row -- and -24 at (0, ws-1).  The
                    dominant key is chosen by the gather index alone.
* ``masked_spike``  (causal routes) q, k scaled by 0.2; for queries i = 3 and N-2, key i+1 is aligned at score 64 (masked: it must change nothing) and key i
                    at score 32 (the diagonal dominates).

Tensors are compared in one canonical form, (windows, heads, N, head_dim) for out / dq / dk / dv, (windows, heads, N) for lse, (heads, ws * ws) for dbias:
``canon_out`` / ``canon_lse`` / ``canon_dqkv`` bring a kernel's flat result there.

Error figure: ``e(T) = max |got - ref64| / max |ref64|`` over the whole tensor (``"all"``) and once more over the rows of interest only (``"rows"``: the spike
queries for out / lse / dq, the spike keys for dk / dv; dbias has no such axis), normalised by the largest reference magnitude of the same rows (at least
``ROWS_MIN`` of the tensor's: a saturated row has no gradient to be measured against).
Gate: ``e(T) <= 4 max(y(T), floor)`` with y(T) the yardstick's same figure and the floor half a unit in the last place of the compared type at max |ref|
(2^-24 f32, 2^-9 bf16, 2^-12 fp16; lse and dbias are f32 in every storage) -- the rule of tests/test_gpu_cls_head.py.  A yardstick is never the kernel:

* f32 storage (``F32_YARDSTICKS``; y(T) is the largest figure of them, each taken over ``ORDERS`` orders of the head-dim contraction and on one thread):
  ``f32``                 the same formula in torch f32 (softmax / logsumexp / autograd).  Held to y <= 1e-5 on every case of the GPU suite by the CPU test.
  ``f32_lse_domain``      the operation order the kernels document, where torch's order hides an error they have: scores in the exp2 domain (s * scale * log2 e:
                          an argument of magnitude up to 46, whose f32 rounding alone is 2.7e-6 of P), lse = m ln 2 + log l stored in f32, and a backward that
                          recomputes P = exp2(fma(q.k, scale log2 e, bias log2 e - lse log2 e)) from that lse instead of keeping the forward's P: no maximum is
                          subtracted again, and the FMA keeps the product unrounded where the forward's maximum was rounded.  On the peaked classes this is
                          what the kernels' dq / dk / dv errors are made of (measured on an MI355X: 2 .. 10 x torch's own f32 error, on every f32 route alike,
                          and at this yardstick's figure); ``plain`` and ``shift+/-`` do not need it.
  ``f32_split_products``  (routes whose products are split-bf16 MFMAs, ``split_products``) the same with every product formed from three bf16 planes per operand,
                          six plane products, small terms first (csrc/attention_split.h).
* bf16 / fp16 storage (``storage``): the fp64 formula with the roundings the project documents for that family: P rounded to the storage type before P.V with
  the row sum of the unrounded P and one rounding of the output (oracle/tinyvit_ref.py, _attention_core); for attention.hip's forward and the backward paired
  with it the bias as bf16(bias / scale) (``rounded_bias``; csrc/attention_flash.hip, gg_attention_flash_bwd_impl); in the backward P and dS rounded before the
  dV / dK / dQ products, delta from the rounded forward output, gradients rounded on store; lse from f32 arithmetic (it is an f32 result), dbias rounded to f32.

Defects (``DEFECTS``) are CPU restatements of kernel bugs applied to the fp64 formula; tests/test_attention_cases_cpu.py shows that each gate rejects them."""
import functools
import math

import torch

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
STORAGE = {"f32": F32, "bf16": BF16, "f16": F16}
FLOOR = {F32: 2.0 ** -24, BF16: 2.0 ** -9, F16: 2.0 ** -12}
CLASSES = ("plain", "late", "early", "shift+", "shift-", "bias_spike", "masked_spike")
DEFECTS = ("phantom_key", "mask_off_by_one", "tile_max", "bias_index", "neighbour_lse")
TENSORS = ("out", "lse", "dq", "dk", "dv", "dbias")
SPIKE = 32.0
# `late` / `early`: the aligned query has half the norm sqrt(32 sqrt(hd)) that would give the score with equal norms, the aligned key twice it.  With equal norms the
# spike query's weight in dk = dS^T q puts torch's own f32 dk error at 1.8e-5 of max |dk| on a 16 x 16 window (dS of the dominant key is a cancellation to 3e-4 of its
# terms), above the 1e-5 the f32 yardstick is held to (tests/test_attention_cases_cpu.py); with this split it is <= 3.1e-6 on every case of the GPU suite.
QK_SPLIT = 2.0
FACTOR = 4.0
# A saturated softmax row has no gradient: on the `late` / `early` / `masked_spike` queries the reference dq is 1e-12 of the tensor's largest value and the quotient
# "error / largest reference of the same rows" would compare rounding noise with nothing.  The rows' normaliser is therefore at least 2^-12 of the tensor's
# largest reference magnitude for an f32 tensor -- 4096 half-ulps of the compared type, so the whole tensor's magnitude for bf16 / fp16 results: rows above that
# level are measured against themselves, rows below it against that level.
ROWS_MIN = {F32: 2.0 ** -12, BF16: 1.0, F16: 1.0}
# the yardsticks whose larger figure is y(T) for f32 storage (see the module docstring)
F32_YARDSTICKS = ("f32", "f32_lse_domain")


def classes_for(bias, causal):
    """The classes that apply to a route: ``bias_spike`` needs a bias table, ``masked_spike`` a causal mask."""
    return tuple(c for c in CLASSES if (c != "bias_spike" or bias) and (c != "masked_spike" or causal))


def bias_idxs(ws):
    """(N, N) gather index of the relative-position table: |dy| * ws + |dx| (== oracle.tinyvit_ref.attention_bias_idxs, asserted in the CPU test)."""
    t = torch.arange(ws * ws)
    y, x = t // ws, t % ws
    return (y[:, None] - y[None, :]).abs() * ws + (x[:, None] - x[None, :]).abs()


def _units(g, windows, heads, hd):
    """Two orthonormal directions per (window, head), (windows, heads, hd) each: every window and head has its own spike vectors, so the last bits of its scores
    (and with them the rounding of every exponent) are its own -- a yardstick then samples windows * heads roundings, not one."""
    u1 = torch.randn(windows, heads, hd, generator=g, dtype=F64)
    u1 = u1 / u1.norm(dim=-1, keepdim=True)
    u2 = torch.randn(windows, heads, hd, generator=g, dtype=F64)
    u2 = u2 - (u2 * u1).sum(-1, keepdim=True) * u1
    return u1, u2 / u2.norm(dim=-1, keepdim=True)


def _stairs(N):
    """[(key, strength)]: one key per 64-key tile among the last four tiles, strengths ... 0.5, 0.75, 1; the last step is key N-1."""
    T = (N + 63) // 64
    steps = []
    for t in range(max(0, T - 4), T - 1):
        key = 64 * t + 20
        if key < N - 1:
            steps.append((key, 1.0 - 0.25 * (T - 1 - t)))
    return steps + [(N - 1, 1.0)]


def _draw(cls, N, hd, heads, windows, ws, causal, seed):
    """canonical q, k, v, dout (windows, heads, N, hd) in fp64, table (heads, ws * ws) or None, and the rows of interest."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, dout = (torch.randn(windows, heads, N, hd, generator=g, dtype=F64) for _ in range(4))
    table = torch.randn(heads, ws * ws, generator=g, dtype=F64) * 0.5 if ws else None
    a = math.sqrt(SPIKE * math.sqrt(hd))                      # |q| = |k| = a along one direction: score a^2 / sqrt(hd) = 32
    u1, u2 = _units(g, windows, heads, hd)
    info = dict(spike_q=[], spike_k=[], dominant={}, spike_bias=None)
    if cls == "plain":
        pass
    elif cls in ("late", "early"):
        q *= 0.2; k *= 0.2
        keys = _stairs(N) if cls == "late" else [(2, 1.0)]
        dom = keys[-1][0]
        for key, s in keys:
            k[:, :, key] = s * a * QK_SPLIT * u1
        qs = sorted({min(5, N - 1), N - 1})
        for i in qs:
            q[:, :, i] = a / QK_SPLIT * u1
        seen = [i for i in qs if not causal or dom <= i]
        info.update(spike_q=seen, spike_k=[key for key, _ in keys], dominant={i: dom for i in seen}, stairs=keys)
    elif cls in ("shift+", "shift-"):
        sign = 1.0 if cls == "shift+" else -1.0
        un = u1[:, :, None, :]
        q += (a - (q * un).sum(-1, keepdim=True)) * un
        k += (sign * a - (k * un).sum(-1, keepdim=True)) * un
    elif cls == "bias_spike":
        q *= 0.2; k *= 0.2
        hi = [(ws - 1) * ws + (ws - 1) if h % 2 == 0 else (ws - 1) * ws for h in range(heads)]
        lo = [(ws - 1) * ws if h % 2 == 0 else ws - 1 for h in range(heads)]
        for h in range(heads):
            table[h, hi[h]], table[h, lo[h]] = 24.0, -24.0
        info["spike_bias"] = (hi, lo)
    elif cls == "masked_spike":
        q *= 0.2; k *= 0.2
        rows = sorted({3, N - 2})
        for i, u in zip(rows, (u1, u2)):
            q[:, :, i] = a * u
            k[:, :, i] = a * u
            k[:, :, i + 1] = 2.0 * a * u                      # score 64, masked
        info.update(spike_q=rows, spike_k=rows + [i + 1 for i in rows], dominant={i: i for i in rows}, masked={i: i + 1 for i in rows})
    else:
        raise ValueError(cls)
    return q, k, v, dout, table, info


def token_index(layout, N, windows, ws, map_hw):
    """(windows, N) row of the flat qkv buffer for every (window, token)."""
    if layout == "tinyvit":
        per = (map_hw // ws) ** 2
        assert windows % per == 0
        return torch.arange(windows * N).view(windows // per, map_hw // ws, ws, map_hw // ws, ws).permute(0, 1, 3, 2, 4).reshape(windows, N)
    return torch.arange(windows * N).view(windows, N)


def columns(layout, heads, hd):
    """q_off, k_off, v_off, head_stride of the flat buffer."""
    return (0, hd, 2 * hd, 3 * hd) if layout == "tinyvit" else (0, heads * hd, 2 * heads * hd, hd)


def _flat(c, x, off=0, into=None):
    """canonical (windows, heads, N, hd) -> a flat buffer: columns [off + h * head_stride, + hd) of ``into`` (the qkv buffer), or a new (tokens, heads * hd) one."""
    W, H, N, D = x.shape
    stride = c["head_stride"] if into is not None else D
    if into is None:
        into = torch.zeros(W * N, H * D, dtype=x.dtype)
    rows = c["idx"].reshape(-1)
    for h in range(H):
        into[rows, off + h * stride:off + h * stride + D] = x[:, h].reshape(W * N, D)
    return into


def canon_out(c, flat):
    """(tokens, heads * hd) -> (windows, heads, N, hd), fp64 on the CPU."""
    f = flat.detach().double().cpu()[c["idx"]]                                 # (W, N, H * D)
    return f.view(c["windows"], c["N"], c["heads"], c["hd"]).permute(0, 2, 1, 3).contiguous()


def canon_lse(c, flat):
    """(tokens, heads) -> (windows, heads, N)."""
    return flat.detach().double().cpu()[c["idx"]].permute(0, 2, 1).contiguous()


def canon_dqkv(c, flat):
    """(tokens, 3 * heads * hd) -> dq, dk, dv in canonical form."""
    f = flat.detach().double().cpu()[c["idx"]]
    H, D, hs = c["heads"], c["hd"], c["head_stride"]
    res = []
    for off in (c["q_off"], c["k_off"], c["v_off"]):
        res.append(torch.stack([f[:, :, off + h * hs:off + h * hs + D] for h in range(H)], 1).contiguous())
    return res


# ------------------------------------------------------------------------------------------- the formula
def _scores(q, k, bias, scale, causal, mask_shift=0):
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias
    if causal:
        N = s.shape[-1]
        s = s.masked_fill(torch.triu(torch.ones(N, N, dtype=torch.bool), 1 + mask_shift), float("-inf"))
    return s


def attention_math(q, k, v, dout, table, bidx, scale, causal, *, dtype=F64, rnd=None, rounded_bias=False, defect=None, out_fwd=None, lse_fwd=None):
    """Forward and the recompute-from-lse backward (the form every backward kernel here has) written out, in ``dtype`` arithmetic.

    rnd: storage type whose roundings the kernels document (P before P.V, output once; P and dS before the backward products, delta from the rounded output,
    gradients on store); rounded_bias: the bias enters as bf16(bias / scale) * scale.  defect: one of DEFECTS.  Returns a dict of TENSORS (dbias None without
    a table)."""
    q, k, v, dout = (t.to(dtype) for t in (q, k, v, dout))
    r = (lambda t: t) if rnd is None else (lambda t: t.to(rnd).to(dtype))
    bias = None
    if table is not None:
        tab = table.to(dtype)
        if rounded_bias:
            tab = (tab / scale).to(BF16).to(dtype) * scale
        gi = bidx if defect != "bias_index" else (bidx + 1) % tab.shape[1]
        bias = tab[:, gi]                                                       # (H, N, N)
    s = _scores(q, k, bias, scale, causal, 1 if defect == "mask_off_by_one" else 0)
    N = s.shape[-1]
    if defect == "tile_max":                                                    # every 64-key tile against its own maximum, no rescale when it moves
        m = torch.cat([s[..., t:t + 64].amax(-1, keepdim=True).expand(*s.shape[:-1], min(64, N - t)) for t in range(0, N, 64)], -1)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    else:
        m = s.amax(-1, keepdim=True)
    pe = torch.exp(s - m)
    l = pe.sum(-1, keepdim=True)
    if defect == "phantom_key":                                                 # one more key of score 0 and v = 0 in the sum
        l = l + torch.exp(-m)
    out = r((r(pe) @ v) / l)
    lse = (m[..., -1:] + torch.log(l)).squeeze(-1)                              # (tile_max: against the last tile's maximum)
    # backward: P again from lse
    lse_b = lse if lse_fwd is None else lse_fwd.to(dtype)
    out_b = out if out_fwd is None else out_fwd.to(dtype)
    if defect == "neighbour_lse":
        lse_b = torch.roll(lse_b, -1, -1)
    p = pe / l if defect == "tile_max" else torch.exp(s - lse_b[..., None])
    dv = r(r(p).transpose(-1, -2) @ dout)
    dp = dout @ v.transpose(-1, -2)
    delta = (dout * out_b).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq = r(r(ds) @ k * scale)
    dk = r(r(ds).transpose(-1, -2) @ q * scale)
    dbias = None
    if table is not None:
        H, T = table.shape
        gi = bidx if defect != "bias_index" else (bidx + 1) % T
        dbias = torch.zeros(H, T, dtype=dtype).index_add_(1, gi.reshape(-1), ds.sum(0).reshape(H, -1))
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dbias=dbias)


def attention_autograd(q, k, v, dout, table, bidx, scale, causal, dtype):
    """torch's own softmax / logsumexp / autograd in ``dtype``."""
    q, k, v = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    tab = None if table is None else table.to(dtype).clone().requires_grad_(True)
    s = _scores(q, k, None if tab is None else tab[:, bidx], scale, causal)
    out = torch.softmax(s, -1) @ v
    lse = torch.logsumexp(s, -1)
    out.backward(dout.to(dtype))
    return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dbias=None if tab is None else tab.grad)


# ------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def case(layout, N, hd, heads=2, windows=2, ws=0, causal=False, storage="f32", cls="plain", map_hw=0):
    """Inputs in the kernels' flat layout, the fp64 reference and the yardsticks' tensors, all canonical.  Computed once; do not modify."""
    assert layout in ("tinyvit", "clip") and cls in CLASSES and storage in STORAGE
    if layout == "tinyvit":
        assert ws * ws == N
        map_hw = map_hw or ws
    else:
        assert ws == 0
    st = STORAGE[storage]
    seed = 7919 * N + 131 * hd + 17 * heads + 5 * windows + CLASSES.index(cls) + (1000003 if causal else 0)
    q, k, v, dout, table, info = _draw(cls, N, hd, heads, windows, ws, causal, seed)
    q, k, v, dout = (t.to(st).double() for t in (q, k, v, dout))                 # the storage type's values; every reference sees these
    table = None if table is None else table.float().double()                   # the table is f32 in every mode
    q_off, k_off, v_off, hs = columns(layout, heads, hd)
    c = dict(layout=layout, N=N, hd=hd, heads=heads, windows=windows, ws=ws, map_hw=map_hw, causal=causal, storage=storage, dtype=st, cls=cls,
             q_off=q_off, k_off=k_off, v_off=v_off, head_stride=hs, idx=token_index(layout, N, windows, ws, map_hw), scale=hd ** -0.5, info=info,
             q=q, k=k, v=v, dout_c=dout, table=None if table is None else table.float())
    qkv = torch.zeros(windows * N, 3 * heads * hd, dtype=F64)
    for x, off in ((q, q_off), (k, k_off), (v, v_off)):
        _flat(c, x, off, into=qkv)
    c["qkv"] = qkv.to(st)
    c["dout"] = _flat(c, dout).to(st)
    bidx = bias_idxs(ws) if ws else None
    c["bidx"] = bidx
    c["ref"] = attention_math(q, k, v, dout, table, bidx, c["scale"], causal)
    c["kw"] = dict(num_windows=windows, tokens_per_window=N, num_heads=heads, head_dim=hd, q_off=q_off, k_off=k_off, v_off=v_off, head_stride=hs,
                   window_size=ws, map_h=map_hw if ws else 0, map_w=map_hw if ws else 0)
    return c


def _math(c, **kw):
    return attention_math(c["q"], c["k"], c["v"], c["dout_c"], None if c["table"] is None else c["table"].double(), c["bidx"], c["scale"], c["causal"], **kw)


def _yard_tensors(c, name, rounded_bias):
    tab = None if c["table"] is None else c["table"].double()
    if name == "f32":
        return attention_autograd(c["q"], c["k"], c["v"], c["dout_c"], tab, c["bidx"], c["scale"], c["causal"], F32)
    if name == "f32_lse_domain":
        return _lse_domain_f32(c)
    if name == "f32_split_products":
        return _lse_domain_f32(c, split=True)
    if name == "storage":
        y = _math(c, rnd=c["dtype"], rounded_bias=rounded_bias)
        y["lse"] = _math(c, rounded_bias=True, dtype=F32)["lse"] if rounded_bias else _yard_tensors(c, "f32", False)["lse"]
        if y["dbias"] is not None:
            y["dbias"] = y["dbias"].float().double()
        return y
    raise ValueError(name)


def _split3(x):
    """x = x1 + x2 + x3 in bf16 planes (24 significand bits: csrc/attention_split.h, gg_split3_bf16)."""
    x1 = x.to(BF16).float()
    x2 = (x - x1).to(BF16).float()
    return x1, x2, (x - x1 - x2).to(BF16).float()


def _mm_split(a, b):
    """a @ b as the six plane products the split kernels form (x3 y2, x2 y3 and x3 y3 are dropped), small terms first, f32 accumulation."""
    a1, a2, a3 = _split3(a)
    b1, b2, b3 = _split3(b)
    return ((a1 @ b3 + a3 @ b1) + a2 @ b2) + (a1 @ b2 + a2 @ b1) + a1 @ b1


def _lse_domain_f32(c, split=False):
    """The f32 formula in the kernels' documented order: scores scaled into the exp2 domain (s * log2 e: one f32 rounding of an argument of magnitude up to 46),
    the forward's maximum subtracted there, lse = m ln 2 + log(l) stored in f32 in the natural domain; the backward's P = exp2(fma(q.k, scale log2 e, bias log2 e -
    lse log2 e)) from that stored lse (csrc/attention_split.h: "-lse in the exp2 domain: joins the bias AFTER the product") -- no maximum is subtracted again, the
    FMA keeps the product unrounded where the forward's maximum was rounded -- and delta from the stored f32 output.  ``split``: every product from three bf16 planes per operand (P and dS too)."""
    LOG2E = 1.4426950408889634
    mm = _mm_split if split else torch.matmul
    q, k, v, dout = (c[n].float() for n in ("q", "k", "v", "dout_c"))
    sc2 = float(torch.tensor(c["scale"] * LOG2E, dtype=F32))
    fma = lambda prod, add: (prod.double() * sc2 + add.double()).float()        # one rounding: the fp64 sum of an f32 product and an f32 addend is exact enough
    qk = mm(q, k.transpose(-1, -2))
    bias2 = torch.zeros(()) if c["table"] is None else (c["table"] * LOG2E)[:, c["bidx"]]
    mask = None
    if c["causal"]:
        mask = torch.triu(torch.ones(qk.shape[-1], qk.shape[-1], dtype=torch.bool), 1)
    s2 = fma(qk, bias2)
    if mask is not None:
        s2 = s2.masked_fill(mask, float("-inf"))
    m2 = s2.amax(-1, keepdim=True)
    pe = torch.exp2(s2 - m2)
    l = pe.sum(-1, keepdim=True)
    out = mm(pe, v) / l
    lse = m2 * 0.6931471805599453 + torch.log(l)                                # natural-log lse, as the forward kernels store it
    arg = fma(qk, bias2 + lse * -LOG2E)                                         # -lse joins the bias, the product joins both in one FMA
    if mask is not None:
        arg = arg.masked_fill(mask, float("-inf"))
    p = torch.exp2(arg)
    dv = mm(p.transpose(-1, -2), dout)
    ds = p * (mm(dout, v.transpose(-1, -2)) - (dout * out).sum(-1, keepdim=True))
    dq, dk = mm(ds, k) * c["scale"], mm(ds.transpose(-1, -2), q) * c["scale"]
    dbias = None
    if c["table"] is not None:
        H, T = c["table"].shape
        dbias = torch.zeros(H, T).index_add_(1, c["bidx"].reshape(-1), ds.sum(0).reshape(H, -1))
    return dict(out=out, lse=lse.squeeze(-1), dq=dq, dk=dk, dv=dv, dbias=dbias)


def case_key(c):
    return (c["layout"], c["N"], c["hd"], c["heads"], c["windows"], c["ws"], c["causal"], c["storage"], c["cls"], c["map_hw"] if c["layout"] == "tinyvit" else 0)


# ------------------------------------------------------------------------------------------- figures and gates
def rows_of_interest(c, name):
    """Index (into the token axis, or into the table for dbias) of the rows the class is about; None when the class has none."""
    info = c["info"]
    if name == "dbias":                                          # no query / key axis
        return None
    if c["cls"] == "bias_spike":                                 # the queries that own a +24 key (and, for dk / dv, those keys: the same set by symmetry)
        ws, N = c["ws"], c["N"]
        return sorted({0, ws - 1, N - ws, N - 1} | set(range(ws)) | set(range(N - ws, N)))
    rows = info["spike_k"] if name in ("dk", "dv") else info["spike_q"]
    return sorted(set(rows)) if rows else None


def errors(c, got):
    """{tensor: {"all": e, "rows": e or None}} of ``got`` (canonical tensors; missing / None entries are left out) against the case's fp64 reference."""
    res = {}
    for name in TENSORS:
        g, ref = got.get(name), c["ref"].get(name)
        if g is None or ref is None:
            continue
        g = g.detach().double().cpu()
        assert g.shape == ref.shape, (name, g.shape, ref.shape)
        e = {"all": float((g - ref).abs().max() / ref.abs().max()), "rows": None}
        rows = rows_of_interest(c, name)
        if rows is not None:
            sel = (lambda t: t[..., rows]) if name in ("lse", "dbias") else (lambda t: t[..., rows, :])
            e["rows"] = float((sel(g) - sel(ref)).abs().max() / max(float(sel(ref).abs().max()), ROWS_MIN[compared_type(c, name)] * float(ref.abs().max())))
        res[name] = e
    return res


def compared_type(c, name):
    return F32 if name in ("lse", "dbias") else c["dtype"]


def floor_for(c, name):
    return FLOOR[compared_type(c, name)]


def _yardstick_of(c, rounded_bias, split_products=False):
    """(y, {yardstick name: its figures}).  Computed on one thread: the order of an f32 reduction, and with it a yardstick's rounding noise, must not depend on
    how many cores the machine has."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _yardstick_1(c, rounded_bias, split_products)
    finally:
        torch.set_num_threads(threads)


# f32 yardsticks are taken over several orders of the head-dim contraction (the components of q, k, v, dout permuted alike: the same numbers, another order of
# every f32 sum over d) and y(T) is the largest figure: "the reduction order differs, the arithmetic does not".  One order alone is one draw of the rounding noise,
# and where a single element carries the figure -- the +24 entry of dbias sums a few dozen cancelling dS terms -- one draw was 3.5e-7 where the next shape's was 3.9e-6.
ORDERS = 4


def _reordered(c, order):
    if order == 0:
        return c, None
    perm = torch.randperm(c["hd"], generator=torch.Generator().manual_seed(order)) if order > 1 else torch.arange(c["hd"] - 1, -1, -1)
    d = dict(c)
    for n in ("q", "k", "v", "dout_c"):
        d[n] = c[n][..., perm].contiguous()
    return d, torch.argsort(perm)


def _yardstick_1(c, rounded_bias, split_products):
    names = F32_YARDSTICKS + (("f32_split_products",) if split_products else ()) if c["storage"] == "f32" else ("storage",)
    per = {}
    for n in names:
        runs = []
        for order in range(ORDERS if c["storage"] == "f32" else 1):
            d, back = _reordered(c, order)
            t = _yard_tensors(d, n, rounded_bias)
            if back is not None:
                t = {k: (v[..., back] if k in ("out", "dq", "dk", "dv") else v) for k, v in t.items()}
            runs.append(errors(c, t))
        per[n] = {name: {w: (None if runs[0][name][w] is None else max(r[name][w] for r in runs)) for w in ("all", "rows")} for name in runs[0]}
    first = per[names[0]]
    y = {name: {w: (None if first[name][w] is None else max(per[n][name][w] for n in names)) for w in ("all", "rows")} for name in first}
    return y, per


@functools.lru_cache(maxsize=None)
def _yardstick(key, rounded_bias, split_products):
    return _yardstick_of(case(*key), rounded_bias, split_products)


def yardstick(c, rounded_bias=False, parts=False, split_products=False):
    """y(T) of the case: {tensor: {"all", "rows"}}; with ``parts`` also the figures of each yardstick by name.  ``rounded_bias`` (bf16 storage): the route adds the
    bias as bf16(bias / scale); ``split_products`` (f32 storage): the route forms its products from three bf16 planes."""
    if "adhoc" in c:
        if split_products not in c["adhoc"]:
            c["adhoc"][split_products] = _yardstick_of(c, False, split_products)
        y, per = c["adhoc"][split_products]
    else:
        y, per = _yardstick(case_key(c), bool(rounded_bias), bool(split_products))
    return (y, per) if parts else y


def adhoc_case(q, k, v, dout, *, causal=False, spike_q=(), spike_k=(), cls="late"):
    """A case around inputs made elsewhere (canonical f32-representable q, k, v, dout of f32 storage, no bias): the fp64 reference, the rows of interest and, on
    first use, the yardstick -- everything ``errors`` / ``gates`` / ``check`` need."""
    q, k, v, dout = (t.detach().double().cpu() for t in (q, k, v, dout))
    W, H, N, D = q.shape
    c = dict(layout="clip", N=N, hd=D, heads=H, windows=W, ws=0, map_hw=0, causal=causal, storage="f32", dtype=F32, cls=cls, scale=D ** -0.5, table=None, bidx=None,
             q=q, k=k, v=v, dout_c=dout, info=dict(spike_q=list(spike_q), spike_k=list(spike_k), spike_bias=None), adhoc={}, idx=token_index("clip", N, W, 0, 0))
    c["q_off"], c["k_off"], c["v_off"], c["head_stride"] = columns("clip", H, D)
    c["ref"] = attention_math(q, k, v, dout, None, None, c["scale"], causal)
    return c


def gates(c, rounded_bias=False, split_products=False):
    """{tensor: {"all": gate, "rows": gate or None}}: 4 max(y, floor)."""
    y = yardstick(c, rounded_bias, split_products=split_products)
    return {n: {w: (None if v is None else FACTOR * max(v, floor_for(c, n))) for w, v in yw.items()} for n, yw in y.items()}


def check(c, got, label, rounded_bias=False, tensors=None, split_products=False):
    """Print every figure next to its gate and return the list of (tensor, which, error, gate) that miss.  ``got``: canonical tensors by name."""
    e, g, y = errors(c, got), gates(c, rounded_bias, split_products), yardstick(c, rounded_bias, split_products=split_products)
    bad, cells = [], []
    for name in TENSORS:
        if name not in e or (tensors is not None and name not in tensors):
            continue
        for w in ("all", "rows"):
            if e[name][w] is None:
                continue
            ok = math.isfinite(e[name][w]) and e[name][w] <= g[name][w]
            cells.append(f"{name}{'' if w == 'all' else '@rows'} {e[name][w]:.1e}/{y[name][w]:.1e}{'' if ok else ' MISS(gate %.1e)' % g[name][w]}")
            if not ok:
                bad.append((name, w, e[name][w], g[name][w]))
    print(f"\n[{label} {c['cls']}] kernel/yardstick: " + "  ".join(cells))
    return bad


# ------------------------------------------------------------------------------------------- the routes of tests/test_gpu_attention_conditioning.py
def _route(name, api, layout, N, hd, *, ws=0, map_hw=0, windows=2, storage="f32", bias=False, causal=False, bwd=True, split=False, ds_handoff=False, dtype_code=None,
           kernels=()):
    split_products = storage == "f32" and (split or api == "causal" or (hd == 32 and (N + 15) // 16 in (4, 9, 13)))
    assert len(kernels) == (2 if bwd else 1)
    return dict(name=name, api=api, layout=layout, N=N, hd=hd, ws=ws, map_hw=map_hw or ws, windows=windows, heads=2, storage=storage, bias=bias, causal=causal, bwd=bwd,
                split=split, ds_handoff=ds_handoff, dtype_code=dtype_code, kernels=tuple(kernels), split_products=split_products)


# api: "flash" = ops.attention_flash (gg_attention_flash_fwd / _bwd), "attention" = ops.attention (gg_attention_fwd / _fwd_f16 / _bwd), "causal" = gg_attention_causal_fwd / _bwd.
# The table and the reading of the dispatch behind it are in the docstring of tests/test_gpu_attention_conditioning.py.
# kernels: ((GG_ATTN_KERNEL_* name, variant) of the forward, the same of the backward) that gg_attention_route (include/gg_attn_route.h) must report for the case --
# names as in geoguessr_ai_amd._lib.ATTN_KERNELS; tests/test_attention_route_cpu.py holds the report to them, the GPU digest test asserts them on the arguments it launches.
_SPLIT = lambda n: (("FLASH_FWD_SPLIT", n), ("FLASH_BWD_SPLIT", n))
_RES, _RES_TAIL, _FWD_STREAM = ("FLASH_FWD_RESIDENT", 0), ("FLASH_FWD_RESIDENT", 1), ("FLASH_FWD_STREAM", 0)
_FUSED = lambda n=0: ("FLASH_BWD_FUSED", n)
_STREAM, _STREAM_DS = (_FWD_STREAM, ("FLASH_BWD_STREAM", 0)), (_FWD_STREAM, ("FLASH_BWD_STREAM_DS", 0))
_SPLIT64 = (("FLASH64_FWD_SPLIT", 0), ("FLASH64_BWD_SPLIT", 0))
_CAUSAL_BF16 = (_FWD_STREAM, _FUSED())
_ATTN = lambda n: (("FWD", n), ("BWD", n))
ROUTES = [
    _route("split_f32_7x7", "flash", "tinyvit", 49, 32, ws=7, map_hw=14, windows=8, bias=True, kernels=_SPLIT(4)),
    _route("split_f32_12x12", "flash", "tinyvit", 144, 32, ws=12, bias=True, kernels=_SPLIT(9)),
    _route("split_f32_14x14", "flash", "tinyvit", 196, 32, ws=14, bias=True, kernels=_SPLIT(13)),
    _route("split_f32_linear200", "flash", "clip", 200, 32, kernels=_SPLIT(13)),      # the 13-strip split kernels without a window geometry or bias
    _route("resident_f32_hd32_17", "flash", "clip", 17, 32, kernels=(_RES, _FUSED())),      # 2 strips, no tail
    _route("resident_f32_hd32_80", "flash", "clip", 80, 32, kernels=(_RES_TAIL, _FUSED())),      # 5 strips: the cooperative tail; single pass with 4 owner waves
    _route("resident_f32_hd64_50", "flash", "clip", 50, 64, kernels=(_RES, _FUSED(4))),      # 4 strips, no tail
    _route("resident_f32_hd64_80", "flash", "clip", 80, 64, kernels=(_RES_TAIL, _FUSED())),      # head dim 64: 5 owner waves (4 < 2 * 64 / 16)
    _route("fused_f32_16x16", "flash", "tinyvit", 256, 32, ws=16, bias=True, kernels=(_FWD_STREAM, _FUSED())),      # forward streams: 77 KB > 64 KB
    _route("stream_f32_hd64_200", "flash", "clip", 200, 64, kernels=_STREAM),
    _route("stream_f32_hd64_257", "flash", "clip", 257, 64, kernels=_STREAM),      # 5 tiles with one live row in the last
    _route("stream_f32_24x24", "flash", "tinyvit", 576, 32, ws=24, bias=True, kernels=_STREAM),
    _route("handoff_f32_hd64_200", "flash", "clip", 200, 64, ds_handoff=True, kernels=_STREAM_DS),
    _route("handoff_f32_24x24", "flash", "tinyvit", 576, 32, ws=24, bias=True, ds_handoff=True, kernels=_STREAM_DS),
    _route("dtype3_65", "flash", "clip", 65, 64, split=True, kernels=_SPLIT64),
    _route("dtype3_200", "flash", "clip", 200, 64, split=True, kernels=_SPLIT64),      # 4 tiles
    _route("flash_bf16_hd64_80", "flash", "clip", 80, 64, storage="bf16", kernels=(_RES_TAIL, _FUSED())),
    _route("flash_bf16_hd64_257", "flash", "clip", 257, 64, storage="bf16", kernels=_STREAM),
    _route("flash_bf16_24x24", "flash", "tinyvit", 576, 32, ws=24, bias=True, storage="bf16", kernels=_STREAM),      # tiny_vit_21m_384 stage 2
    _route("causal_bf16_17", "causal", "clip", 17, 64, storage="bf16", causal=True, dtype_code=0, kernels=_CAUSAL_BF16),
    _route("causal_bf16_77", "causal", "clip", 77, 64, storage="bf16", causal=True, dtype_code=0, kernels=_CAUSAL_BF16),      # 2 tiles / 5 strips
    _route("causal_f32_17", "causal", "clip", 17, 64, causal=True, dtype_code=1, kernels=_SPLIT64),
    _route("causal_f32_77", "causal", "clip", 77, 64, causal=True, dtype_code=1, kernels=_SPLIT64),
    _route("causal_split_17", "causal", "clip", 17, 64, causal=True, dtype_code=3, kernels=_SPLIT64),      # dtype 3: the same kernels as dtype 1
    _route("causal_split_77", "causal", "clip", 77, 64, causal=True, dtype_code=3, kernels=_SPLIT64),
    _route("attn_bf16_7x7", "attention", "tinyvit", 49, 32, ws=7, map_hw=14, windows=8, storage="bf16", bias=True, kernels=_ATTN(4)),
    _route("attn_bf16_10x10", "attention", "tinyvit", 100, 32, ws=10, storage="bf16", bias=True, kernels=_ATTN(10)),
    _route("attn_bf16_13x13", "attention", "tinyvit", 169, 32, ws=13, storage="bf16", bias=True, kernels=_ATTN(14)),
    _route("attn_bf16_16x16", "attention", "tinyvit", 256, 32, ws=16, storage="bf16", bias=True, kernels=_ATTN(16)),
    _route("attn_bf16_12x12", "attention", "tinyvit", 144, 32, ws=12, storage="bf16", bias=True, kernels=(("FWD", 10), ("FLASH_BWD_SPLIT", 9))),      # rounded bias
    _route("attn_bf16_14x14", "attention", "tinyvit", 196, 32, ws=14, storage="bf16", bias=True, kernels=(("FWD", 14), ("FLASH_BWD_SPLIT", 13))),      # rounded bias
    _route("attn_bf16_grouped_7x7", "attention", "tinyvit", 49, 32, ws=7, map_hw=35, windows=75, storage="bf16", bias=True,
           kernels=(("FWD_GROUPED", 0), ("BWD_GROUPED", 0))),      # 75 windows: a ragged last group
    _route("attn_bf16_clip_50", "attention", "clip", 50, 64, storage="bf16", bwd=False, kernels=(("FWD", 4),)),      # (the backward of head dim 64 is the flash one above)
    _route("attn_f16_50", "attention", "clip", 50, 64, storage="f16", bwd=False, kernels=(("FWD", 4),)),
    _route("attn_f16_197", "attention", "clip", 197, 64, storage="f16", bwd=False, kernels=(("FWD", 14),)),
    _route("attn_f16_257", "attention", "clip", 257, 64, storage="f16", bwd=False, kernels=(_FWD_STREAM,)),      # beyond 256 tokens
]
ROUTE = {r["name"]: r for r in ROUTES}


def route_case(r, cls):
    return case(r["layout"], r["N"], r["hd"], r["heads"], r["windows"], r["ws"], r["causal"], r["storage"], cls, r["map_hw"] if r["layout"] == "tinyvit" else 0)


def route_params():
    """[(route name, class)] for every class that applies to every route."""
    return [(r["name"], c) for r in ROUTES for c in classes_for(r["bias"], r["causal"])]


# ------------------------------------------------------------------------------------------- the bits of the streaming backward before it lost its resident forms
# tests/golden/attention_bwd_parent.json (tools/make_attention_bwd_parent_golden.py) holds SHA-256 digests of dq, dk, dv of these calls from the build in which
# flash_bwd_dq_kernel, flash_bwd_dq_ds_kernel and flash_bwd_dkv_kernel still carried their resident (RES) template forms; the smallest shapes that reach each
# streaming kernel, 2 heads, 2 sequences / images, the `plain` class.  (name, layout, N, head dim, ws, map side, windows, storage, dS hand-off):
#   161 tokens at head dim 64: npad 176, the single-pass kernel would need 173,904 B of LDS against 163,840 -- the first length that streams at head dim 64;
#   257 tokens at head dim 32: the first length beyond 256, 5 tiles with one token in the last;
#   17 x 17 windows on a 34 x 34 map (4 windows an image), bias and dbias: the windowed streaming route.
PARENT_BWD = (
    ("lin161_hd64_f32", "clip", 161, 64, 0, 0, 2, "f32", False),
    ("lin161_hd64_bf16", "clip", 161, 64, 0, 0, 2, "bf16", False),
    ("lin161_hd64_f32_handoff", "clip", 161, 64, 0, 0, 2, "f32", True),
    ("lin257_hd32_f32", "clip", 257, 32, 0, 0, 2, "f32", False),
    ("lin257_hd32_bf16", "clip", 257, 32, 0, 0, 2, "bf16", False),
    ("win17_hd32_f32", "tinyvit", 289, 32, 17, 34, 8, "f32", False),
    ("win17_hd32_f32_handoff", "tinyvit", 289, 32, 17, 34, 8, "f32", True),
    ("win17_hd32_bf16", "tinyvit", 289, 32, 17, 34, 8, "bf16", False),
)


def _sha(t):
    """SHA-256 of a tensor's raw bytes (f32 or 16-bit storage, C order)."""
    import hashlib
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.int32 if t.dtype == F32 else torch.int16).numpy().tobytes()).hexdigest()


def parent_bwd_bits(ops):
    """{name: {"inputs": {tensor: digest}, "dq" / "dk" / "dv": digest}} of the PARENT_BWD calls, run on the GPU through ``ops`` (geoguessr_ai_amd.ops).  The
    inputs are the seeded qkv / dout / table and the forward's own out / lse (the backward recomputes P from them); dq, dk, dv are hashed in canonical form,
    in the storage type.  dbias is requested on the window cases and not hashed: its bins are filled by floating-point atomics in no fixed order."""
    store = {}
    for name, layout, N, hd, ws, map_hw, windows, storage, handoff in PARENT_BWD:
        c = case(layout, N, hd, 2, windows, ws, False, storage, "plain", map_hw)
        qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
        table = c["table"].cuda() if ws else None
        out, lse = ops.attention_flash(qkv, want_lse=True, bias_table=table, **c["kw"])
        dqkv, dbias = ops.attention_flash(qkv, dout=dout, out=out, lse=lse, bias_table=table, want_dbias=table is not None, ds_handoff=handoff, **c["kw"])
        assert (dbias is not None) == bool(ws) and dqkv.dtype == c["dtype"]
        inputs = dict(qkv=_sha(qkv), dout=_sha(dout), out=_sha(out), lse=_sha(lse))
        if table is not None:
            inputs["table"] = _sha(table)
        store[name] = dict(inputs=inputs, **{n: _sha(t.to(c["dtype"])) for n, t in zip(("dq", "dk", "dv"), canon_dqkv(c, dqkv))})
    return store
