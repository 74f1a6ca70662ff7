"""Every attention kernel the dispatch reaches without a GG_* switch, forward and backward (dbias included wherever the route has a bias), on the peaked,
shifted and masked score rows of tests/attention_cases.py -- against fp64, gated by 4 x max(yardstick, half an ulp) per tensor, over the whole tensor and once
more over the spike rows alone.  The classes, the yardsticks and the error figure are described there; tests/test_attention_cases_cpu.py shows on the CPU that
the gates reject a phantom (padded) key, an off-by-one causal mask, a per-tile maximum, a shifted bias gather and a neighbour's lse.  Every figure is printed
next to its yardstick (`pytest -s`); DESIGN.md 5 holds the measured table.

Routes (attention_cases.ROUTES), as read from the dispatch.  Heads = 2 and windows / images = 2 unless the route needs more.

gg_attention_flash_fwd (csrc/attention_flash.hip), in this order:
  dtype 3                                               -> flash64_split_q_kernel<3,false> at every length                      dtype3_65, dtype3_200
  dtype 1, head dim 32, 4 / 9 / 13 strips of 16 tokens  -> flash_fwd_split_kernel<float,3,NT> (no window geometry needed)       split_f32_7x7 (7 x 7 on a 14 x 14 map),
                                                                                                                                _12x12, _14x14, split_f32_linear200
  resident (both operand images within 64 KB of LDS:    -> flash_fwd_kernel<T,D,true>; 4 n + 1 strips (5 .. 17): cooperative    resident_f32_hd32_17 (no tail), _hd32_80
  <= 208 tokens at head dim 32, <= 112 at 64)              tail                                                                 (tail), _hd64_50 (no tail), _hd64_80 (tail),
                                                                                                                                flash_bf16_hd64_80
  else                                                  -> flash_fwd_kernel<T,D,false> (streaming, 64-query tiles)              fused_f32_16x16 (77 KB), stream_f32_hd64_200,
                                                                                                                                _hd64_257, stream_f32_24x24, flash_bf16_hd64_257,
                                                                                                                                flash_bf16_24x24, attn_f16_257 (dtype 2)
gg_attention_flash_bwd_impl, in this order:
  dtype 3                                               -> flash64_split_q_kernel<3,true> + flash64_split_dkv_kernel<3>         dtype3_65, dtype3_200
  dtype 0 / 1, head dim 32, 4 / 9 / 13 strips           -> flash_bwd_split_kernel<T,planes,dbias,NT> (single pass)              split_f32_* (three planes, with dbias and
                                                                                                                                without), attn_bf16_12x12 / _14x14 (one plane,
                                                                                                                                through gg_attention_bwd: rounded bias)
  <= 256 padded tokens and the three window images fit  -> flash_bwd_fused_kernel<T,D,dbias,NT> (single pass; 4 n + 1 strips    fused_f32_16x16 (with bias), resident_f32_*
  160 KB (head dim 32: always; head dim 64: <= 160)        and enough waves: one owner wave fewer, cooperative tail)            (hd32_80: 4 owner waves), flash_bf16_hd64_80
  else, ds_scratch given                                -> flash_bwd_dkv_kernel<T,D,dbias,true> + flash_bwd_dq_ds_kernel<T,D>   handoff_f32_hd64_200, handoff_f32_24x24
                                                           (streaming: a workgroup per 64-row tile; dS handed to the dQ pass)
  else                                                  -> flash_bwd_dq_kernel<T,D> + flash_bwd_dkv_kernel<T,D,dbias>,          stream_f32_hd64_200, _257, stream_f32_24x24,
                                                           streaming                                                            flash_bf16_hd64_257, flash_bf16_24x24
  The resident form of the two-pass kernels (whole-window images in LDS) was removed: a window small enough for it (<= 208 / 112 tokens) always passes the
  single-pass test before it (derivation in gg_attention_flash_bwd_impl), so GG_ATTN_NO_FUSED_BWD selects these same streaming kernels.
gg_attention_causal_fwd / _bwd (head dim 64 only, at most 77 tokens):
  dtype 0                                               -> flash_fwd_kernel<bf16,64,false,true> + flash_bwd_fused_kernel<bf16,64,false,0,true>   causal_bf16_17, _77
  dtype 1, 3 (the same kernels)                         -> flash64_split_q_kernel<3,*,true> + flash64_split_dkv_kernel<3,true>                   causal_f32_17, _77, causal_split_17, _77
gg_attention_fwd / _fwd_f16 / _bwd (csrc/attention.hip; bf16 / fp16 storage, at most 256 tokens and 16 x 16 windows, beyond: the flash entry points above):
  forward, 4 / 10 / 14 / 16 key tiles by token count    -> attn_fwd_kernel<D,KT[,f16]>                                          attn_bf16_7x7 (4), _10x10 (10), _12x12 (10),
                                                                                                                                _13x13 (14), _14x14 (14), _16x16 (16),
                                                                                                                                attn_bf16_clip_50 (head dim 64), attn_f16_50, _197
  head dim 32, 4 key tiles, >= 64 windows               -> attn_fwd_small_kernel / attn_bwd_small_kernel (8 windows a group)     attn_bf16_grouped_7x7 (75 windows: ragged group)
  backward, head dim 32 windows of 9 / 13 strips        -> flash_bwd_split_kernel<bf16,1,..> (above)
  backward, else (head dim 32 only)                     -> attn_bwd_kernel<32,KT,dbias>                                         attn_bf16_7x7, _10x10, _13x13, _16x16

The backward is given the kernel's own forward output and lse, as the models give it.  Every element of every output is compared."""
import pytest
import torch

from tests import attention_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from geoguessr_ai_amd import ops as o
    from geoguessr_ai_amd import _lib
    _lib.require_gpu()
    return o


def _run(ops, r, c, want_dbias=True):
    """One forward and (where the route has one) one backward through the route's entry points; canonical tensors by name."""
    from geoguessr_ai_amd import _lib as L
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    table = c["table"].cuda() if r["bias"] else None
    got = {}
    if r["api"] == "causal":
        from tests.clip_text_helpers import causal
        from tests.clip_text_train_helpers import attn_bwd
        B, T, H = c["windows"], c["N"], c["heads"]
        rc, out, lse = causal(L, qkv, B, T, H, r["dtype_code"], qkv.stride(0))
        assert rc == 0, L.lib().gg_last_error()
        rc, dqkv = attn_bwd(L, qkv, out, lse, dout, B, T, H, r["dtype_code"])
        assert rc == 0, L.lib().gg_last_error()
        dbias = None
    else:
        fn = ops.attention_flash if r["api"] == "flash" else ops.attention
        kw = dict(c["kw"])
        kw["bias_table" if r["api"] == "flash" else "bias"] = table
        bkw = dict(kw)
        if r["api"] == "flash":
            kw["split"] = bkw["split"] = r["split"]
            bkw["ds_handoff"] = r["ds_handoff"]
        out, lse = fn(qkv, want_lse=True, **kw)
        dqkv = dbias = None
        if r["bwd"]:
            dqkv, dbias = fn(qkv, dout=dout, out=out, lse=lse, want_dbias=want_dbias and table is not None, **bkw)
    torch.cuda.synchronize()
    assert out.dtype == c["dtype"] and lse.dtype == torch.float32
    got["out"], got["lse"] = A.canon_out(c, out), A.canon_lse(c, lse)
    if dqkv is not None:
        assert dqkv.dtype == c["dtype"]
        got["dq"], got["dk"], got["dv"] = A.canon_dqkv(c, dqkv)
        got["dbias"] = None if dbias is None else dbias.double().cpu()
    return got


@pytest.mark.parametrize("route,cls", A.route_params())
def test_attention_route_on_conditioned_inputs(ops, route, cls):
    r = A.ROUTE[route]
    c = A.route_case(r, cls)
    rounded_bias = r["api"] == "attention" and r["bias"]          # attention.hip adds the bias as bf16(bias / scale); its paired backward recomputes P with it
    got = _run(ops, r, c)
    expect = ("out", "lse") + (("dq", "dk", "dv") + (("dbias",) if r["bias"] else ()) if r["bwd"] else ())
    assert all(got.get(n) is not None for n in expect), [n for n in expect if got.get(n) is None]
    bad = A.check(c, got, route, rounded_bias, split_products=r["split_products"])
    if r["bias"] and r["bwd"]:          # the frozen-bias instantiation of the backward (no dbias bins)
        frozen = _run(ops, r, c, want_dbias=False)
        assert frozen["dbias"] is None
        bad += A.check(c, frozen, route + " (no dbias)", rounded_bias, tensors=("dq", "dk", "dv"), split_products=r["split_products"])
    assert not bad, bad


def test_split_attention_backward_on_the_rescale_spike_input(ops):
    """The input of tests/test_gpu_clip_split.py::test_split_attention_online_softmax_rescale_branch (head dim 64, 200 tokens, query 5 of image 0 / head 0 against
    keys 20 / 70 / 140 / 195 of four tiles, ever more strongly), whose backward that test prints and does not gate: here out, lse, dq, dk, dv of the split kernels
    (dtype 3) and of the f32 kernels (dtype 1) are held to 4 x max(yardstick, 2^-24), whole tensor and spike rows.  Measured on an MI355X (kernel / yardstick):
    dtype 3 dq 4.8e-06 / 1.0e-05, dk 1.1e-05 / 1.4e-05, dv 5.6e-07 / 4.3e-07; dtype 1 dq 1.3e-05 / 1.0e-05, dk 2.2e-05 / 1.4e-05, dv 4.4e-07 / 4.3e-07."""
    from tests.test_gpu_clip_split import NH, HD, NIMG, _attn_case, _attn_run
    N = 200
    s = _attn_case(N, spike=True)
    x = s["qkv"].reshape(NIMG, N, 3, NH, HD)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    dout = s["dout"].reshape(NIMG, N, NH, HD).transpose(1, 2)
    c = A.adhoc_case(q, k, v, dout, spike_q=(5,), spike_k=(20, 70, 140, 195))
    assert float((A.canon_out(c, s["out"]) - c["ref"]["out"]).abs().max()) < 1e-12      # the same reference
    bad = []
    for split in (True, False):
        g, _, _ = _attn_run(ops, s, N, split)
        got = dict(out=A.canon_out(c, g["out"]), lse=A.canon_lse(c, g["lse"]))
        got["dq"], got["dk"], got["dv"] = (A.canon_out(c, g[n]) for n in ("dq", "dk", "dv"))
        bad += A.check(c, got, f"rescale spike hd64 N={N} {'dtype 3' if split else 'dtype 1'}", split_products=split)
    assert not bad, bad


def test_streaming_backward_bits_unchanged_from_the_parent_build(ops):
    """dq, dk, dv of the seeded streaming-route calls of tests/attention_cases.py::parent_bwd_bits (head dim 64 at 161 tokens, head dim 32 at 257 tokens and on
    17 x 17 windows with bias and dbias; f32 and bf16 storage; with and without the dS hand-off) equal, bit for bit, what the build gave in which the two-pass
    backward kernels still had their resident template forms (tests/golden/attention_bwd_parent.json, tools/make_attention_bwd_parent_golden.py).  The inputs'
    digests -- the forward's out and lse among them -- are compared first, so that a changed input is reported as such.  dbias is not compared here (atomics in
    no fixed order); the fp64 gates above hold it."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bwd_parent.json")) as f:
        gold = json.load(f)
    got = A.parent_bwd_bits(ops)
    assert sorted(got) == sorted(gold) == sorted(c[0] for c in A.PARENT_BWD)
    for name in sorted(got):
        assert got[name]["inputs"] == gold[name]["inputs"], f"{name}: the inputs differ from the golden file's (not a finding about the backward)"
    bad = [(name, t) for name in sorted(got) for t in ("dq", "dk", "dv") if got[name][t] != gold[name][t]]
    assert not bad, bad
