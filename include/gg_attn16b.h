/* libgg -- long-sequence attention backward on the 16-bit matrix pipe ("Attention backward beyond 256 tokens on the 16-bit MFMA"): the backward of
 * bf16 rows the single-pass kernel of csrc/attention_flash.hip cannot hold (CLIP ViT-L/14-336: 577 tokens), with all five products on v_mfma_f32_16x16x32_bf16
 * instead of the f32 MFMA of gg_attention_flash_bwd (dtype 0), and the opt-in switch that routes the bf16 CLIP vision tower's TRAINING step -- the forward, the
 * recompute replay and the attention backward -- to the 16-bit-MFMA pair.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Arithmetic contract (tests/attention_cases.py, attention_math(..., rnd = bf16); tests/attention16_bwd_cases.py restates the tiled form on the CPU):
 *   scores       S = Q K^T on the 16-bit MFMA with f32 accumulation;
 *   P            exp2(fma(acc, scale log2 e, -lse log2 e)) in f32, from the forward's lse: no maximum is subtracted again;
 *   dP           dO V^T on the same MFMA;
 *   delta        delta_i = sum_d dO_id O_id in f32, from the stored bf16 `out`;
 *   dS           P (dP - delta) in f32;
 *   dV           P rounded to bf16 once, as the operand of dV = P^T dO;
 *   dK, dQ       dS rounded to bf16 once, as the operand of dK = dS^T Q and dQ = dS K;
 *   store        the three accumulators are f32; dq and dk are multiplied by `scale` in f32; each gradient is rounded to bf16 once, on store;
 *   padding      keys and queries beyond tokens_per_window in a ragged tile contribute exactly zero and are never stored.
 * No atomics and a fixed summation order: two calls give the same bits, and a window's result does not depend on num_windows.  The forward's out / lse may come
 * from gg_attention_flash16_fwd or from gg_attention_flash_fwd (dtype 0): either pair is a valid input. */
#ifndef GG_ATTN16B_H
#define GG_ATTN16B_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* dqkv [tokens][ld] (the dq, dk and dv columns of every live token, at qkv's ld, column offsets and head_stride; nothing else is written) from qkv, the forward's
 * out [tokens][ldo] and lse f32 [tokens][num_heads], and dout [tokens][lddo] (head h at column h * 64 of out and dout).  `dtype` 0 = bf16 only: 2 is refused
 * ("fp16 storage is inference-only"), 1 and 3 are f32 storage.  Of GgAttnArgs it reads qkv, ld, q_off, k_off, v_off, head_stride (both qkv layouts of
 * gg_attention_flash_fwd), head_dim (64), num_heads, num_windows, tokens_per_window (>= 1, any), window_size (0: linear tokens), scale (any), out, ldo, lse, dout,
 * lddo, dqkv; ds_scratch is ignored.  Alignment as the forward's: qkv, out, dout and dqkv 16-byte aligned, ld, ldo, lddo, the offsets and head_stride multiples of
 * 4 elements.  head_dim != 64, window_size != 0, bias, bias_table, dbias, window_map, num_windows_dev and a missing lse, out, dout or dqkv are refused by name. */
int gg_attention_flash16_bwd(const GgAttnArgs* args, int dtype, void* stream);
/* calls of gg_attention_flash16_bwd enqueued by this process so far: one count per call, however many kernels it launches (tests count routes with it) */
int64_t gg_attention_flash16_bwd_calls(void);

/* on != 0: a TRAINING step of the bf16 CLIP vision tower (GgClipCfg.act_dtype 0, not causal) with more than 256 tokens sends every layer's attention forward
 * (gg_clip_forward with training != 0, lse where a layer is kept, and the recompute replay inside gg_clip_backward) to gg_attention_flash16_fwd and the attention
 * backward to gg_attention_flash16_bwd.  Every other route is as before whatever the switch says: inference forwards (gg_clip_set_attention16 is theirs), fp32,
 * fp32_split, fp16 and fp8, the text tower, towers of at most 256 tokens, TinyViT.  The workspace plan is unchanged (the dS region stays planned and is not read).
 * Process-wide, default 0; returns the previous value.  The switch is read when a call is enqueued; a value that differs between the forward and the backward
 * of one step is not refused (either forward's out / lse is a valid input to either backward), but recompute's bit-identity holds only with the switch held
 * constant over the step. */
int gg_clip_set_attention16_train(int on);

#ifdef __cplusplus
}
#endif
#endif
