/* libgg -- long-sequence attention forward on the 16-bit matrix pipe ("Attention beyond 256 tokens on the 16-bit MFMA"): the online-softmax forward
 * for rows the register-resident kernels of csrc/attention.hip cannot hold (CLIP ViT-L/14-336: 577 tokens), with both products on v_mfma_f32_16x16x32_{f16,bf16}
 * instead of the f32 MFMA of gg_attention_flash_fwd (dtype 0 / 2), and the opt-in switch that routes the CLIP vision tower's inference forward to it.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Arithmetic contract (tests/attention_cases.py, attention_math(..., rnd = storage); tests/test_attention16_cpu.py restates the tiled form on the CPU):
 *   scores       S = Q K^T on the 16-bit MFMA with f32 accumulation, scaled in f32 into the exp2 domain (s * scale * log2 e);
 *   softmax      online over 64-key tiles in f32: running maximum m, P = exp2(s - m), the row sum l is taken from the UNROUNDED P;
 *   P V          P rounded to the storage type once, as the operand of the product; O accumulated in f32 (rescaled when m moves), divided by l and rounded to the
 *                storage type once, on store;
 *   lse          m ln 2 + log l, f32;
 *   padding      keys beyond tokens_per_window in the last tile never enter the maximum or the sum; query rows beyond it are not stored.
 * No atomics and a fixed summation order: two calls give the same bits, and a window's result does not depend on num_windows. */
#ifndef GG_ATTN16_H
#define GG_ATTN16_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out [tokens][ldo] (head h at column h * 64) and, when args->lse is given, lse f32 [tokens][num_heads], from qkv [tokens][ld] in the storage type `dtype` names:
 * 0 = bf16, 2 = fp16 (gg_attention_flash_fwd's codes; 1 and 3 -- f32 storage -- are refused).  Of GgAttnArgs it reads qkv, ld, q_off, k_off, v_off, head_stride
 * (both qkv layouts of gg_attention_flash_fwd), head_dim (64), num_heads, num_windows, tokens_per_window (>= 1, any), window_size (0: linear tokens), scale (any),
 * out, ldo, lse.  Alignment as gg_attention_flash_fwd's: qkv and out 16-byte aligned, ld, ldo, the offsets and head_stride multiples of 4 elements (on gfx950
 * either pitch compiles to one 16-byte load per 8 elements).  head_dim != 64, window_size != 0, bias, bias_table, window_map and num_windows_dev are refused by name. */
int gg_attention_flash16_fwd(const GgAttnArgs* args, int dtype, void* stream);
/* launches of gg_attention_flash16_fwd's kernel enqueued by this process so far (tests count routes with it) */
int64_t gg_attention_flash16_calls(void);

/* on != 0: an INFERENCE forward of the CLIP vision tower (gg_clip_forward with training == 0: nothing kept) in the bf16 (0), fp16 (2) and fp8 (8) modes sends the
 * attention of rows beyond 256 tokens to gg_attention_flash16_fwd -- num_layers launches per forward.  Every other route is as before whatever the switch says: the
 * training forward and the backward's recompute, fp32 and fp32_split, the text tower, rows of at most 256 tokens, TinyViT.  Process-wide, default 0; returns the
 * previous value (gg_tinyvit_set_drop_compact's pattern).  The switch is read when a forward is enqueued; gg_clip_forward captures no graph, so no cached graph
 * depends on it. */
int gg_clip_set_attention16(int on);

#ifdef __cplusplus
}
#endif
#endif
