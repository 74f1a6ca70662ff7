/* libgg -- window attention beyond 256 tokens on the 16-bit matrix pipe ("TinyViT windows beyond 256 tokens on the 16-bit MFMA"): the online-softmax
 * forward of include/gg_attn16.h for head dim 32, tokens gathered from the windows of an NHWC map and the relative-position bias -- the stage-2 blocks of
 * tiny_vit_21m_384 (24 x 24 = 576 tokens) and tiny_vit_21m_512 (32 x 32 = 1024 tokens), which gg_attention_fwd sends to gg_attention_flash_fwd (f32 MFMA) -- and
 * the opt-in switch that routes TinyViT's bf16 inference forward to it.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Arithmetic contract: that of include/gg_attn16.h plus the bias (tests/attention16_cases.py restates the tiled form on the CPU):
 *   scores       S = Q K^T on v_mfma_f32_16x16x32_bf16 with f32 accumulation, taken into the exp2 domain in f32 as
 *                acc * (scale * log2 e) + bias_table[h][|dy| * ws + |dx|] * log2 e -- the f32 parameter, unrounded, as gg_attention_flash_fwd reads it (not the
 *                bf16(bias / scale) of the register-resident kernels); the bias joins the score before the running maximum;
 *   softmax      online over 64-key tiles in f32: running maximum m, P = exp2(s - m), the row sum l from the UNROUNDED P;
 *   P V          P rounded to bf16 once, as the operand; O accumulated in f32 (rescaled when m moves), one true division by l and one rounding on store;
 *   lse          m ln 2 + log l, f32;
 *   padding      keys beyond tokens_per_window in the last tile never enter the maximum or the sum; query rows beyond it are not stored.
 * No atomics and a fixed summation order: two calls give the same bits, and a window's result depends neither on num_windows nor on where the window lies in
 * its map. */
#ifndef GG_ATTN16W_H
#define GG_ATTN16W_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out [tokens][ldo] (head h at column h * 32) and, when args->lse is given, lse f32 [tokens][num_heads], from bf16 qkv [tokens][ld]: `dtype` must be 0 (bf16;
 * TinyViT has no fp16 mode: 1, 2 and 3 are refused).  Token (y, x) of window w is row img * H * W + (wy * ws + y) * W + wx * ws + x of the NHWC map (H = map_h,
 * W = map_w, windows in row-major order within an image: gg_attention_flash_fwd's geometry and rules -- window_size divides map_h and map_w, num_windows is a
 * multiple of the windows per image).  Of GgAttnArgs it reads qkv, ld, q_off, k_off, v_off, head_stride (both qkv layouts; TinyViT's is 0 / 32 / 64, stride 96),
 * head_dim (32), num_heads, num_windows, tokens_per_window (= window_size^2), window_size (1 .. 32), map_h, map_w, bias_table (the compact f32 [heads][ws * ws]
 * table, or NULL: no bias), scale (any), out, ldo, lse.  `bias` (the expanded bf16 table of the register-resident kernels) is ignored next to bias_table and
 * refused without it.  Alignment as gg_attention_flash16_fwd's: qkv and out 16-byte aligned, ld, ldo, the offsets and head_stride multiples of 4 elements
 * (on gfx950 either pitch compiles to one 16-byte load per 8 elements).  head_dim != 32, window_size == 0 or > 32, window_map, num_windows_dev and dbias are refused by name. */
int gg_attention_flash16_win_fwd(const GgAttnArgs* args, int dtype, void* stream);
/* launches of gg_attention_flash16_win_fwd's kernel enqueued by this process so far (tests count routes with it; gg_attention_flash16_calls does not move) */
int64_t gg_attention_flash16_win_calls(void);

/* on != 0: an INFERENCE forward of TinyViT (gg_tinyvit_forward with training == 0) in the bf16 mode (act_dtype 0) sends the attention of every block whose window
 * gg_attention_fwd would hand to gg_attention_flash_fwd (more than 256 tokens) to gg_attention_flash16_win_fwd.  Every other route is as before whatever the switch
 * says: the training forward, the recompute replay and the backward, fp32 and fp32_split, windows of at most 256 tokens, CLIP.  Process-wide, default 0; returns
 * the previous value (gg_clip_set_attention16's pattern).  The switch is read when a forward is enqueued and is part of the key of the graph gg_tinyvit_forward
 * captures for launch-bound sizes: a graph captured under one setting is never replayed under the other. */
int gg_tinyvit_set_attention16(int on);

#ifdef __cplusplus
}
#endif
#endif
