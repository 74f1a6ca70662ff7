/* libgg -- window attention backward beyond 256 tokens on the 16-bit matrix pipe ("TinyViT training beyond 256 tokens on the 16-bit MFMA"): the
 * two-pass backward of include/gg_attn16b.h for head dim 32, tokens gathered from the windows of an NHWC map, the relative-position bias inside P and the bias
 * gradient -- the stage-2 blocks of tiny_vit_21m_384 (24 x 24 = 576 tokens) and tiny_vit_21m_512 (32 x 32 = 1024 tokens), which gg_attention_bwd sends to the
 * f32-MFMA streaming pair of gg_attention_flash_bwd -- and the opt-in switch that routes TinyViT's bf16 TRAINING step to the 16-bit-MFMA kernels.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Arithmetic contract (tests/attention16_win_bwd_cases.py restates the tiled form on the CPU):
 *   scores       S = Q K^T on v_mfma_f32_16x16x32_bf16 with f32 accumulation (one MFMA per 16 x 16 block: k = the whole head dim);
 *   P            exp2(fma(acc, scale log2 e, b2 + nl)) in f32, where b2 = bias_table[h][|dy| * ws + |dx|] * log2 e in f32 (the f32 parameter unrounded, as the
 *                forward's pre-multiplied signed-offset table holds it; 0 without a table) and nl = -lse log2 e in f32, from the forward's lse: no maximum is
 *                subtracted again;
 *   dP           dO V^T on the same MFMA;
 *   delta        delta_i = sum_d dO_id O_id in f32, from the stored bf16 `out`;
 *   dS           P (dP - delta) in f32;
 *   dV           P rounded to bf16 once, as the operand of dV = P^T dO;
 *   dK, dQ       dS rounded to bf16 once, as the operand of dK = dS^T Q and dQ = dS K;
 *   store        the three accumulators are f32; dq and dk are multiplied by `scale` in f32; each gradient is rounded to bf16 once, on store;
 *   padding      keys and queries beyond tokens_per_window in a ragged tile contribute exactly zero and are never stored;
 *   dbias        dbias[h][|dy| * ws + |dx|] += the sum over windows, queries and keys of the UNROUNDED f32 dS: binned by signed offset in an LDS table of
 *                (2 ws - 1)^2 floats with LDS float adds in the dK / dV pass, folded onto |dy|, |dx| at the end of the workgroup, one partial row per workgroup
 *                (window, 128-key block) into dbias_scratch and a second stage that sums the rows in a fixed order; without a scratch, global float atomics.
 * dq, dk and dv use no atomics and a fixed summation order: two calls give the same bits, and they depend neither on whether dbias was requested, nor on
 * num_windows, nor on where a window lies in its map.  dbias is NOT bit-reproducible (LDS adds land in no fixed order).  The forward's out / lse may come from
 * gg_attention_flash16_win_fwd or from gg_attention_fwd / gg_attention_flash_fwd (dtype 0): either is a valid input. */
#ifndef GG_ATTN16WB_H
#define GG_ATTN16WB_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* dqkv [tokens][ld] (the dq, dk and dv columns of every live token, at qkv's ld, column offsets and head_stride; nothing else is written) and, when args->dbias is
 * given, dbias f32 [num_heads][ws * ws] (ACCUMULATED into), from qkv, the forward's out [tokens][ldo] and lse f32 [tokens][num_heads], and dout [tokens][lddo]
 * (head h at column h * 32 of out and dout).  Tokens are those of gg_attention_flash16_win_fwd: token (y, x) of window w is row
 * img * H * W + (wy * ws + y) * W + wx * ws + x of the NHWC map.  `dtype` must be 0 (bf16): 2 is refused ("fp16 storage is inference-only"), 1 and 3 are f32
 * storage.  Of GgAttnArgs it reads the forward's fields -- qkv, ld, q_off, k_off, v_off, head_stride, head_dim (32), num_heads, num_windows, tokens_per_window
 * (= window_size^2), window_size (1 .. 32), map_h, map_w, bias_table (compact f32 [heads][ws * ws] or NULL), scale -- plus out, ldo, lse, dout, lddo, dqkv, dbias
 * (or NULL) and dbias_scratch (f32 [gg_attention_flash16_win_dbias_rows(...)][num_heads][ws * ws] or NULL; read only with dbias); ds_scratch is ignored, `bias`
 * (the expanded bf16 table) is ignored next to bias_table.  Alignment: qkv, out, dout and dqkv 16-byte aligned, ld, ldo, lddo, the offsets and head_stride
 * multiples of 4 elements.  Refused by name: head_dim != 32, window_size == 0 or > 32, bias without bias_table, dbias without bias_table, window_map,
 * num_windows_dev, a missing lse, out, dout or dqkv, misalignment. */
int gg_attention_flash16_win_bwd(const GgAttnArgs* args, int dtype, void* stream);
/* calls of gg_attention_flash16_win_bwd enqueued by this process so far: one count per call, however many kernels it launches (tests count routes with it) */
int64_t gg_attention_flash16_win_bwd_calls(void);
/* partial rows of dbias_scratch a caller must provide: one per workgroup of the dK / dV pass and head (num_windows * ceil(tokens_per_window / 128)) plus the
 * GG_REDUCE_SLICES (64) rows the second stage folds into -- the entry's one route (GgAttnRoute.dbias_rows of include/gg_attn_route.h) */
int64_t gg_attention_flash16_win_dbias_rows(int num_windows, int tokens_per_window);

/* on != 0: a TRAINING step of TinyViT in the bf16 mode (act_dtype 0) sends the attention of every block whose window gg_attention_fwd would hand to
 * gg_attention_flash_fwd (more than 256 tokens) -- the training forward (gg_tinyvit_forward with training != 0, with lse), the recompute replay inside
 * gg_tinyvit_backward, and the attention backward, padded blocks included -- to gg_attention_flash16_win_fwd / gg_attention_flash16_win_bwd.  Every other route is
 * as before whatever the switch says: inference forwards (gg_tinyvit_set_attention16 is theirs), fp32 and fp32_split, windows of at most 256 tokens, CLIP.  The
 * workspace plan is unchanged.  Process-wide, default 0; returns the previous value.  The switch is read when a call is enqueued and is part of the keys of the
 * graphs gg_tinyvit_forward and gg_tinyvit_backward capture for launch-bound sizes.  A value that differs between the forward and the backward of one step is not
 * refused (either forward's out / lse is a valid input to either backward), but recompute's bit-identity holds only with the switch held constant over the step. */
int gg_tinyvit_set_attention16_train(int on);

#ifdef __cplusplus
}
#endif
#endif
