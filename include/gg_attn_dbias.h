/* libgg -- the relative-position bias gradient of window attention as a kernel of its own that adds in a FIXED order ("Fixed-order bias
 * gradient"), and the opt-in switch that makes TinyViT's training step use it.  Every attention backward that produces attention_biases.grad bins dS into an
 * LDS table with float atomics, so the last bits of that one gradient vary between any two steps; dq / dk / dv do not depend on whether dbias was requested.
 * This entry computes the bias gradient alone, from the tensors the backward of the same block receives, without any float atomic.
 *
 * Same conventions as include/gg.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); `stream` is a hipStream_t, work is only enqueued;
 * every pointer is a caller-owned device pointer.  A refused call writes nothing.
 *
 * Arithmetic contract (tests/attention_dbias_cases.py restates the order of the adds on the CPU):
 *   scores       S = Q K^T: dtype 0 on v_mfma_f32_16x16x32_bf16 of the stored bf16 operands, dtype 1 and 3 on v_mfma_f32_16x16x4_f32 of the stored f32
 *                operands (eight steps per 16 x 16 block); f32 accumulation either way.  dtype 3's split planes are not formed: the gradient is a sum over
 *                thousands of pairs;
 *   P            exp2(fma(S, scale log2 e, b2 - lse log2 e)) in f32 from the forward's lse (no maximum is subtracted again), b2 = bias_table[h][|dy| * ws +
 *                |dx|] * log2 e, or, with round_bias, f32(bf16(bias_table[..] / scale)) * scale log2 e: the value gg_attention_fwd's expanded table holds
 *                (`bias`, the expanded table itself, is not read: the rounding is restated from the compact table);
 *   dP, delta    dP = dO V^T on the same MFMA; delta_i = sum_d dO_id O_id in f32 from the stored `out`;
 *   dS           P (dP - delta) in f32, unrounded; a padded key or query of a ragged 16-token tile contributes exactly zero;
 *   order        workgroup (g, h) takes head h of windows g, g + G, g + 2 G, ... (G = min(num_windows, 512)) in that order; wave v of its four takes the 16-query
 *                strips v, v + 4, ... of a window, and 64-key tiles in ascending order inside a strip.  A strip's dS tile is laid into a wave-private LDS slot;
 *                lane l then owns |dx| = l mod 32 and the side l / 32 (0: key column = query column - |dx|, 1: + |dx|, |dx| > 0) and adds, for query rows in
 *                ascending order and key rows in ascending order, the one dS element at its offset into bin (|dy|, |dx|) of its wave's and side's table -- plain
 *                LDS reads and writes, no two lanes of an instruction on one bin.  The eight tables of a workgroup are added in (wave, side) order into partial
 *                row g of dbias_scratch; the rows go through the library's deterministic second stage (fp64, fixed order) and the result is ADDED to dbias.
 * The grid and the order of every add are functions of the arguments alone -- not of the device's CU count, of occupancy or of timing -- and there is no float
 * atomic in LDS or in memory: two calls on the same inputs give the same bits, whatever dbias_scratch held before. */
#ifndef GG_ATTN_DBIAS_H
#define GG_ATTN_DBIAS_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rows [num_heads][ws * ws] of args->dbias_scratch that gg_attention_dbias needs for these arguments: its partial rows (one per window group, min(num_windows,
 * 512)) plus the GG_REDUCE_SLICES (64) rows they are folded into.  Host arithmetic on the geometry alone (dtype, head_dim, window_size, map_h, map_w,
 * num_windows, tokens_per_window, num_heads, window_map): pointers other than window_map / num_windows_dev are not looked at.  < 0: refused, with the entry's
 * own text in gg_last_error(). */
int64_t gg_attention_dbias_rows(const GgAttnArgs* args, int dtype);

/* args->dbias[h][|dy| * ws + |dx|] += the sum over windows, queries q and keys k at that offset of dS[q][k] (above).  Of GgAttnArgs it reads what the backward of
 * the same block receives: qkv, ld, q_off, k_off, v_off, head_stride, head_dim (32), num_heads, num_windows, tokens_per_window (= window_size^2), window_size
 * (1 .. 32), map_h, map_w, bias_table (compact f32 [heads][ws * ws]), scale, out, ldo, lse (f32 [tokens][num_heads]), dout, lddo -- and writes only dbias (f32
 * [heads][ws * ws], ACCUMULATED into) and dbias_scratch (f32 [gg_attention_dbias_rows(args, dtype)][heads][ws * ws]; never read before it is written).  Token
 * (y, x) of window w is row img * H * W + (wy * ws + y) * W + wx * ws + x of the NHWC map.  `dtype`: 0 = bf16 storage of qkv / out / dout, 1 and 3 = f32 storage;
 * `round_bias`: GgAttnRoute.rounded_bias of the backward this call stands next to (include/gg_attn_route.h).  dqkv, ds_scratch and `bias` are ignored.
 * Alignment: qkv, out and dout 16-byte aligned with ld, ldo, lddo, the column offsets and head_stride multiples of 16 bytes (8 bf16 or 4 f32 elements); lse,
 * bias_table, dbias and dbias_scratch 4-byte aligned.  Refused by name: fp16 (dtype 2) and any other dtype, head_dim != 32, window_size == 0 (no window
 * geometry) or > 32, window_map / num_windows_dev, a missing qkv, lse, out, dout, bias_table, dbias or dbias_scratch, misalignment. */
int gg_attention_dbias(const GgAttnArgs* args, int dtype, int round_bias, void* stream);
/* calls of gg_attention_dbias enqueued by this process so far (tests count launches with it) */
int64_t gg_attention_dbias_calls(void);

/* on != 0: gg_tinyvit_backward hands the attention backward of every block whose attention_biases is trainable dbias = NULL and then launches
 * gg_attention_dbias on the same qkv / out / lse / dout, with the partial rows in the split-K region of its workspace (gg_attention_dbias_rows of them; the plan
 * is unchanged) -- on every route (the bf16 resident kernels, the f32 / split flash pair, the 16-bit-MFMA window pair under gg_tinyvit_set_attention16_train),
 * with recompute on or off, padded blocks included.  Every gradient of the step is then bit-reproducible, the attention_biases' too, and every other gradient
 * has the bits it has with the switch off.  (One route keeps its dbias: the f32 instantiation of the split single-pass kernel -- f32 storage, 7 x 7 / 12 x 12 /
 * 14 x 14 windows -- whose dq / dk / dv differ by an ulp between its with- and without-dbias forms; it bins into a table nobody reads, so that the other
 * gradients keep their bits.  Next to the resident bf16 kernels, which read the expanded table, round_bias is 1.)  A block whose table is frozen launches nothing new.  Process-wide, default 0; returns the previous value.  Read when
 * the backward is enqueued; part of the key of the graphs gg_tinyvit_backward captures for launch-bound sizes. */
int gg_tinyvit_set_deterministic_dbias(int on);

#ifdef __cplusplus
}
#endif
#endif
