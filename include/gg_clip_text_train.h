/* libgg -- third header: training the CLIP text tower (causal attention backward, token-embedding scatter-add, the tower's training forward and backward).
 *
 * Fine-tuning both towers under the contrastive loss is the standard use of a CLIP checkpoint (PIGEON, which the reference re-implements, does it).
 * include/gg_clip_text.h holds the frozen text tower and the contrastive head; this header holds what training the tower needs besides.  Same conventions
 * as gg.h and gg_clip_text.h (and the same libgg.so): 0 on success, < 0 on error with gg_last_error(); caller-owned DEVICE pointers unless marked "host";
 * `stream` is a hipStream_t, work is only enqueued; a refused call has written nothing.  No entry point here uses an atomic: two calls give the same bits.
 */
#ifndef GG_CLIP_TEXT_TRAIN_H
#define GG_CLIP_TEXT_TRAIN_H
#include <stdint.h>
#include "gg.h"
#include "gg_clip_text.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- causal attention, backward (of gg_attention_causal_fwd)
 * GgAttnArgs as gg_attention_flash_bwd reads it, on the forward's geometry: linear tokens, head_dim 64, no bias.  Reads qkv, out, lse (the forward's) and dout
 * (row pitch lddo); writes ALL of dqkv (the q | k | v columns of every token of every head; same pitch and offsets as qkv).  ds_scratch is not read.
 * dtype 1 and 3 (f32 storage): the split-bf16 product arithmetic of gg_attention_flash_bwd's dtype 3 in both cases (same kernels, same bits), as two passes
 * (dQ; dK and dV) that each recompute P from lse; dtype 0: bf16 storage, f32 arithmetic, one pass.  Key tiles / strips wholly above the diagonal are not
 * visited; on the diagonal a masked score becomes -inf before the exponent, so its P, its dS and its contributions to dK and dV are exact zeros.
 * Refused: head_dim != 64, a bias, windows, dtype 2, tokens_per_window > GG_CLIP_TEXT_MAX_POSITIONS. */
int gg_attention_causal_bwd(const GgAttnArgs* args, int dtype, void* stream);

/* ---------------------------------------------------------------- token-embedding gradient: dtable[id] += sum over the rows r with ids[r] == id of dx[r]
 * dx f32 [rows][D] (D % 4 == 0), ids int32 [rows] (clamped into [0, vocab) exactly as the forward's gather clamps them), dtable f32 [vocab][D], ACCUMULATED.
 * Row r leads its id when no earlier row carries the same id; the leader's workgroup adds the matching rows in index order onto the table row: a fixed
 * summation order per table row, no float atomics.  Only the table rows that occur are touched; the table is never streamed.
 * scratch: gg_embedding_scatter_add_scratch_bytes(rows) bytes, 16-byte aligned (the clamped ids and each row's leader flag). */
int64_t gg_embedding_scatter_add_scratch_bytes(int64_t rows);
int gg_embedding_scatter_add_f32(const float* dx, const int32_t* ids, float* dtable, int64_t rows, int D, int vocab, void* scratch, void* stream);

/* ---------------------------------------------------------------- CLIP text tower, training forward and backward
 * `trainable`: host, one byte per tensor of gg_clip_text_tensor_info's table, or NULL = everything trains.  The layers from the first trained one up keep the
 * tensors their backward reads (as the vision tower's: layer input, both LayerNorm outputs + statistics, qkv, attention output + lse, fc1 pre-activation and
 * activation), the layers below run the inference schedule; when one of the two embedding tables trains every layer is kept.  No activation recompute.
 * gg_clip_text_first_trained_layer: that layer (num_layers: no layer is kept -- nothing below final_layer_norm trains).
 * gg_clip_text_train_workspace_bytes: with nothing trainable the inference size (gg_clip_text_workspace_bytes).
 * gg_clip_text_forward_train: pooled / last_hidden bit-identical to gg_clip_text_forward's (same kernels, same arguments; only where the kept tensors go differs).
 * Refused: act_dtype 2, tokens > max_positions or > GG_CLIP_TEXT_MAX_POSITIONS, head dim != 64. */
int64_t gg_clip_text_train_workspace_bytes(const GgClipTextCfg* cfg, int batch, int tokens, const uint8_t* trainable /* host */);
int gg_clip_text_first_trained_layer(const GgClipTextCfg* cfg, const uint8_t* trainable /* host */);
int gg_clip_text_forward_train(const GgClipTextCfg* cfg, int batch, int tokens, const float* params, const void* wcache, const int32_t* input_ids,
                               const int32_t* eos_pos, void* workspace, float* last_hidden, float* pooled, const uint8_t* trainable /* host */, void* stream);
/* Backward of the training forward that last wrote `workspace` (same cfg, batch, tokens, ids, eos_pos and mask).  d_pooled: f32 (batch, hidden) or NULL, scattered
 * to the EOS rows; d_last_hidden: f32 (batch, tokens, hidden) or NULL (both given: summed; one of them is required).  final_layer_norm's backward, the layer loop
 * of gg_clip_backward with gg_attention_causal_bwd, then -- only when an embedding table trains -- the token scatter-add and the position sum
 * dpos[t] += sum_b dx[b,t,:].  Gradients of the trainable tensors are ACCUMULATED into `grads` (flat, the offsets of params); a frozen tensor's range is never
 * written.  The all-zero mask returns 0 and touches nothing. */
int gg_clip_text_backward(const GgClipTextCfg* cfg, int batch, int tokens, const float* params, const void* wcache, const int32_t* input_ids,
                          const int32_t* eos_pos, void* workspace, const float* d_pooled, const float* d_last_hidden, float* grads,
                          const uint8_t* trainable /* host */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
