/* libgg -- second header: the CLIP contrastive pre-training stage (text tower, contrastive head, gradient norm).
 *
 * The reference's pretrain_idun.py:205-300 trains a transformers CLIPModel on (image, caption) batches with return_loss=True, everything frozen
 * but visual_projection and logit_scale (freeze_backbone_keep_head, :220-239); tests/test_clip.py uses the same two towers for zero-shot prompts.
 * include/gg.h holds the vision tower; this header holds what that stage needs besides.  Same conventions as gg.h (and the same libgg.so):
 * 0 on success, < 0 on error with gg_last_error(); caller-owned DEVICE pointers unless marked "host"; `stream` is a hipStream_t, work is only
 * enqueued; a refused call has written nothing (what is refused is shape and configuration: the VALUES of index tensors -- input_ids, eos_pos -- are data the
 * C call never reads on the host; the kernels clamp them into range and the Python layer refuses them by message).
 */
#ifndef GG_CLIP_TEXT_H
#define GG_CLIP_TEXT_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- causal attention, forward (transformers CLIPTextTransformer, is_causal=True)
 * GgAttnArgs as gg_attention_flash_fwd reads it: linear tokens (window_size 0), head_dim 64, no bias (bias, bias_table NULL), lse optional.  Query t
 * of a sequence sees keys 0..t of the same sequence.  dtype 1 and 3 (f32 storage): the six-product split-bf16 arithmetic of gg_attention_flash_fwd's
 * dtype 3 in both cases (same kernel, same bits); dtype 0: bf16 storage, f32 arithmetic (the bf16 online-softmax forward).  Key tiles wholly above the
 * query tile are not visited, the diagonal tile is masked before the running maximum: a masked key contributes an exact 0.
 * Refused: head_dim != 64, a bias, windows, dtype 2, tokens_per_window > GG_CLIP_TEXT_MAX_POSITIONS. */
#define GG_CLIP_TEXT_MAX_POSITIONS 77
int gg_attention_causal_fwd(const GgAttnArgs* args, int dtype, void* stream);

/* ---------------------------------------------------------------- CLIP text tower, forward (frozen weights; inference workspace)
 * transformers CLIPTextModel: token + position embedding, num_layers pre-LN encoder layers with causal attention and QuickGELU (the vision tower's
 * layer schedule through the same GEMM routes of act_dtype 0 / 1 / 3), final_layer_norm, pooled = the final_layer_norm row at eos_pos[b].
 * Parameters: one flat f32 buffer, HF state-dict names without the "text_model." prefix (gg_clip_text_tensor_info); every tensor starts at a
 * multiple of 8 floats.  The weight cache holds the fused [3D][D] qkv matrix, out_proj, fc1, fc2 (and their bf16 planes in mode 3) as the vision
 * tower's does.  act_dtype 2 (fp16) is refused.  Right-padding needs no mask: under the causal mask a pad token cannot reach a row at or before
 * eos_pos[b]; rows after it are defined (finite for finite weights) but mean nothing. */
typedef struct GgClipTextCfg {
    int hidden_size, intermediate_size, num_layers, num_heads, vocab_size, max_positions;
    float ln_eps;
    int act_dtype;                         /* 0 bf16, 1 fp32, 3 fp32_split */
} GgClipTextCfg;
int gg_clip_text_num_tensors(const GgClipTextCfg* cfg);
int gg_clip_text_tensor_info(const GgClipTextCfg* cfg, int i, char* name /* host */, int name_cap, int64_t* offset, int64_t* numel, int* ndim, int64_t* shape4 /* host[4] */);
int64_t gg_clip_text_param_floats(const GgClipTextCfg* cfg);
int64_t gg_clip_text_wcache_bytes(const GgClipTextCfg* cfg);
int64_t gg_clip_text_workspace_bytes(const GgClipTextCfg* cfg, int batch, int tokens);
int gg_clip_text_refresh_weights(const GgClipTextCfg* cfg, const float* params, void* wcache, void* stream);
/* input_ids: int32 [batch][tokens]; the caller guarantees 0 <= id < vocab_size (an id outside is clamped into the table by the gather, never read
 * outside it).  eos_pos: int32 [batch], each in [0, tokens) (the Python layer refuses anything else in the same host check as the ids; the pooling
 * gather clamps).  last_hidden: f32 (batch, tokens, hidden) after final_layer_norm, or NULL.  pooled: f32 (batch, hidden).
 * Refused: act_dtype 2, tokens > max_positions or > GG_CLIP_TEXT_MAX_POSITIONS, head dim != 64. */
int gg_clip_text_forward(const GgClipTextCfg* cfg, int batch, int tokens, const float* params, const void* wcache, const int32_t* input_ids,
                         const int32_t* eos_pos, void* workspace, float* last_hidden, float* pooled, void* stream);

/* ---------------------------------------------------------------- contrastive head (transformers CLIPModel.forward after the projections; clip_loss)
 * img [Bi][P], txt [Bt][P]: f32 projection outputs, not normalised (row pitch ldi / ldt, multiples of 4).  Forward:
 *   img_n = img / |img|, txt_n = txt / |txt| (rows), logits_per_text [Bt][Bi] = exp(*logit_scale) * txt_n . img_n^T, logits_per_image its transpose.
 * want_loss (needs Bi == Bt == B): loss = (CE_rows + CE_cols) / 2 against the diagonal, and the gradients of
 * d_loss_scale * loss:  dS = (softmax_rows + softmax_cols - 2 I) / (2B);  d_logit_scale = sum dS o S;  d txt_n = exp(ls) dS . img_n,
 * d img_n = exp(ls) dS^T . txt_n;  through the normalisation dx = (dn - n (n . dn)) / |x|  ->  d_txt [Bt][P], d_img [Bi][P] (contiguous; either may be NULL).
 * Log-softmax is formed as torch forms it, (s - max) - log(sum exp(s - max)): the row / column maxima and the logs of the sums are kept as separate vectors
 * (their f32 sum would be an ulp of the maximum off, 7.6e-6 at a logit of 100), the sum of the f32 exponentials and its log are taken in double, a softmax term
 * is exp((s - max) - logsum), on the diagonal dS is expm1 + expm1, and a row's loss is (logsum_r - (s_rr - max_r)) + (logsum_c - (s_rr - max_c)).
 * exp(*logit_scale) is the double exponential rounded once.  A row's norm is summed in double and the row divided by it there, every element of img_n / txt_n
 * rounded once; the cosines are sums in double of the (exact) products of those f32 elements, times exp(ls), rounded once.
 * The gradient products are gg_gemm_nt_f32 launches; the reductions are fixed-order trees (no atomics: two calls
 * give the same bits).  scratch: gg_clip_contrastive_scratch_floats(Bi, Bt, P) floats, 16-byte aligned. */
typedef struct GgContrastiveArgs {
    const float* img; int64_t ldi;
    const float* txt; int64_t ldt;
    int Bi, Bt, P;
    const float* logit_scale;             /* device scalar (the parameter, a log) */
    float* img_n; float* txt_n;           /* f32 [Bi][P], [Bt][P]: image_embeds / text_embeds */
    float* logits_per_text;               /* f32 [Bt][Bi] */
    float* logits_per_image;              /* f32 [Bi][Bt] or NULL */
    int want_loss;
    float d_loss_scale;                   /* incoming gradient of the loss (1 for loss.backward()) */
    float* loss;                          /* f32 scalar */
    float* d_logit_scale;                 /* f32 scalar, WRITTEN (not accumulated), or NULL */
    float* d_img; float* d_txt;           /* f32 [Bi][P], [Bt][P], WRITTEN, or NULL */
    float* scratch;
} GgContrastiveArgs;
int64_t gg_clip_contrastive_scratch_floats(int Bi, int Bt, int P);
int gg_clip_contrastive(const GgContrastiveArgs* args, void* stream);
/* pooled[b][:] = x[b][pos[b]][:]  (x f32 (B, T, C), pos device int32 [B], clamped into [0, T)); the backward scatters: dx zero-filled, row pos[b] = dpooled[b].
 * The vision tower's pooler_output takes row 0 (pos NULL = all zeros). */
int gg_row_gather_f32(const float* x, const int32_t* pos, float* pooled, int B, int T, int C, void* stream);
int gg_row_scatter_f32(const float* dpooled, const int32_t* pos, float* dx, int B, int T, int C, void* stream);

/* ---------------------------------------------------------------- gradient-norm clipping (torch.nn.utils.clip_grad_norm_; HF max_grad_norm)
 * Sum of squares of n floats in two deterministic stages: block partials (double) into scratch, then one block adds them in index order.
 * out[0] (double, device) = accumulate ? out[0] + sum : sum.  scratch: gg_grad_sq_norm_scratch_doubles(n) doubles. */
int64_t gg_grad_sq_norm_scratch_doubles(int64_t n);
int gg_grad_sq_norm(const float* g, int64_t n, double* scratch, double* out, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
