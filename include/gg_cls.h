/* libgg -- fourth header: the TinyViT country-classifier fine-tune (the reference's finetune_tinyvit/ stage).
 *
 * finetune_tinyvit/train_tinyvit_timm.py trains timm's tiny_vit_*(num_classes = C) with nn.CrossEntropyLoss and tracks timm.utils.accuracy top-1 / top-5;
 * extract_embeddings.py exports the pooled last feature map.  include/gg.h holds the encoder and the GEMMs the classifier's Linear runs on; this header
 * holds what that stage needs besides: a cross-entropy head that knows nothing about geocells (gg_geo_head needs a centroid table and does haversine work
 * per class), and where the inference forward leaves the last stage's feature map.  Same conventions as gg.h (and the same libgg.so): 0 on success, < 0 on
 * error with gg_last_error(); caller-owned DEVICE pointers; `stream` is a hipStream_t, work is only enqueued; a refused call has written nothing.
 */
#ifndef GG_CLS_H
#define GG_CLS_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- classification head: cross-entropy, its gradient, rank of the label, arg-max
 * One pass per row over f32 logits [N][ldl] (C <= ldl valid columns):
 *   loss_rows[n] = logsumexp(logits[n][:C]) - logits[n][label]      (the row maximum is subtracted first; f32 accumulation)
 *   dlogits[n][c] = (softmax(logits[n])[c] - (c == label)) * grad_scale * (upstream ? *upstream : 1);  columns C..ldd-1 are written as zero
 *   rank[n]  = #{c : logits[n][c] > logits[n][label]} + #{c < label : logits[n][c] == logits[n][label]}
 *              -- top-k hit <=> rank < k: timm.utils.accuracy (topk, largest, sorted) for tie-free rows, without a sort and deterministic
 *   preds[n] = arg-max, lowest index on ties
 *   loss     = mean of loss_rows, summed in a fixed order (no float atomics: two calls give the same bits); needs loss_rows
 * A label outside [0, C) (torch's CrossEntropyLoss raises; a kernel cannot): loss_rows[n], the mean loss and row n of dlogits are NaN, rank[n] = C,
 * preds[n] is still the arg-max; nothing outside the row is read.
 * Rows of up to 1024 classes take one wave each (four rows per workgroup, the row held in registers), longer rows one workgroup each, looping.
 * Refused (nothing launched, nothing written): NULL args / logits / labels, N <= 0, C < 1, ldl < C, dlogits with ldd < C, loss without loss_rows, and any
 * pointer the runtime does not know as device memory (hipPointerGetAttributes: host and unregistered pointers). */
typedef struct GgClsHeadArgs {
    const float* logits; int64_t ldl;     /* f32 [N][ldl] */
    int N, C;
    const int64_t* labels;                /* int64 (N,) */
    float grad_scale;                     /* 1 / N for the gradient of the mean loss */
    const float* upstream;                /* device scalar multiplied into grad_scale (the incoming gradient of the loss), or NULL */
    float* loss_rows;                     /* f32 (N,) or NULL */
    float* loss;                          /* f32 scalar or NULL */
    void* dlogits; int64_t ldd;           /* bf16 (f32 if dlogits_f32) [N][ldd] or NULL */
    int dlogits_f32;
    int32_t* rank;                        /* int32 (N,) or NULL */
    int64_t* preds;                       /* int64 (N,) or NULL */
} GgClsHeadArgs;
int gg_cls_head(const GgClsHeadArgs* args, void* stream);

/* ---------------------------------------------------------------- feature export (timm forward_features; finetune_tinyvit/extract_embeddings.py)
 * Where gg_tinyvit_forward(training = 0) at this batch leaves the output of the last TinyVitBlock: byte offset and size inside the INFERENCE workspace of
 * the map [batch][res][res][embed_dims[3]] in the model's storage type (bf16, or f32 for act_dtype 1 / 3) -- the tensor in front of the global pool.  The
 * region is a slot of the inference ring that nothing after the last block writes, so it is valid from the end of that forward to the next one. */
int gg_tinyvit_last_map_info(const GgTinyVitCfg* cfg, int batch, int64_t* offset, int64_t* bytes, int* res, int* channels);

#ifdef __cplusplus
}
#endif
#endif
