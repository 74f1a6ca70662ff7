/* libgg -- DropPath row compaction of the fp32_split TinyViT training step.  Same conventions as include/gg.h: 0 on success, caller-owned device
 * pointers, work only enqueued on `stream`.  The row-compaction fields of GgSplit3Args (groups_dev, group_rows, a_map, c_map) and GgAttnArgs (window_map,
 * num_windows_dev) are declared with those structs in include/gg.h and take the lists this header's kernel writes. */
#ifndef GG_DROP_H
#define GG_DROP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* A dropped sample's branch is multiplied by zero in forward and gets a zero
 * gradient in backward, so its rows are left out of the branch's kernels.  gg_drop_kept_lists: per slot of `scales` [slots][batch] (gg_drop_path_scales; kept <=>
 * scale != 0) one list of gg_drop_list_ints(batch) ints: [count, batch, 0, 0][kept: the kept sample indices, ascending -- count of them][pos: per sample its index
 * among the kept ones, or -1], kept at GG_DROP_LIST_HEAD, pos at GG_DROP_LIST_HEAD + batch.  One launch, a block scan, no atomics, nothing read back.
 * The _map forms of the LayerNorm kernels (f32, C <= 640; pos = that array): gg_layernorm_fwd_bn_f32_map writes xout / mean / rstd for every row, `out` compact
 * (row pos[sample] * rows_per_sample + row within the sample; kept samples only) and copies xout to xcopy on the dropped samples' rows (xcopy optional);
 * gg_layernorm_bwd_map reads dout compact and takes zeros for the dropped samples (dx = dres there) -- part == NULL: gg_layernorm_bwd without parameter
 * gradients, part given: gg_layernorm_bwd_colsum (same partial rows, same order).  Results equal the unmapped calls' on scattered / gathered tensors bit for bit. */
#define GG_DROP_LIST_HEAD 4
int gg_drop_list_ints(int batch);
int gg_drop_kept_lists(const float* scales, int slots, int batch, int* lists, void* stream);
int gg_layernorm_fwd_bn_f32_map(const float* y, const float* bn_stat, const float* bn_gamma, const float* bn_beta, float* xout, const float* gamma, const float* beta,
                                int64_t M, int C, float eps, float* out, float* mean, float* rstd, const int* pos, int rows_per_sample, float* xcopy, void* stream);
int gg_layernorm_bwd_map(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma, int64_t M, int C, const float* dres, float* dx,
                         float* part, const int* pos, int rows_per_sample, void* stream);

/* DropPath row compaction of the training step (act_dtype 3, a drop_scales array given): in a stage-2 block whose every parameter is frozen and whose eight Linear
 * launches all take the 256 x 128 split GEMM (width >= 384: the 21M variants), the kept samples' rows are compacted -- the MLP branch (forward and backward) and the
 * backward of the attention branch run over the kept rows only.  The kept lists are derived on the device from drop_scales (one small launch in front of such a block's
 * forward, recompute replay and backward, into scratch memory the frozen block leaves idle: the workspace plan is unchanged), nothing is read back, and everything a
 * step returns is bit-identical to the uncompacted schedule.
 * on != 0 (the default) / 0: process-global; returns the previous value.  For A/B runs and tests; set it between steps, not between a forward and its backward. */
int gg_tinyvit_set_drop_compact(int on);

#ifdef __cplusplus
}
#endif
#endif
