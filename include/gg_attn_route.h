/* libgg -- the route of an attention call ("One attention route"): which kernel a public attention entry point launches for its arguments, in how
 * many passes, on what grid, and what scratch it consumes.  The entry points execute this struct and gg_attention_route reports it: one decision (csrc/
 * attention.hip, attn_route; csrc/attention_flash.hip, flash_route; one route per flash16 entry), development switches included, so a planner, an encoder
 * or a test that asks about its arguments cannot be told about another kernel than the one the launch runs.
 *
 * Same conventions as include/gg.h (and the same libgg.so).  Host arithmetic only: no HIP call, no launch, no device. */
#ifndef GG_ATTN_ROUTE_H
#define GG_ATTN_ROUTE_H
#include <stdint.h>
#include "gg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the public attention entry points */
enum {
    GG_ATTN_ENTRY_FWD = 0,          /* gg_attention_fwd (`dtype` is ignored: bf16 storage) */
    GG_ATTN_ENTRY_FWD_F16,          /* gg_attention_fwd_f16 (`dtype` is ignored: fp16 storage) */
    GG_ATTN_ENTRY_BWD,              /* gg_attention_bwd (`dtype` is ignored: bf16 storage) */
    GG_ATTN_ENTRY_FLASH_FWD,        /* gg_attention_flash_fwd */
    GG_ATTN_ENTRY_FLASH_BWD,        /* gg_attention_flash_bwd */
    GG_ATTN_ENTRY_CAUSAL_FWD,       /* gg_attention_causal_fwd (include/gg_clip_text.h) */
    GG_ATTN_ENTRY_CAUSAL_BWD,       /* gg_attention_causal_bwd (include/gg_clip_text_train.h) */
    GG_ATTN_ENTRY_FLASH16_FWD,      /* gg_attention_flash16_fwd (include/gg_attn16.h) */
    GG_ATTN_ENTRY_FLASH16_WIN_FWD,  /* gg_attention_flash16_win_fwd (include/gg_attn16w.h) */
    GG_ATTN_ENTRY_FLASH16_BWD,      /* gg_attention_flash16_bwd (include/gg_attn16b.h) */
    GG_ATTN_ENTRY_FLASH16_WIN_BWD,  /* gg_attention_flash16_win_bwd (include/gg_attn16wb.h) */
    GG_ATTN_ENTRY_COUNT
};

/* the kernels (function templates of csrc/; storage type, head dim and the causal mask follow from the entry, `dtype` and head_dim; `variant` names the rest) */
enum {
    GG_ATTN_KERNEL_NONE = 0,
    GG_ATTN_KERNEL_FWD,               /* attn_fwd_kernel: one window per workgroup, full-row softmax in registers; variant = key tiles 4 / 10 / 14 / 16 */
    GG_ATTN_KERNEL_FWD_GROUPED,       /* attn_fwd_small_kernel: 8 windows of at most 64 tokens per workgroup */
    GG_ATTN_KERNEL_BWD,               /* attn_bwd_kernel; variant = key tiles 4 / 10 / 14 / 16 */
    GG_ATTN_KERNEL_BWD_GROUPED,       /* attn_bwd_small_kernel: 8 windows per workgroup */
    GG_ATTN_KERNEL_FLASH_FWD_RESIDENT,/* flash_fwd_kernel<RES = true>: the whole window in LDS; variant 1 = with the cooperative tail strip */
    GG_ATTN_KERNEL_FLASH_FWD_STREAM,  /* flash_fwd_kernel<RES = false>: one workgroup per 64-query tile */
    GG_ATTN_KERNEL_FLASH_FWD_SPLIT,   /* flash_fwd_split_kernel (f32 storage, head dim 32, split-bf16 products); variant = strips 4 / 9 / 13 */
    GG_ATTN_KERNEL_FLASH64_FWD_SPLIT, /* flash64_split_q_kernel<3, false>: dtype 3 and the f32 causal forward */
    GG_ATTN_KERNEL_FLASH_BWD_SPLIT,   /* flash_bwd_split_kernel: single pass, head dim 32 (f32: split products; bf16: one plane); variant = strips 4 / 9 / 13 */
    GG_ATTN_KERNEL_FLASH_BWD_FUSED,   /* flash_bwd_fused_kernel: single pass; variant = its strip specialisation 13 / 4 / 0 */
    GG_ATTN_KERNEL_FLASH_BWD_STREAM,  /* flash_bwd_dq_kernel, then flash_bwd_dkv_kernel: both recompute P */
    GG_ATTN_KERNEL_FLASH_BWD_STREAM_DS,/* flash_bwd_dkv_kernel<STORE_DS>, then flash_bwd_dq_ds_kernel: dS handed over in ds_scratch */
    GG_ATTN_KERNEL_FLASH64_BWD_SPLIT, /* flash64_split_q_kernel<3, true>, then flash64_split_dkv_kernel<3>: dtype 3 and the f32 causal backward */
    GG_ATTN_KERNEL_FLASH16_FWD,       /* flash16_fwd_kernel, linear tokens, head dim 64 */
    GG_ATTN_KERNEL_FLASH16_WIN_FWD,   /* flash16_fwd_kernel, windows, head dim 32; variant 1 = with the bias table */
    GG_ATTN_KERNEL_FLASH16_BWD,       /* flash16_bwd_dkv_kernel, then flash16_bwd_dq_kernel, linear tokens, head dim 64 */
    GG_ATTN_KERNEL_FLASH16_WIN_BWD,   /* the same pair, windows, head dim 32; variant 0 = no bias, 1 = bias table, 2 = bias table and its gradient */
    GG_ATTN_KERNEL_COUNT
};

typedef struct GgAttnRoute {
    int kernel;                       /* GG_ATTN_KERNEL_* */
    int variant;                      /* the kernel's specialisation (see the enum); 0 where it has none */
    int passes;                       /* kernel launches, 1 or 2, in launch order in `pass` (the bias gradient's second stage is not counted) */
    struct { uint32_t grid, block, lds; } pass[2];      /* workgroups, threads per workgroup, dynamic LDS bytes */
    int64_t dbias_rows;               /* rows [num_heads][ws * ws] of dbias_scratch that the route's second stage needs with args->dbias set: its partial rows
                                         plus the GG_REDUCE_SLICES (64) rows they are folded into.  0: no dbias in the call, so no second stage */
    int reads_ds_scratch;             /* 1: the route reads and writes args->ds_scratch (it is given and the route is the two-pass hand-off form) */
    int rounded_bias;                 /* 1: P is recomputed with the bias as bf16(bias / scale), the value gg_attention_fwd's expanded table holds */
} GgAttnRoute;

/* The route `entry` (GG_ATTN_ENTRY_*) executes for exactly these arguments and this `dtype` (the entry's own dtype code; ignored by the entries that take
 * none) under the development switches of this process: 0 and *out filled, or -1 with the entry's own refusal text in gg_last_error().  Pointers of `args`
 * are tested for null and alignment only and never dereferenced; window_map / num_windows_dev are never read -- their being non-null is the input. */
int gg_attention_route(const GgAttnArgs* args, int entry, int dtype, GgAttnRoute* out);

#ifdef __cplusplus
}
#endif
#endif
