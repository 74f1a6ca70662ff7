// The route of an attention call (include/gg_attn_route.h): what the attention sources share around the two decision functions -- attn_route
// (attention.hip: gg_attention_fwd / _fwd_f16 / _bwd) and flash_route (attention_flash.hip: the flash and the causal entries) -- and the one route of each
// flash16 entry.  A launcher computes the route once from checked arguments and switches on it; gg_attention_route (attention.hip) returns the same struct.
#pragma once
#include "common.h"
#include "../../include/gg.h"
#include "../../include/gg_attn_route.h"

// Every GG_ATTN_* development switch, read here once per process (gg_dev_env: only under GG_DEV_SWITCHES).  The first six belong to the two decision
// functions, no_ds_scratch to the encoders' entry pickers (tinyvit.hip, clip.hip: whether a planned dS region is passed at all).
struct AttnSwitches {
    bool no_split;          // GG_ATTN_NO_SPLIT: no split / single-plane single-pass kernels of attention_split.h
    bool no_grouped;        // GG_ATTN_SMALL=0: no grouped kernels for windows of at most 64 tokens
    bool no_fused_bwd;      // GG_ATTN_NO_FUSED_BWD: the two-pass backward at every length
    bool no_resident;       // GG_ATTN_FLASH_NO_RES: the streaming forward at every length
    bool fwd_no_tail;       // GG_ATTN_FWD_NO_TAIL: resident forward with a wave per strip
    bool fused_no_tail;     // GG_ATTN_FUSED_NO_TAIL: single-pass backward with a wave per strip
    bool no_ds_scratch;     // GG_ATTN_NO_DS_SCRATCH: the encoders pass no dS region
};
inline const AttnSwitches& attn_switches() {
    static const AttnSwitches s = [] {
        const char* small = gg_dev_env("GG_ATTN_SMALL");
        return AttnSwitches{gg_dev_env("GG_ATTN_NO_SPLIT") != nullptr,      small && small[0] == '0',
                            gg_dev_env("GG_ATTN_NO_FUSED_BWD") != nullptr,  gg_dev_env("GG_ATTN_FLASH_NO_RES") != nullptr,
                            gg_dev_env("GG_ATTN_FWD_NO_TAIL") != nullptr,   gg_dev_env("GG_ATTN_FUSED_NO_TAIL") != nullptr,
                            gg_dev_env("GG_ATTN_NO_DS_SCRATCH") != nullptr};
    }();
    return s;
}

// the routes of the other attention sources, for attn_route's forwards and for gg_attention_route: checks, decision, no launch
int gg_attn_route_flash(const GgAttnArgs* a, int entry, int dtype, int forward_rounded_bias, GgAttnRoute* out);      // attention_flash.hip
int gg_attn_route_flash16_fwd(const GgAttnArgs* a, int entry, int dtype, GgAttnRoute* out);                          // attention_flash16.hip
int gg_attn_route_flash16_bwd(const GgAttnArgs* a, int entry, int dtype, GgAttnRoute* out);                          // attention_flash16_bwd.hip
// gg_attention_flash_bwd with the forward's bias rounding named (attention_flash.hip): what gg_attention_bwd forwards to
int gg_attention_flash_bwd_impl(const GgAttnArgs* a, int dtype, int forward_rounded_bias, void* stream);

static inline void attn_route_pass(GgAttnRoute& r, int64_t grid, int block, size_t lds) {
    r.pass[r.passes].grid = (uint32_t)grid; r.pass[r.passes].block = (uint32_t)block; r.pass[r.passes].lds = (uint32_t)lds;
    ++r.passes;
}
// rows of dbias_scratch behind `part_rows` partial rows: gg_reduce_rows folds them into up to GG_REDUCE_SLICES rows written behind them
static inline int64_t attn_dbias_scratch_rows(int64_t part_rows) { return part_rows + GG_REDUCE_SLICES; }
static inline int64_t attn_dbias_part_rows(const GgAttnRoute& r) { return r.dbias_rows - GG_REDUCE_SLICES; }

// Second stage of every bias gradient: the partial rows (one per workgroup that binned dS) folded and summed in fp64 in a fixed order, then added to dbias.
static __global__ void attn_dbias_final_kernel(const float* __restrict__ rows, int nrows, int W, float* __restrict__ dbias) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W) return;
    double s = 0.0;
    for (int r = 0; r < nrows; ++r) s += (double)rows[(int64_t)r * W + i];
    dbias[i] += (float)s;
}
static inline void attn_dbias_reduce(float* dbias, float* part, int part_rows, int Wd, hipStream_t s) {
    if (!dbias || !part) return;
    const float* rows; int nrows;
    gg_reduce_rows(part, part_rows, Wd, s, &rows, &nrows);
    hipLaunchKernelGGL(attn_dbias_final_kernel, dim3((unsigned)gg_cdiv(Wd, 256)), dim3(256), 0, s, rows, nrows, Wd, dbias);
}

// What every windowed entry asks of its geometry with one text.  positive_map: the flash16 entries also refuse an empty map under the divisibility text.
static inline int attn_check_windows(const GgAttnArgs* a, bool positive_map, const char* who) {
    GG_CHECK(a->window_size * a->window_size == a->tokens_per_window, "%s: window_size^2 != tokens_per_window", who);
    GG_CHECK((!positive_map || (a->map_h > 0 && a->map_w > 0)) && a->map_h % a->window_size == 0 && a->map_w % a->window_size == 0, "%s: map not divisible by window", who);
    GG_CHECK(a->num_windows % ((a->map_h / a->window_size) * (a->map_w / a->window_size)) == 0, "%s: window count", who);
    return 0;
}
// The 20-bit reciprocals the kernels divide by (t / ws for t < span, t / (2 ws - 1) inside the signed-offset bias table), verified over their whole range.
static inline int attn_window_reciprocals(int ws, int span, uint32_t& rcp_ws, uint32_t& rcp_w2, const char* who) {
    const int w2 = 2 * ws - 1;
    rcp_ws = (uint32_t)(((1u << 20) + ws - 1) / ws);
    rcp_w2 = (uint32_t)(((1u << 20) + w2 - 1) / w2);
    for (int t = 0; t < span; ++t) GG_CHECK((int)(((uint32_t)t * rcp_ws) >> 20) == t / ws, "%s: reciprocal division fails at %d / %d", who, t, ws);
    for (int t = 0; t < w2 * w2; ++t) GG_CHECK((int)(((uint32_t)t * rcp_w2) >> 20) == t / w2, "%s: reciprocal division fails at %d / %d", who, t, w2);
    return 0;
}
