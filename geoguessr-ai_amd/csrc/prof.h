// RAII HIP-event bracket around a kernel launch (active only after gg_prof_enable(1)).
#pragma once
void gg_set_error(const char* fmt, ...);
enum { GG_CAT_GEMM = 0, GG_CAT_ATTN = 1, GG_CAT_DWCONV = 2, GG_CAT_NORM = 3, GG_CAT_HEAD = 4, GG_CAT_OPTIM = 5, GG_CAT_MOVE = 6, GG_CAT_PAD = 7 /* gg_window_pad / gg_window_crop_add (include/gg_pad.h) */,
       GG_CAT_ATTN_DBIAS = 8 /* gg_attention_dbias (include/gg_attn_dbias.h) */, GG_NUM_CATS = 9,
       GG_CAT_SPLIT_FLAG = 16 };      // or-ed into GG_CAT_GEMM by the split-bf16 GEMMs: bench.py prices them against the bf16 matrix peak / 6 (category = value & 15)
struct GgProfScope {
    GgProfScope(int cat, double flops, double bytes, void* stream);
    ~GgProfScope();
    int idx_; void* stream_;
};
#define GG_PROF(cat, flops, bytes, stream) GgProfScope gg_prof_scope_((cat), (double)(flops), (double)(bytes), (stream))
// Row compaction (kernels whose live extent is a device-side count): the count the roofline should price a launch by -- `full` unless the profiling hooks are
// on and the stream is not capturing; then the device value, read back with a blocking copy behind the stream's earlier work.
int gg_prof_live_groups(const int* count_dev, int full, void* stream);
