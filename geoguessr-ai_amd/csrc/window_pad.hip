// Padded attention windows of TinyViT (include/gg_pad.h): zero-pad a [B, H, W, C] map to [B, Hp, Wp, C] and crop a padded map back with the block's
// residual add.  Both kernels are pure data movement in 16-byte accesses (one thread per 16-byte piece of a pixel's channel vector): bandwidth-bound, no LDS.
#include "common.h"
#include "../../include/gg.h"
#include "../../include/gg_pad.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// cpr = 16-byte pieces per pixel; n = B * Hp * Wp * cpr pieces of y, all of them written
__global__ __launch_bounds__(256) void window_pad_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int H, int W, int Hp, int Wp, int cpr, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % cpr);
    const int64_t pix = idx / cpr;
    const int j = (int)(pix % Wp), i = (int)((pix / Wp) % Hp);
    const int64_t b = pix / ((int64_t)Wp * Hp);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (i < H && j < W) v = x[((b * H + i) * W + j) * cpr + c];
    y[idx] = v;
}

__device__ __forceinline__ float crop_add_one(float t, float r, float s, bool has_res, bool has_scale) {
    if (has_scale) t = __fmul_rn(s, t);         // (separate roundings: the product is not contracted into the sum)
    return has_res ? __fadd_rn(r, t) : t;
}
// n = B * H * W * cpr pieces of y; t is read at the padded pitch.  res and y may be the same buffer: a thread reads its piece of res before it writes that piece of y.
template <bool F32>
__global__ __launch_bounds__(256) void window_crop_add_kernel(const u32x4* __restrict__ t, const u32x4* res, const float* __restrict__ rowscale, u32x4* y,
                                                              int H, int W, int Hp, int Wp, int cpr, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % cpr);
    const int64_t pix = idx / cpr;
    const int j = (int)(pix % W), i = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    const u32x4 tv = t[((b * Hp + i) * Wp + j) * cpr + c];
    const bool has_res = res != nullptr, has_scale = rowscale != nullptr;
    const float s = has_scale ? rowscale[b] : 1.0f;
    u32x4 rv = {0u, 0u, 0u, 0u};
    if (has_res) rv = res[idx];
    u32x4 out;
    if (F32) {
        const f32x4 tf = __builtin_bit_cast(f32x4, tv), rf = __builtin_bit_cast(f32x4, rv);
        f32x4 o;
        for (int k = 0; k < 4; ++k) o[k] = crop_add_one(tf[k], rf[k], s, has_res, has_scale);
        out = __builtin_bit_cast(u32x4, o);
    } else {
        const bf16x8 tb = __builtin_bit_cast(bf16x8, tv), rb = __builtin_bit_cast(bf16x8, rv);
        bf16x8 o;
        for (int k = 0; k < 8; ++k) o[k] = (bf16)crop_add_one((float)tb[k], (float)rb[k], s, has_res, has_scale);
        out = __builtin_bit_cast(u32x4, o);
    }
    y[idx] = out;
}

static int pad_shape_check(const char* who, int B, int H, int W, int Hp, int Wp, int C, int dtype, int64_t pieces) {
    GG_CHECK(dtype == 0 || dtype == 1, "%s: dtype must be 0 (bf16) or 1 (f32)", who);
    GG_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && H <= Hp && W <= Wp, "%s: bad shape (B %d, map %d x %d, padded %d x %d, C %d)", who, B, H, W, Hp, Wp, C);
    GG_CHECK(((int64_t)C * (dtype == 1 ? 4 : 2)) % 16 == 0, "%s: C = %d is not a whole number of 16-byte pieces", who, C);
    GG_CHECK(gg_cdiv(pieces, 256) < ((int64_t)1 << 31), "%s: too many elements for one launch", who);
    return 0;
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int gg_window_pad(const void* x, void* y, int B, int H, int W, int Hp, int Wp, int C, int dtype, void* stream) {
    GG_CHECK(x && y, "gg_window_pad: null pointer");
    const int es = dtype == 1 ? 4 : 2;
    const int cpr = C * es / 16;
    const int64_t n = (int64_t)B * Hp * Wp * cpr;
    GG_TRY(pad_shape_check("gg_window_pad", B, H, W, Hp, Wp, C, dtype, n));
    GG_CHECK(aligned16(x) && aligned16(y), "gg_window_pad: pointers must be 16-byte aligned");
    GG_PROF(GG_CAT_PAD, 0, 16.0 * ((double)B * H * W * cpr + (double)n), stream);
    hipLaunchKernelGGL(window_pad_kernel, dim3((unsigned)gg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)x, (u32x4*)y, H, W, Hp, Wp, cpr, n);
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int gg_window_crop_add(const void* t, const void* res, const float* rowscale, void* y, int B, int H, int W, int Hp, int Wp, int C, int dtype, void* stream) {
    GG_CHECK(t && y, "gg_window_crop_add: null pointer");
    const int es = dtype == 1 ? 4 : 2;
    const int cpr = C * es / 16;
    const int64_t n = (int64_t)B * H * W * cpr;
    GG_TRY(pad_shape_check("gg_window_crop_add", B, H, W, Hp, Wp, C, dtype, n));
    GG_CHECK(aligned16(t) && aligned16(res) && aligned16(y) && ((uintptr_t)rowscale & 3) == 0, "gg_window_crop_add: pointers must be 16-byte aligned");
    GG_PROF(GG_CAT_PAD, 0, 16.0 * (double)n * (res ? 3 : 2), stream);
    if (dtype == 1)
        hipLaunchKernelGGL(window_crop_add_kernel<true>, dim3((unsigned)gg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)t, (const u32x4*)res, rowscale,
                           (u32x4*)y, H, W, Hp, Wp, cpr, n);
    else
        hipLaunchKernelGGL(window_crop_add_kernel<false>, dim3((unsigned)gg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)t, (const u32x4*)res, rowscale,
                           (u32x4*)y, H, W, Hp, Wp, cpr, n);
    GG_LAUNCH_CHECK();
    return 0;
}
