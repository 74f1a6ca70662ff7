// Position-table resampling of the CLIP vision tower at a foreign input size (include/gg_clip_interp.h): transformers'
// CLIPVisionEmbeddings.interpolate_pos_encoding -- torch's bicubic F.interpolate (A = -0.75, align_corners = False, border-clamped taps, no antialiasing) of the
// (Gs, Gs, D) patch grid to (Gh, Gw, D), the class row kept -- and its adjoint.  Both are gathers: the forward's lane owns 4 channels of one destination row and
// reads its 16 taps; the backward's workgroup owns one SOURCE row and walks the destination rows that read it, so no atomics and a fixed summation order.
// The source coordinate and the cubic weights are formed in f64 and rounded to f32 once; the tap sums accumulate in f64 and are rounded to f32 once, on store
// (a few dozen f64 operations per lane next to its row loads: both kernels are bound by those).
#include <algorithm>
#include "common.h"
#include "../../include/gg_clip_interp.h"

namespace {
// the four taps of destination index o along one axis (Gout destinations over Gs sources): clamped source indices and Keys' weights (A = -0.75)
__device__ __forceinline__ void cubic_taps(int o, int Gout, int Gs, int (&idx)[4], float (&w)[4]) {
    const double A = -0.75;
    const double s = ((double)o + 0.5) * (double)Gs / (double)Gout - 0.5;
    const double fl = floor(s);
    const double t = s - fl;
    const int i0 = (int)fl;
    double x = t + 1.0;
    w[0] = (float)(((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A);
    x = t;
    w[1] = (float)(((A + 2.0) * x - (A + 3.0)) * x * x + 1.0);
    x = 1.0 - t;
    w[2] = (float)(((A + 2.0) * x - (A + 3.0)) * x * x + 1.0);
    x = 2.0 - t;
    w[3] = (float)(((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A);
#pragma unroll
    for (int a = 0; a < 4; ++a) idx[a] = min(max(i0 - 1 + a, 0), Gs - 1);
}

typedef double f64x4 __attribute__((ext_vector_type(4)));
// c + a * w in f64 (the product of two f32 is exact there)
__device__ __forceinline__ f64x4 mad4(f32x4 a, float w, f64x4 c) { return c + __builtin_convertvector(a, f64x4) * (double)w; }
__device__ __forceinline__ f64x4 mad4(f64x4 a, float w, f64x4 c) { return c + a * (double)w; }

// out[0,:] = pos[0,:]; out[1 + oy Gw + ox,:] = sum_a wy[a] (sum_b wx[b] pos[1 + iy[a] Gs + ix[b],:]); a lane owns 4 consecutive channels (D % 4 == 0)
__global__ __launch_bounds__(256) void pos_interp_fwd_kernel(const float* __restrict__ pos, int Gs, int Gh, int Gw, int D, float* __restrict__ out) {
    const int D4 = D / 4;
    const int64_t total = (int64_t)(Gh * Gw + 1) * D4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int dd = (int)(i % D4) * 4;
        const int t = (int)(i / D4);
        f32x4 v;
        if (t == 0) v = *reinterpret_cast<const f32x4*>(pos + dd);
        else {
            const int oy = (t - 1) / Gw, ox = (t - 1) - oy * Gw;
            int iy[4], ix[4];
            float wy[4], wx[4];
            cubic_taps(oy, Gh, Gs, iy, wy);
            cubic_taps(ox, Gw, Gs, ix, wx);
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float* row = pos + ((int64_t)1 + (int64_t)iy[a] * Gs) * D + dd;
                f64x4 r = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int b = 0; b < 4; ++b) r = mad4(*reinterpret_cast<const f32x4*>(row + (int64_t)ix[b] * D), wx[b], r);
                acc = mad4(r, wy[a], acc);
            }
            v = __builtin_convertvector(acc, f32x4);
        }
        *reinterpret_cast<f32x4*>(out + (int64_t)t * D + dd) = v;
    }
}

// d_pos[r,:] += sum_oy wyT[oy] (sum_ox wxT[ox] d_out[1 + oy Gw + ox,:]) for the source row r = 1 + sy Gs + sx of this workgroup (row 0: d_pos[0,:] += d_out[0,:]).
// wyT[oy]: the weight destination row oy gives source row sy (clamped taps that land on the same border row add up), 0 where it reads none -- formed once per
// workgroup in LDS; a zero weight skips its row / column for every lane alike (workgroup-uniform).
__global__ __launch_bounds__(256) void pos_interp_bwd_kernel(const float* __restrict__ d_out, int Gs, int Gh, int Gw, int D, float* __restrict__ d_pos) {
    __shared__ float wT[2][GG_CLIP_INTERP_MAX_SIDE];
    const int r = blockIdx.x, D4 = D / 4;
    if (r == 0) {
        for (int c4 = threadIdx.x; c4 < D4; c4 += blockDim.x) {
            f32x4* dst = reinterpret_cast<f32x4*>(d_pos + 4 * c4);
            *dst = *dst + *reinterpret_cast<const f32x4*>(d_out + 4 * c4);
        }
        return;
    }
    const int sy = (r - 1) / Gs, sx = (r - 1) - sy * Gs;
    {
        const int axis = threadIdx.x >> 6, o = threadIdx.x & 63;      // wave 0: rows, wave 1: columns
        if (axis < 2 && o < (axis == 0 ? Gh : Gw)) {
            int idx[4];
            float w[4];
            cubic_taps(o, axis == 0 ? Gh : Gw, Gs, idx, w);
            const int mine = axis == 0 ? sy : sx;
            float s = 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a) if (idx[a] == mine) s += w[a];
            wT[axis][o] = s;
        }
    }
    __syncthreads();
    for (int c4 = threadIdx.x; c4 < D4; c4 += blockDim.x) {
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int oy = 0; oy < Gh; ++oy) {
            const float wy = wT[0][oy];
            if (wy == 0.f) continue;
            f64x4 racc = {0.0, 0.0, 0.0, 0.0};
            const float* row = d_out + ((int64_t)1 + (int64_t)oy * Gw) * D + 4 * c4;
            for (int ox = 0; ox < Gw; ++ox) {
                const float wx = wT[1][ox];
                if (wx == 0.f) continue;
                racc = mad4(*reinterpret_cast<const f32x4*>(row + (int64_t)ox * D), wx, racc);
            }
            acc = mad4(racc, wy, acc);
        }
        f32x4* dst = reinterpret_cast<f32x4*>(d_pos + (int64_t)r * D + 4 * c4);
        *dst = *dst + __builtin_convertvector(acc, f32x4);      // the sum is rounded to f32 once, then added: d_pos + (the result into zeros), bit for bit
    }
}

static int check_args(const char* who, const void* a, const void* b, int Gs, int Gh, int Gw, int D) {
    GG_CHECK(a && b, "%s: null pointer", who);
    GG_CHECK(D >= 4 && (D & 3) == 0, "%s: D must be a positive multiple of 4 (a lane owns 4 consecutive channels), got %d", who, D);
    GG_CHECK(Gs >= 1 && Gh >= 1 && Gw >= 1, "%s: a grid side below 1 (source %d, destination %d x %d)", who, Gs, Gh, Gw);
    GG_CHECK(Gs <= GG_CLIP_INTERP_MAX_SIDE && Gh <= GG_CLIP_INTERP_MAX_SIDE && Gw <= GG_CLIP_INTERP_MAX_SIDE,
             "%s: a grid side above the cap of %d (source %d, destination %d x %d)", who, GG_CLIP_INTERP_MAX_SIDE, Gs, Gh, Gw);
    GG_CHECK(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0, "%s: pointers must be 16-byte aligned", who);
    return 0;
}
}  // namespace

extern "C" int gg_clip_pos_interp_fwd(const float* pos, int Gs, int Gh, int Gw, int D, float* out, void* stream) {
    GG_TRY(check_args("gg_clip_pos_interp_fwd", pos, out, Gs, Gh, Gw, D));
    const int64_t n = (int64_t)(Gh * Gw + 1) * D;
    GG_PROF(GG_CAT_MOVE, 0, 8.0 * n, stream);
    if (Gs == Gh && Gs == Gw) {      // the native grid: the input bits
        GG_HIP(hipMemcpyAsync(out, pos, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return 0;
    }
    const unsigned grid = (unsigned)std::min<int64_t>((n / 4 + 255) / 256, 32768);
    hipLaunchKernelGGL(pos_interp_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pos, Gs, Gh, Gw, D, out);
    GG_LAUNCH_CHECK();
    return 0;
}

extern "C" int gg_clip_pos_interp_bwd(const float* d_out, int Gs, int Gh, int Gw, int D, float* d_pos, void* stream) {
    GG_TRY(check_args("gg_clip_pos_interp_bwd", d_out, d_pos, Gs, Gh, Gw, D));
    GG_PROF(GG_CAT_MOVE, 0, 4.0 * ((int64_t)(Gh * Gw + 1) + 2 * (int64_t)(Gs * Gs + 1)) * D, stream);
    hipLaunchKernelGGL(pos_interp_bwd_kernel, dim3((unsigned)(Gs * Gs + 1)), dim3(256), 0, (hipStream_t)stream, d_out, Gs, Gh, Gw, D, d_pos);
    GG_LAUNCH_CHECK();
    return 0;
}
