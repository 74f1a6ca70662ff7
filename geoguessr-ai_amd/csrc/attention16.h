// What the 16-bit-MFMA attention kernels share (attention_flash16.hip: the forward; attention_flash16_bwd.hip: the backward): the MFMA of a storage type, the
// 16-byte global load of 8-byte-aligned rows, and the two LDS placements of a 64-row image -- one for row reads (ds_read_b128), one for transposed reads
// (ds_read_b64_tr_b16).  The header comment of attention_flash16.hip derives the swizzles.
#pragma once
#include "common.h"

namespace {

typedef short a16_s4 __attribute__((ext_vector_type(4)));
typedef unsigned int a16_u4 __attribute__((ext_vector_type(4)));
typedef unsigned int a16_u2 __attribute__((ext_vector_type(2)));
typedef int a16_i4 __attribute__((ext_vector_type(4)));

template <typename T> struct A16Op;
template <> struct A16Op<f16> {
    typedef f16x8 v8; typedef f16x4 v4;
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct A16Op<bf16> {
    typedef bf16x8 v8; typedef bf16x4 v4;
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// 8 consecutive 16-bit elements.  Rows are 8-byte aligned by contract, so the source states two 8-byte loads; on gfx950 they compile to one 16-byte load
__device__ __forceinline__ a16_u4 a16_ld8(const void* p) {
    const a16_u2 a = reinterpret_cast<const a16_u2*>(p)[0], b = reinterpret_cast<const a16_u2*>(p)[1];
    return (a16_u4){a[0], a[1], b[0], b[1]};
}

// The images of one head dim: 64 rows of 2 D bytes, and where 16-byte chunk ch of row `row` is stored: koff for an image read by rows (the forward's K), voff
// for an image read transposed (the forward's V)
template <int D> struct A16Lds {
    static constexpr int ROW = 2 * D, TILE = 64 * ROW;          // bytes of a row; of one image
    static constexpr int CPR = D / 8, NST = D / 32;             // 16-byte chunks per row; staged chunks of each image per thread (256 threads, 64 rows)
    static __device__ __forceinline__ constexpr int kswz(int row) {            // K chunk swizzle
        if (D == 64) return (row >> 1) & 7;
        const int g = (row >> 2) & 3;
        return g ^ ((g & 1) << 1);
    }
    static __device__ __forceinline__ constexpr int vswz(int row) { return D == 64 ? (row >> 1) & 3 : (row >> 2) & 1; }          // V 32-byte block swizzle
    static __device__ __forceinline__ constexpr int koff(int row, int ch) { return row * ROW + ((ch ^ kswz(row)) << 4); }
    static __device__ __forceinline__ constexpr int voff(int row, int ch) { return row * ROW + (((ch >> 1) ^ vswz(row)) << 5) + ((ch & 1) << 4); }
};

constexpr int A16_EMAX = 63 * 63;            // floats of the expanded (signed-offset) bias table at ws = 32
// t / d by the reciprocal rcp = ceil(2^20 / d): exact for every index the kernels form (checked on the host)
__device__ __forceinline__ int a16_div(int t, uint32_t rcp) { return (int)(((uint32_t)t * rcp) >> 20); }

}  // namespace
