// Per-pixel and per-table arithmetic of the training transform (include/gg_aug.h), as functions that compile for the device and for the host alike: the kernels of
// augment.hip call them per element, and a plain C++ program can run the very same statements on a CPU.  Every function that restates Pillow's float / double
// arithmetic switches fused multiply-adds off: a contracted a * b + c rounds once where Pillow rounds twice, which changes bytes.
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/gg_aug.h"
#if defined(__HIPCC__)
#define GG_HD __host__ __device__ inline
#else
#define GG_HD inline
#endif

GG_HD bool aug_is_affine(int op) { return op == GG_AUG_ROTATE || (op >= GG_AUG_SHEAR_X && op <= GG_AUG_TRANSLATE_Y); }
GG_HD bool aug_is_blend(int op) { return op >= GG_AUG_COLOR && op <= GG_AUG_SHARPNESS; }
GG_HD bool aug_is_table(int op) { return op == GG_AUG_AUTO_CONTRAST || op == GG_AUG_EQUALIZE || op == GG_AUG_INVERT || (op >= GG_AUG_POSTERIZE && op <= GG_AUG_SOLARIZE_ADD); }
GG_HD bool aug_needs_hist(int op) { return op == GG_AUG_AUTO_CONTRAST || op == GG_AUG_EQUALIZE; }
GG_HD bool aug_needs_stats(int op) { return aug_needs_hist(op) || op == GG_AUG_CONTRAST; }

GG_HD int aug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
GG_HD unsigned char aug_grey(int r, int g, int b) { return (unsigned char)((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16); }

// Invert / Posterize / Solarize / SolarizeAdd: entry i of the table
GG_HD unsigned char aug_static_lut(int op, int iarg, int i) {
    if (op == GG_AUG_INVERT) return (unsigned char)(255 - i);
    if (op == GG_AUG_POSTERIZE) return (unsigned char)(iarg >= 8 ? i : (i & ~((1 << (8 - (iarg < 0 ? 0 : iarg))) - 1) & 255));
    if (op == GG_AUG_SOLARIZE) return (unsigned char)(i < iarg ? i : 255 - i);
    /* GG_AUG_SOLARIZE_ADD */ return (unsigned char)(i < 128 ? (i + iarg > 255 ? 255 : (i + iarg < 0 ? 0 : i + iarg)) : i);
}
// ImageOps.autocontrast(cutoff = 0) of one channel: h its 256-bin histogram
GG_HD void aug_autocontrast_lut(const unsigned* h, unsigned char* lut) {
#pragma clang fp contract(off)
    int lo = 0, hi = 255;
    while (lo < 256 && !h[lo]) ++lo;
    while (hi >= 0 && !h[hi]) --hi;
    if (hi <= lo) { for (int i = 0; i < 256; ++i) lut[i] = (unsigned char)i; return; }
    const double scale = 255.0 / (hi - lo);
    const double offset = -lo * scale;
    for (int i = 0; i < 256; ++i) {
        const double v = i * scale + offset;
        lut[i] = (unsigned char)(v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v));
    }
}
// ImageOps.equalize of one channel
GG_HD void aug_equalize_lut(const unsigned* h, unsigned char* lut) {
    int64_t sum = 0, last = 0;
    int occupied = 0;
    for (int i = 0; i < 256; ++i) if (h[i]) { sum += h[i]; last = h[i]; ++occupied; }
    const int64_t step = (sum - last) / 255;
    if (occupied <= 1 || step == 0) { for (int i = 0; i < 256; ++i) lut[i] = (unsigned char)i; return; }
    int64_t n = step / 2;
    for (int i = 0; i < 256; ++i) {
        const int64_t v = n / step;
        lut[i] = (unsigned char)(v > 255 ? 255 : v);           // past the last occupied bin no pixel reads the entry
        n += h[i];
    }
}
// Image.blend(degenerate, image, f) on one byte
GG_HD unsigned char aug_blend(unsigned char d, unsigned char x, float f) {
#pragma clang fp contract(off)
    const float prod = f * ((float)x - (float)d);
    const float t = (float)d + prod;
    if (f >= 0.0f && f <= 1.0f) return (unsigned char)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (unsigned char)t);
}
// ImageFilter.SMOOTH at an interior pixel: img is S x S x 3, c the channel
GG_HD unsigned char aug_smooth(const unsigned char* img, int S, int y, int x, int c) {
#pragma clang fp contract(off)
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    float ss = 0.5f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const float prod = (float)img[((int64_t)(y + dy) * S + (x + dx)) * 3 + c] * ((dy == 0 && dx == 0) ? k5 : k1);
            ss = ss + prod;
        }
    return ss <= 0.0f ? 0 : (ss >= 255.0f ? 255 : (unsigned char)ss);
}
GG_HD double aug_cubic(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    const double a = d * p4;
    const double b = d * (p3 + a);
    const double c = d * (p2 + b);
    return p1 + c;
}
GG_HD unsigned char aug_clip8d(double v) { return v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (unsigned char)(int)v); }
// Image.transform(size, AFFINE, m, resample, fillcolor) at output pixel (x, y): img is S x S x 3; out gets the three bytes
GG_HD void aug_affine(const unsigned char* img, int S, const double* m, int resample, const unsigned char* fill, int x, int y, unsigned char* out) {
#pragma clang fp contract(off)
    const double xc = x + 0.5, yc = y + 0.5;
    const double t0 = m[0] * xc, t1 = m[1] * yc, t3 = m[3] * xc, t4 = m[4] * yc;
    double xin = (t0 + t1) + m[2];
    double yin = (t3 + t4) + m[5];
    if (!(xin >= 0.0 && xin < (double)S && yin >= 0.0 && yin < (double)S)) { out[0] = fill[0]; out[1] = fill[1]; out[2] = fill[2]; return; }
    xin -= 0.5; yin -= 0.5;
    const int xi = (int)floor(xin), yi = (int)floor(yin);
    const double dx = xin - xi, dy = yin - yi;
    if (resample == 2) {
        const int x0 = aug_clampi(xi, 0, S - 1) * 3, x1 = aug_clampi(xi + 1, 0, S - 1) * 3;
        const unsigned char* r0 = img + (int64_t)aug_clampi(yi, 0, S - 1) * S * 3;
        const bool has1 = yi + 1 >= 0 && yi + 1 < S;
        const unsigned char* r1 = img + (int64_t)aug_clampi(yi + 1, 0, S - 1) * S * 3;
        for (int c = 0; c < 3; ++c) {
            const double a0 = r0[x0 + c], b0 = r0[x1 + c];
            const double e0 = (b0 - a0) * dx;
            const double v1 = a0 + e0;
            double v2 = v1;
            if (has1) { const double a1 = r1[x0 + c], b1 = r1[x1 + c]; const double e1 = (b1 - a1) * dx; v2 = a1 + e1; }
            const double e2 = (v2 - v1) * dy;
            out[c] = aug_clip8d(v1 + e2);
        }
    } else {
        int xo[4];
        for (int j = 0; j < 4; ++j) xo[j] = aug_clampi(xi - 1 + j, 0, S - 1) * 3;
        for (int c = 0; c < 3; ++c) {
            double v[4];
            for (int j = 0; j < 4; ++j) {
                const int yy = yi - 1 + j;
                if (j == 0 || (yy >= 0 && yy < S)) {
                    const unsigned char* r = img + (int64_t)aug_clampi(yy, 0, S - 1) * S * 3 + c;
                    v[j] = aug_cubic(r[xo[0]], r[xo[1]], r[xo[2]], r[xo[3]], dx);
                } else {
                    v[j] = v[j - 1];
                }
            }
            out[c] = aug_clip8d(aug_cubic(v[0], v[1], v[2], v[3], dy));
        }
    }
}
