// Pillow's 8-bit-per-channel resampling taps (ImagingResample, BILINEAR), the one copy shared by the two-launch reduction of
// crappify.hip (pssr_bilinear_down_u8), the fused reduction + moments of consistency.hip (pssr_reduce_moments_u8) and the shift search of
// register.hip (pssr_register_shifts_u8); the last two take it through u8_planes.h, which holds the steps they share beyond the taps.
#pragma once
#include "common.h"

constexpr int PRECISION_BITS = 32 - 8 - 2;   // Pillow ImagingResample 8bpc fixed point

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for one output index (bilinear = triangle filter).
// Evaluated in double in Pillow's operation order, so the integer taps are the ones Pillow uses.
struct Taps { int xmin, n; int k[40]; };
__device__ __forceinline__ void pil_taps(int xx, int in_size, int out_size, Taps& t) {
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    double w[40];
    double ww = 0.0;
    for (int x = 0; x < n && x < 40; ++x) {
        double a = (x + xmin - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        const double v = a < 1.0 ? 1.0 - a : 0.0;
        w[x] = v; ww += v;
    }
    t.xmin = xmin; t.n = n < 40 ? n : 40;
    for (int x = 0; x < t.n; ++x) {
        const double v = ww != 0.0 ? w[x] / ww : w[x];
        t.k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
    }
}
// The same for Pillow's other filters and any in_size -> out_size (the enlargement of baseline.hip): BILINEAR (triangle, support 1) and
// BICUBIC (Keys, a = -0.5, support 2).  At most MAXN taps are kept (enlarging: ceil(support) * 2 + 1 = 3 or 5).  No contraction: a fused
// multiply-add would round the cubic differently from Pillow's compiled C.
enum PilFilter { PIL_BILINEAR = 0, PIL_BICUBIC = 1 };
template <int FILTER> struct PilFilterOf;
template <> struct PilFilterOf<PIL_BILINEAR> {
    static constexpr double SUPPORT = 1.0;
    static __device__ __forceinline__ double f(double a) {
        if (a < 0.0) a = -a;
        return a < 1.0 ? 1.0 - a : 0.0;
    }
};
template <> struct PilFilterOf<PIL_BICUBIC> {
    static constexpr double SUPPORT = 2.0;
    static __device__ __forceinline__ double f(double a) {
#pragma clang fp contract(off)
        constexpr double A = -0.5;
        if (a < 0.0) a = -a;
        if (a < 1.0) return ((A + 2.0) * a - (A + 3.0)) * a * a + 1;
        if (a < 2.0) return (((a - 5) * a + 8) * a - 4) * A;
        return 0.0;
    }
};
template <int FILTER, int MAXN>
__device__ __forceinline__ void pil_taps_f(int xx, int in_size, int out_size, int& t_xmin, int& t_n, int* t_k) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = PilFilterOf<FILTER>::SUPPORT * filterscale;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    int n = xmax - xmin;
    if (n > MAXN) n = MAXN;
    double w[MAXN];
    double ww = 0.0;
#pragma unroll
    for (int x = 0; x < MAXN; ++x) {
        const double v = x < n ? PilFilterOf<FILTER>::f((x + xmin - center + 0.5) * ss) : 0.0;
        w[x] = v;
        if (x < n) ww += v;
    }
    t_xmin = xmin; t_n = n;
#pragma unroll
    for (int x = 0; x < MAXN; ++x) {
        const double v = ww != 0.0 ? w[x] / ww : w[x];
        t_k[x] = x < n ? (v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS))) : 0;
    }
}
__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
