// Pillow's BICUBIC resampling taps, shared by the forward preprocessing (clip.hip) and its transpose (clip_grad.hip): both
// kernels build the SAME float32 weights from this one function.
#pragma once
#include "common.h"

// Pillow's resampling coefficients (ImagingResample's precompute_coeffs with the bicubic filter, a = -0.5) for output index `o` of
// an `in` -> `out` resize: the window starts at *lo and holds the returned number of taps (<= ksize); w[k] = the normalised
// weights, computed in double as Pillow does and rounded to float32 once.
__device__ __forceinline__ double keys_cubic(double x) {
    x = fabs(x);
    if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;               // ((a + 2) x - (a + 3)) x^2 + 1
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;    // a (x^3 - 5 x^2 + 8 x - 4)
    return 0.0;
}

__device__ __forceinline__ int cubic_taps(int o, int in, int out, int ksize, float* w, int* lo) {
    const double scale = (double)in / (double)out;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fscale, ss = 1.0 / fscale;
    const double center = (o + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    int cnt = xmax - xmin;
    if (cnt > ksize) cnt = ksize;                                    // (never: ksize = 2 ceil(support) + 1; keeps the table's bounds local)
    double ww = 0.0;
    for (int k = 0; k < cnt; ++k) ww += keys_cubic((k + xmin - center + 0.5) * ss);
    const double inv = ww != 0.0 ? 1.0 / ww : 0.0;
    for (int k = 0; k < cnt; ++k) w[k] = (float)(keys_cubic((k + xmin - center + 0.5) * ss) * inv);
    *lo = xmin;
    return cnt;
}
