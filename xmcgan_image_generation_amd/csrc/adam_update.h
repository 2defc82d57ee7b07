// The arithmetic of the Adam (+ EMA) update and of the gradient through sigma: the ONE definition that adam_kernel (pointwise.hip:
// float4 loop, scalar tail) and adam_wprep_kernel (spectral_batched.hip: tile loop) call.
//
// Every rounding is fixed here, in source: contraction is switched off inside these functions and each fused multiply-add is
// written out.  Written as `b1 * m + (1 - b1) * gr` under -ffp-contract=fast, which of the two products is rounded on its own is
// the compiler's choice, made per copy of the expression; tests/test_gpu_fused_opt.py and tests/test_gpu_nonfinite_guard.py
// require the flat kernel, the tile kernel and their guarded forms to agree bit for bit, and tests/test_gpu_adam_bits.py holds
// every entry point to recorded bits (tests/golden/adam_parent_bits.npz).
#pragma once
#include "common.h"

struct AdamHyper {
    float lr, b1, b2, eps;
    float ic1, ic2;      // 1 / (1 - beta^t): the bias corrections
    float gs;            // gradient scale
    float d;             // EMA decay
};

// gr = gs g;  m = b1 m + (1 - b1) gr;  v = b2 v + (1 - b2) gr^2;  p -= lr (m ic1) / (sqrt(v ic2) + eps)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamHyper& h) {
#pragma clang fp contract(off)
    const float gr = g * h.gs;
    m = __builtin_fmaf(h.b1, m, (1.f - h.b1) * gr);
    v = __builtin_fmaf(gr, (1.f - h.b2) * gr, h.b2 * v);
    p -= h.lr * (m * h.ic1) / (sqrtf(v * h.ic2) + h.eps);
}

// ema = d ema + (1 - d) p
__device__ __forceinline__ float ema_mix(float ema, float p, float d) {
#pragma clang fp contract(off)
    return __builtin_fmaf(d, ema, (1.f - d) * p);
}

__device__ __forceinline__ void adam_update4(float4& p, const float4& g, float4& m, float4& v, const AdamHyper& h) {
    adam_update(p.x, g.x, m.x, v.x, h);
    adam_update(p.y, g.y, m.y, v.y, h);
    adam_update(p.z, g.z, m.z, v.z, h);
    adam_update(p.w, g.w, m.w, v.w, h);
}

__device__ __forceinline__ void ema_mix4(float4& ema, const float4& p, float d) {
    ema.x = ema_mix(ema.x, p.x, d);
    ema.y = ema_mix(ema.y, p.y, d);
    ema.z = ema_mix(ema.z, p.z, d);
    ema.w = ema_mix(ema.w, p.w, d);
}

// The gradient through sigma of a spectrally-normalised weight (xmcgan/libml/layers.py:217-219 of the reference):
// g' = (g - k a b) / (sigma + eps), k = <G, W> / (sigma + eps), a b = u_r v_c; is = 1 / (sigma + eps).
// Row form: four consecutive elements of one row share a; ak = sigma_row_factor(a, k) once per row.
__device__ __forceinline__ float sigma_row_factor(float a, float k) {
#pragma clang fp contract(off)
    return a * k;
}
__device__ __forceinline__ void sigma_term4(float4& g, float ak, const float4& b, float is) {
#pragma clang fp contract(off)
    g.x = __builtin_fmaf(-ak, b.x, g.x) * is;
    g.y = __builtin_fmaf(-ak, b.y, g.y) * is;
    g.z = __builtin_fmaf(-ak, b.z, g.z) * is;
    g.w = __builtin_fmaf(-ak, b.w, g.w) * is;
}
// Scalar form (a float4 that straddles rows)
__device__ __forceinline__ float sigma_term(float g, float k, float a, float b, float is) {
#pragma clang fp contract(off)
    return __builtin_fmaf(-k, a * b, g) * is;
}

// What becomes of the consumed gradient.  zero_g == 1: overwritten with zeros (the next half step accumulates into a clean
// arena without a separate fill); zero_g == 2: the FINAL gradient of a tensor with a sigma term is written back (tests, tools);
// zero_g == 0: left as it is.
__device__ __forceinline__ void store_consumed_grad(float4* g, const float4& final_g, int zero_g, bool has_sigma_term) {
    if (zero_g == 1) *g = make_float4(0.f, 0.f, 0.f, 0.f);
    else if (zero_g == 2 && has_sigma_term) *g = final_g;
}
