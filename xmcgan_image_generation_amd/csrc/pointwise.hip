// Streaming pointwise / resampling kernels (HBM-bound; 16-byte vectors, grid-stride) and the
// fused Adam(+EMA) arena update.
#include <cmath>

#include "adam_update.h"
#include "common.h"

namespace {

template <typename T, int VE> struct Acc {
    static __device__ __forceinline__ void load(const T* p, float* f) { Vec<T> v; v.load(p); v.get(f); }
    static __device__ __forceinline__ void store(T* p, const float* f) { Vec<T> v; v.set(f); v.store(p); }
};
template <typename T> struct Acc<T, 1> {
    static __device__ __forceinline__ void load(const T* p, float* f) { f[0] = to_f<T>(*p); }
    static __device__ __forceinline__ void store(T* p, const float* f) { *p = from_f<T>(f[0]); }
};

// y[n][oy][ox][c] = scale * sum_{2x2} x + res;  XR: also xr = max(x, 0) at full resolution -- the pass already holds every
// element of x in registers, and the discriminator block that pools its input for the shortcut (nets/common.py:74-78 of the
// reference) reads relu(x) in its first convolution AND in that convolution's weight gradient, where an in-LDS ReLU pass
// over the DMA-staged patch costs 20-28 % of the kernel (tools/relu_cost.py)
template <typename T, int VE, bool XR>
__global__ __launch_bounds__(256) void pool2_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                    T* __restrict__ y, T* __restrict__ xr, int H, int W, int C, float scale,
                                                    long long nvec) {
    const int CV = C / VE, Wo = W >> 1, Ho = H >> 1;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
        const long long opix = v / CV;
        const int c = (int)(v - opix * CV) * VE;
        const int ox = (int)(opix % Wo);
        const long long t = opix / Wo;
        const int oy = (int)(t % Ho);
        const long long n = t / Ho;
        const long long o00 = (((n * H + 2 * oy) * W) + 2 * ox) * C + c, o10 = o00 + (long long)W * C;
        float a[VE], b[VE], d[VE], e2[VE], s[VE];
        Acc<T, VE>::load(x + o00, a);
        Acc<T, VE>::load(x + o00 + C, b);
        Acc<T, VE>::load(x + o10, d);
        Acc<T, VE>::load(x + o10 + C, e2);
#pragma unroll
        for (int e = 0; e < VE; ++e) s[e] = ((a[e] + b[e]) + d[e] + e2[e]) * scale;
        if (res) {
            float r[VE];
            Acc<T, VE>::load(res + opix * C + c, r);
#pragma unroll
            for (int e = 0; e < VE; ++e) s[e] += r[e];
        }
        Acc<T, VE>::store(y + opix * C + c, s);
        if constexpr (XR) {
#pragma unroll
            for (int e = 0; e < VE; ++e) { a[e] = fmaxf(a[e], 0.f); b[e] = fmaxf(b[e], 0.f); d[e] = fmaxf(d[e], 0.f); e2[e] = fmaxf(e2[e], 0.f); }
            Acc<T, VE>::store(xr + o00, a);
            Acc<T, VE>::store(xr + o00 + C, b);
            Acc<T, VE>::store(xr + o10, d);
            Acc<T, VE>::store(xr + o10 + C, e2);
        }
    }
}

// out[n][y][x][tap * C + c] = in[n][y + s*dy(tap)][x + s*dx(tap)][c]  (0 outside the image, 0 for k >= taps*C),
// 32 output channels, C <= 3: turns a 3x3 (or 1x1) convolution on an RGB-like tensor into a 1x1 convolution
// on a 32-channel tensor, so it runs on the MFMA patch kernels instead of the scalar-gather path.
// s = +1 gathers the forward im2col; s = -1 gathers dy(p - d(tap)) for the weight gradient of a Cout = 3 conv.
// One thread writes Vec<T>::N consecutive k of one pixel (a 16-byte store: the 32-channel output is the traffic, the
// RGB-like input is cache-resident).
template <typename T>
__global__ __launch_bounds__(256) void expand_taps_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W,
                                                          int C, int ks, int sign, long long npix) {
    constexpr int V = Vec<T>::N, G = 32 / V;                       // vectors per pixel
    const int taps = ks * ks, half = ks >> 1, kmax = taps * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix * G; i += (long long)gridDim.x * 256) {
        const long long pix = i / G;
        const int k0 = (int)(i - pix * G) * V;
        const int px = (int)(pix % W);
        const long long t = pix / W;
        const int py = (int)(t % H);
        const long long n = t / H;
        float v[V];
        int tap = k0 / C, c = k0 - tap * C;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            // branch-free: an out-of-range element reads x[0] and is replaced by zero afterwards (a conditional load per
            // element compiled to V serial (branch, load, s_waitcnt vmcnt(0)) sequences: V exposed memory latencies)
            const int ty = tap / ks, tx = tap - ty * ks;
            const int iy = py + sign * (ty - half), ix = px + sign * (tx - half);
            const bool ok = k0 + e < kmax && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            const long long idx = ok ? ((n * H + iy) * W + ix) * C + c : 0;
            const float val = to_f<T>(x[idx]);
            v[e] = ok ? val : 0.f;
            if (++c == C) { c = 0; ++tap; }
        }
        Vec<T> o;
        o.set(v);
        o.store(y + pix * 32 + k0);
    }
}

// The 3x3 expansion of a 3-channel bf16 tensor, one workgroup per image row: the three input rows are staged in LDS with
// coalesced 16-byte loads (8 zero elements either side = the left / right padding, zero rows outside the image), every
// thread then assembles 16-byte output vectors from 2-byte LDS reads.  (The generic kernel: eight 2-byte global loads per
// vector, 50 us for 117 MB.)  W * 3 % 8 == 0, W <= 512, 16-byte aligned tensors.
constexpr int ET_W_MAX = 512, ET_ROW = 8 + ET_W_MAX * 3 + 8;
__global__ __launch_bounds__(256) void expand_taps3_rows_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int H, int W, int sign) {
    __shared__ __attribute__((aligned(16))) bf16_t rows[3][ET_ROW];
    const int py = blockIdx.x % H, n = blockIdx.x / H;
    const int nvec = (8 + W * 3 + 8) / 8, vvec = W * 3 / 8;
    for (int it = threadIdx.x; it < 3 * nvec; it += 256) {
        const int r = it / nvec, v = it - r * nvec;
        const int iy = py + sign * (r - 1);
        uint4 q = make_uint4(0, 0, 0, 0);
        if ((unsigned)iy < (unsigned)H && v >= 1 && v - 1 < vvec)
            q = *reinterpret_cast<const uint4*>(x + ((long long)n * H + iy) * W * 3 + (v - 1) * 8);
        *reinterpret_cast<uint4*>(&rows[r][v * 8]) = q;
    }
    __syncthreads();
    bf16_t* out = y + ((long long)n * H + py) * W * 32;
    for (int it = threadIdx.x; it < W * 4; it += 256) {
        const int px = it >> 2, k0 = (it & 3) * 8;
        unsigned short h[8];
        int tap = k0 / 3, c = k0 - tap * 3;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ty = tap / 3, tx = tap - ty * 3;
            h[e] = tap < 9 ? rows[ty][8 + (px + sign * (tx - 1)) * 3 + c] : (unsigned short)0;
            if (++c == 3) { c = 0; ++tap; }
        }
        *reinterpret_cast<uint4*>(out + (long long)px * 32 + k0) =
            make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bcast_relu_bwd_kernel(const float* __restrict__ dpool,
                                                             const T* __restrict__ x, T* __restrict__ dx,
                                                             long long R, long long C, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long a = i / (R * C), c = i % C;
        dx[i] = from_f<T>(to_f<T>(x[i]) > 0.f ? dpool[a * C + c] : 0.f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void tanh_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        y[i] = from_f<T>((tanhf(to_f<T>(x[i])) + 1.f) * 0.5f);
}
template <typename T>
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                                       T* __restrict__ dx, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float t = 2.f * to_f<T>(y[i]) - 1.f;
        dx[i] = from_f<T>(to_f<T>(dy[i]) * 0.5f * (1.f - t * t));
    }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        y[i] = from_f<TO>(to_f<TI>(x[i]));
}

template <typename T>
__global__ __launch_bounds__(256) void add_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                  T* __restrict__ o, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        o[i] = from_f<T>(to_f<T>(a[i]) + to_f<T>(b[i]));
}

// flax.optim.Adam + EMA over a flat arena, float4 per lane.
// Round 4: FIX -- the gradient through sigma of the spectrally-normalised tensors (xmcgan/libml/layers.py:217-219:
// G <- (G - k u (x) v) / (sigma + eps), k = <G, W> / (sigma + eps)) is applied to the gradient on its way into the moments
// instead of by a separate read-modify-write pass over the gradient arena (sn_fix_kernel: 2 reads + 1 write of 352 MB per
// half step).  `map` has one int16 per 64 arena elements (every tensor starts 64-aligned: ParamArena.ALIGN): the index of the
// spectral table entry that owns them, or -1.  zero_g: the consumed gradient is overwritten with zeros (the next half step
// accumulates into a clean arena without a separate fill).
// GUARD (config.skip_nonfinite_updates; xmc_*_guarded): verdict[0] != 0 (xmc_nonfinite_verdict found a NaN or an infinity in what
// this half step would commit) leaves p, m, v and ema as they are; the gradient is still zeroed where zero_g == 1 would zero
// it, so that the bad values do not reach the next half step.  The GUARD = false instantiation is the kernel as it was, and
// stays so in BITS: the arithmetic of all four instantiations (and of adam_wprep_kernel) is the one definition of adam_update.h,
// whose roundings are written out and reproduce what the float4 loop computed before (tests/test_gpu_adam_bits.py).  The scalar
// tail -- never run by the product: ParamArena pads every arena to 64 -- takes the loop's rounding too.
// SCHED (xmc_*_sched; libml/opt_schedule.py): lr and d are the float32 values adam_advance_sched_kernel has just left in slots 4
// and 5 of the step state instead of the host's arguments -- two more uniform loads beside the corrections', then the same
// AdamHyper and the same adam_update.  The SCHED = false instantiations are the kernels as they were.
template <bool FIX, bool GUARD = false, bool SCHED = false>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   float* __restrict__ ema, long long n, float lr, float b1,
                                                   float b2, float eps, float ic1, float ic2, float gs, float d,
                                                   const float* __restrict__ corr, int zero_g, const short* __restrict__ map,
                                                   const xmc_sn_entry* __restrict__ tab, const float* __restrict__ kvec,
                                                   const float* __restrict__ scal, const float* __restrict__ uvec,
                                                   const float* __restrict__ vvec, const int* __restrict__ verdict = nullptr) {
    if constexpr (GUARD) {
        if (verdict[0] != 0) {                       // skipped half step (uniform over the grid)
            if (zero_g != 1) return;
            const long long q4 = n >> 2;
            for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < q4; i += (long long)gridDim.x * 256) {
                if (map && map[i >> 4] == -2) continue;
                reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if (blockIdx.x == 0 && threadIdx.x < (n & 3)) g[(q4 << 2) + threadIdx.x] = 0.f;
            return;
        }
    }
    if (corr) { ic1 = corr[1]; ic2 = corr[2]; }      // device-side step counter (hipGraph replay): see adam_advance_kernel
    if constexpr (SCHED) { lr = corr[4]; d = corr[5]; }      // this update's rate and EMA decay: see adam_advance_sched_kernel
    const AdamHyper h = {lr, b1, b2, eps, ic1, ic2, gs, d};
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        float* gf = reinterpret_cast<float*>(&gg);
        bool fixed = false;
        if constexpr (!FIX) {
            if (map && map[i >> 4] == -2) continue;  // a tensor the fused optimiser + preparation kernel updates (adam_wprep_kernel)
        }
        if constexpr (FIX) {
            const int ent = map[i >> 4];
            if (ent == -2) continue;
            fixed = ent >= 0;
            if (ent >= 0) {
                const xmc_sn_entry e = tab[ent];
                const float k = kvec[ent], is = scal[2 * ent + 1];
                const unsigned t = (unsigned)((i << 2) - e.w_off), cols = (unsigned)e.cols;     // <= 21 M elements per tensor
                const float* uu = uvec + e.u_off;
                const float* vw = vvec + e.v_off;
                if ((cols & 3u) == 0 && t >= (unsigned)e.rows * cols) {
                    // the tensor's 64-element alignment padding (rows * cols % 64 != 0): it carries no gradient and must not
                    // index u / v past the entry's slices (round-4 advisor finding; no current shape has padding)
                } else if ((cols & 3u) == 0) {       // a float4 never straddles a row
                    const unsigned r = t / cols, c = t - r * cols;
                    if (e.u_axis == 0) sigma_term4(gg, sigma_row_factor(uu[r], k), *reinterpret_cast<const float4*>(vw + c), is);
                    else sigma_term4(gg, sigma_row_factor(vw[r], k), *reinterpret_cast<const float4*>(uu + c), is);
                } else {
                    const unsigned total = (unsigned)e.rows * cols;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned tq = t + q;
                        if (tq < total) {            // (the tensor's 64-element padding carries no gradient)
                            const unsigned r = tq / cols, c = tq - r * cols;
                            gf[q] = e.u_axis == 0 ? sigma_term(gf[q], k, uu[r], vw[c], is) : sigma_term(gf[q], k, uu[c], vw[r], is);
                        }
                    }
                }
            }
        }
        adam_update4(pp, gg, mm, vv, h);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        store_consumed_grad(reinterpret_cast<float4*>(g) + i, gg, zero_g, fixed);
        if (ema) {
            float4 ee = reinterpret_cast<float4*>(ema)[i];
            ema_mix4(ee, pp, d);
            reinterpret_cast<float4*>(ema)[i] = ee;
        }
    }
    // tail (arena sizes are padded to 64 by the host, kept for safety; never part of a spectral tensor)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        adam_update(p[i], g[i], m[i], v[i], h);
        if (zero_g == 1) g[i] = 0.f;
        if (ema) ema[i] = ema_mix(ema[i], p[i], d);
    }
}

inline unsigned grid_for(long long n) {
    long long b = (n + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

extern "C" int xmc_pool2_relu(const void* x, const void* res, void* y, void* xr, int32_t n, int32_t h, int32_t w, int32_t c,
                              float scale, int32_t dtype, void* stream) {
    XMC_REQUIRE(x && y && n > 0 && h >= 2 && w >= 2 && (h % 2) == 0 && (w % 2) == 0 && c > 0);
    XMC_REQUIRE(dtype == XMC_F32 || dtype == XMC_BF16);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ve0 = dtype == XMC_BF16 ? 8 : 4;
    const bool vec = (c % ve0) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 &&
                     (res == nullptr || ((uintptr_t)res % 16) == 0) && (xr == nullptr || ((uintptr_t)xr % 16) == 0);
    const int ve = vec ? ve0 : 1;
    const long long nvec = (long long)n * (h / 2) * (w / 2) * (c / ve);
    dim3 grid(grid_for(nvec)), block(256);
#define XMC_POOL2(T, VE_)                                                                                                       \
    do {                                                                                                                        \
        if (xr) hipLaunchKernelGGL((pool2_kernel<T, VE_, true>), grid, block, 0, s, static_cast<const T*>(x), static_cast<const T*>(res), \
                                   static_cast<T*>(y), static_cast<T*>(xr), h, w, c, scale, nvec);                             \
        else hipLaunchKernelGGL((pool2_kernel<T, VE_, false>), grid, block, 0, s, static_cast<const T*>(x), static_cast<const T*>(res),  \
                                static_cast<T*>(y), static_cast<T*>(nullptr), h, w, c, scale, nvec);                           \
    } while (0)
    if (dtype == XMC_BF16) {
        if (vec) XMC_POOL2(bf16_t, 8);
        else XMC_POOL2(bf16_t, 1);
    } else {
        if (vec) XMC_POOL2(float, 4);
        else XMC_POOL2(float, 1);
    }
#undef XMC_POOL2
    XMC_LAUNCH_RET();
}

extern "C" int xmc_pool2(const void* x, const void* res, void* y, int32_t n, int32_t h, int32_t w, int32_t c,
                         float scale, int32_t dtype, void* stream) {
    return xmc_pool2_relu(x, res, y, nullptr, n, h, w, c, scale, dtype, stream);
}

extern "C" int xmc_expand_taps(const void* x, void* y, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ks,
                               int32_t sign, int32_t dtype, void* stream) {
    XMC_REQUIRE(x && y && n > 0 && h > 0 && w > 0 && c > 0 && (ks == 1 || ks == 3) && ks * ks * c <= 32);
    XMC_REQUIRE(sign == 1 || sign == -1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long npix = (long long)n * h * w;
    if (dtype == XMC_BF16 && ks == 3 && c == 3 && w <= ET_W_MAX && (w * 3) % 8 == 0 && (long long)n * h < (1ll << 31) &&
        (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0)
        hipLaunchKernelGGL(expand_taps3_rows_kernel, dim3((unsigned)((long long)n * h)), dim3(256), 0, s, static_cast<const bf16_t*>(x),
                           static_cast<bf16_t*>(y), h, w, sign);
    else if (dtype == XMC_BF16)
        hipLaunchKernelGGL((expand_taps_kernel<bf16_t>), dim3(grid_for(npix * 4)), dim3(256), 0, s,
                           static_cast<const bf16_t*>(x), static_cast<bf16_t*>(y), h, w, c, ks, sign, npix);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((expand_taps_kernel<float>), dim3(grid_for(npix * 8)), dim3(256), 0, s,
                           static_cast<const float*>(x), static_cast<float*>(y), h, w, c, ks, sign, npix);
    else return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bcast_relu_bwd(const float* dpool, const void* x, void* dx, int64_t a, int64_t r, int64_t c,
                                  int32_t dtype, void* stream) {
    XMC_REQUIRE(dpool && x && dx && a > 0 && r > 0 && c > 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long n = (long long)a * r * c;
    if (dtype == XMC_BF16)
        hipLaunchKernelGGL((bcast_relu_bwd_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s, dpool,
                           static_cast<const bf16_t*>(x), static_cast<bf16_t*>(dx), (long long)r, (long long)c, n);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((bcast_relu_bwd_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s, dpool,
                           static_cast<const float*>(x), static_cast<float*>(dx), (long long)r, (long long)c, n);
    else return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

extern "C" int xmc_tanh_out_fwd(const void* x, void* y, int64_t n, int32_t dtype, void* stream) {
    XMC_REQUIRE(x && y && n > 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == XMC_BF16)
        hipLaunchKernelGGL((tanh_fwd_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s,
                           static_cast<const bf16_t*>(x), static_cast<bf16_t*>(y), (long long)n);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((tanh_fwd_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s,
                           static_cast<const float*>(x), static_cast<float*>(y), (long long)n);
    else return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

extern "C" int xmc_tanh_out_bwd(const void* dy, const void* y, void* dx, int64_t n, int32_t dtype, void* stream) {
    XMC_REQUIRE(dy && y && dx && n > 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == XMC_BF16)
        hipLaunchKernelGGL((tanh_bwd_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s,
                           static_cast<const bf16_t*>(dy), static_cast<const bf16_t*>(y), static_cast<bf16_t*>(dx),
                           (long long)n);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((tanh_bwd_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s,
                           static_cast<const float*>(dy), static_cast<const float*>(y), static_cast<float*>(dx),
                           (long long)n);
    else return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

extern "C" int xmc_cast(const void* x, int32_t dtype_in, void* y, int32_t dtype_out, int64_t n, void* stream) {
    XMC_REQUIRE(x && y && n > 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    dim3 grid(grid_for(n)), block(256);
    if (dtype_in == XMC_F32 && dtype_out == XMC_BF16)
        hipLaunchKernelGGL((cast_kernel<float, bf16_t>), grid, block, 0, s, static_cast<const float*>(x),
                           static_cast<bf16_t*>(y), (long long)n);
    else if (dtype_in == XMC_BF16 && dtype_out == XMC_F32)
        hipLaunchKernelGGL((cast_kernel<bf16_t, float>), grid, block, 0, s, static_cast<const bf16_t*>(x),
                           static_cast<float*>(y), (long long)n);
    else if (dtype_in == XMC_F32 && dtype_out == XMC_F32)
        hipLaunchKernelGGL((cast_kernel<float, float>), grid, block, 0, s, static_cast<const float*>(x),
                           static_cast<float*>(y), (long long)n);
    else if (dtype_in == XMC_BF16 && dtype_out == XMC_BF16)
        hipLaunchKernelGGL((cast_kernel<bf16_t, bf16_t>), grid, block, 0, s, static_cast<const bf16_t*>(x),
                           static_cast<bf16_t*>(y), (long long)n);
    else return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

extern "C" int xmc_add(const void* a, const void* b, void* out, int64_t n, int32_t dtype, void* stream) {
    XMC_REQUIRE(a && b && out && n > 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == XMC_BF16)
        hipLaunchKernelGGL((add_kernel<bf16_t>), dim3(grid_for(n)), dim3(256), 0, s, static_cast<const bf16_t*>(a),
                           static_cast<const bf16_t*>(b), static_cast<bf16_t*>(out), (long long)n);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((add_kernel<float>), dim3(grid_for(n)), dim3(256), 0, s, static_cast<const float*>(a),
                           static_cast<const float*>(b), static_cast<float*>(out), (long long)n);
    else return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

// step counter of one optimiser kept in DEVICE memory: state[0] = t (int32 bits), state[1] = 1 / (1 - beta1^t),
// state[2] = 1 / (1 - beta2^t).  One thread advances t and refreshes the two bias corrections in double precision;
// the Adam kernel launched right behind it reads them -- so a captured hipGraph replays the right step.
template <bool GUARD = false>
__global__ void adam_advance_kernel(float* state, double b1, double b2, const int* verdict = nullptr) {
    if constexpr (GUARD) {
        if (verdict[0] != 0) return;                 // a skipped update does not advance Adam's t
    }
    const int t = __float_as_int(state[0]) + 1;
    state[0] = __int_as_float(t);
    state[1] = (float)(1.0 / (1.0 - pow(b1, (double)t)));
    state[2] = (float)(1.0 / (1.0 - pow(b2, (double)t)));
}

// The scheduled form (xmc_*_sched): the same advance of t and of the two corrections, then this update's learning rate and EMA
// decay from the schedule `s` -- a pure function of t and of constants, so one captured graph serves a whole run with warm-up,
// decay and an EMA ramp.  libml/opt_schedule.evaluate is the specification: IEEE double in its order, and no multiply may fuse
// with the add behind it (contraction is switched off for the function, as in lecam.hip).  state[4] = lr_t, state[5] = d_t,
// state[6] = float32(w f); slots 3 and 7 are not touched.  ONE thread; a skipped half step (GUARD, verdict[0] != 0) writes nothing.
template <bool GUARD = false>
__global__ void adam_advance_sched_kernel(float* state, double b1, double b2, xmc_opt_schedule s, const int* verdict = nullptr) {
#pragma clang fp contract(off)
    if constexpr (GUARD) {
        if (verdict[0] != 0) return;
    }
    const int t = __float_as_int(state[0]) + 1;
    state[0] = __int_as_float(t);
    state[1] = (float)(1.0 / (1.0 - pow(b1, (double)t)));
    state[2] = (float)(1.0 / (1.0 - pow(b2, (double)t)));
    const double td = (double)t;
    const double w = (s.warmup > 0 && (long long)t < s.warmup) ? td / (double)s.warmup : 1.0;
    double x;
    if ((long long)t <= s.decay_start) x = 0.0;
    else if ((long long)t >= s.decay_end) x = 1.0;
    else x = (double)((long long)t - s.decay_start) / (double)(s.decay_end - s.decay_start);
    const double r = s.final_ratio;
    double f = 1.0;
    if (s.kind == XMC_SCHED_LINEAR) f = 1.0 + (r - 1.0) * x;
    else if (s.kind == XMC_SCHED_COSINE) f = r + (1.0 - r) * (0.5 * (1.0 + cos(3.141592653589793 * x)));
    state[4] = (float)((s.base * w) * f);
    state[6] = (float)(w * f);
    float d;
    if ((long long)t <= s.ema_start) d = 0.f;
    else if (s.ema_ramp > 0.0) d = (float)fmin(s.ema_decay, (1.0 + td) / (s.ema_ramp + td));
    else d = (float)s.ema_decay;
    state[5] = d;
}

namespace {

// What the five flat entry points below hand to launch_adam_flat, in the order of their own parameters: an entry point fills the
// fields it has, the rest keep their defaults (the gradient left alone, no map, no table, no verdict).
struct AdamFlatArgs {
    float *p, *g, *m, *v, *ema;
    int64_t n;
    float lr;
    double beta1, beta2;
    float eps;
    float* step_state;                               // advanced here, read by the kernel (NULL with host_step)
    float grad_scale, ema_decay;
    void* stream;
    int32_t zero_grads = 0;
    const void *map = nullptr, *table = nullptr;
    int32_t n_entries = 0;
    const float *kvec = nullptr, *scal = nullptr, *u = nullptr, *vv = nullptr;
    bool guarded = false;
    const int32_t* verdict = nullptr;
    bool host_step = false;                          // xmc_adam_ema: the caller computed c = 1 - beta^t
    float c1 = 1.f, c2 = 1.f;
    bool scheduled = false;                          // xmc_*_sched: lr and ema_decay come from `sched` through the step state
    const xmc_opt_schedule* sched = nullptr;
};

// the domain of a schedule descriptor (include/xmcgan_hip.h; libml/opt_schedule.Schedule.validate is the same list)
int validate_opt_schedule(const xmc_opt_schedule* s) {
    XMC_REQUIRE(s != nullptr);
    XMC_REQUIRE(s->kind == XMC_SCHED_CONSTANT || s->kind == XMC_SCHED_LINEAR || s->kind == XMC_SCHED_COSINE);
    XMC_REQUIRE(s->reserved == 0);
    XMC_REQUIRE(std::isfinite(s->base) && s->base > 0.0);
    XMC_REQUIRE(s->warmup >= 0 && s->decay_start >= 0 && s->decay_end >= 0 && s->ema_start >= 0);
    XMC_REQUIRE(s->kind == XMC_SCHED_CONSTANT || s->decay_end > s->decay_start);
    XMC_REQUIRE(std::isfinite(s->final_ratio) && s->final_ratio >= 0.0 && s->final_ratio <= 1.0);
    XMC_REQUIRE(s->ema_decay >= 0.0 && s->ema_decay < 1.0);                 // (a NaN fails both)
    XMC_REQUIRE(std::isfinite(s->ema_ramp) && s->ema_ramp >= 0.0);
    return XMC_OK;
}

int validate_adam_flat(const AdamFlatArgs& a) {
    XMC_REQUIRE(a.p && a.g && a.m && a.v && a.n > 0);
    XMC_REQUIRE(xmc_aligned(a.p, 16) && xmc_aligned(a.g, 16) && xmc_aligned(a.m, 16) && xmc_aligned(a.v, 16) && xmc_aligned(a.ema, 16));     // (ema may be NULL)
    XMC_REQUIRE(a.host_step ? (a.c1 > 0.f && a.c2 > 0.f) : a.step_state != nullptr);
    XMC_REQUIRE(!a.table || (a.map && a.n_entries > 0 && a.kvec && a.scal && a.u && a.vv));     // (map without table: skip marks only)
    XMC_REQUIRE(!a.guarded || (a.verdict && xmc_aligned(a.verdict, 4)));
    if (a.scheduled) {
        XMC_REQUIRE(!a.host_step);
        if (const int rc = validate_opt_schedule(a.sched)) return rc;
    }
    return XMC_OK;
}

// adam_kernel<FIX = a table is given, GUARD = the entry point is a guarded one, SCHED = a scheduled one>, behind
// adam_advance_kernel (adam_advance_sched_kernel) where the step lives on the device
int launch_adam_flat(const AdamFlatArgs& a) {
    if (const int rc = validate_adam_flat(a)) return rc;
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    const int* verdict = a.guarded ? static_cast<const int*>(a.verdict) : nullptr;
    if (a.scheduled)
        hipLaunchKernelGGL(a.guarded ? adam_advance_sched_kernel<true> : adam_advance_sched_kernel<false>, dim3(1), dim3(1), 0, s,
                           a.step_state, a.beta1, a.beta2, *a.sched, verdict);
    else if (!a.host_step)
        hipLaunchKernelGGL(a.guarded ? adam_advance_kernel<true> : adam_advance_kernel<false>, dim3(1), dim3(1), 0, s, a.step_state,
                           a.beta1, a.beta2, verdict);
    const auto plain = a.table ? (a.guarded ? adam_kernel<true, true> : adam_kernel<true, false>)
                               : (a.guarded ? adam_kernel<false, true> : adam_kernel<false, false>);
    const auto sched = a.table ? (a.guarded ? adam_kernel<true, true, true> : adam_kernel<true, false, true>)
                               : (a.guarded ? adam_kernel<false, true, true> : adam_kernel<false, false, true>);
    const auto kernel = a.scheduled ? sched : plain;
    hipLaunchKernelGGL(kernel, dim3(grid_for(a.n / 4 + 1)), dim3(256), 0, s, a.p, a.g, a.m, a.v, a.ema, (long long)a.n, a.lr,
                       (float)a.beta1, (float)a.beta2, a.eps, a.host_step ? 1.f / a.c1 : 1.f, a.host_step ? 1.f / a.c2 : 1.f,
                       a.grad_scale, a.ema_decay, static_cast<const float*>(a.step_state), a.zero_grads,
                       static_cast<const short*>(a.map), static_cast<const xmc_sn_entry*>(a.table), a.kvec, a.scal, a.u, a.vv, verdict);
    XMC_LAUNCH_RET();
}

}  // namespace

extern "C" int xmc_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr,
                            float beta1, float beta2, float eps, float c1, float c2, float grad_scale,
                            float ema_decay, void* stream) {
    AdamFlatArgs a = {p, const_cast<float*>(g), m, v, ema, n, lr, beta1, beta2, eps, nullptr, grad_scale, ema_decay, stream};
    a.host_step = true;
    a.c1 = c1;
    a.c2 = c2;
    return launch_adam_flat(a);
}

extern "C" int xmc_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr,
                                double beta1, double beta2, float eps, float* step_state, float grad_scale,
                                float ema_decay, void* stream) {
    return launch_adam_flat({p, const_cast<float*>(g), m, v, ema, n, lr, beta1, beta2, eps, step_state, grad_scale, ema_decay, stream});
}

// xmc_adam_ema_dev with (a) the consumed gradient zeroed in place (zero_grads) and (b) the gradient through sigma of the
// spectrally-normalised tensors applied on the fly (map != NULL: one int16 per 64 arena elements naming the owning entry of
// `table` -- the dot-chunk table of xmc_sn_batched_dot, whose kvec this reads -- or -1; u / v / scal of the forward's power
// iteration).  Replaces xmc_sn_batched_grad_fix's second kernel + a fill + xmc_adam_ema_dev.
extern "C" int xmc_adam_ema_dev_sn(float* p, float* g, float* m, float* v, float* ema, int64_t n, float lr, double beta1,
                                   double beta2, float eps, float* step_state, float grad_scale, float ema_decay,
                                   int32_t zero_grads, const void* map, const void* table, int32_t n_entries,
                                   const float* kvec, const float* scal, const float* u, const float* vv, void* stream) {
    return launch_adam_flat({p, g, m, v, ema, n, lr, beta1, beta2, eps, step_state, grad_scale, ema_decay, stream, zero_grads, map, table,
                             n_entries, kvec, scal, u, vv});
}

// ---- config.skip_nonfinite_updates: the guarded forms.  Same arguments as the entry points above plus `verdict` (the int32[4]
// of xmc_nonfinite_verdict, read on the device): verdict[0] == 0 runs the same arithmetic, bit for bit; verdict[0] != 0 leaves
// p, m, v, ema and step_state untouched and only zeroes the gradient where the unguarded form would (zero_grads == 1).
extern "C" int xmc_adam_ema_dev_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, double beta1,
                                        double beta2, float eps, float* step_state, float grad_scale, float ema_decay,
                                        const int32_t* verdict, void* stream) {
    AdamFlatArgs a = {p, const_cast<float*>(g), m, v, ema, n, lr, beta1, beta2, eps, step_state, grad_scale, ema_decay, stream};
    a.guarded = true;
    a.verdict = verdict;
    return launch_adam_flat(a);
}

extern "C" int xmc_adam_ema_dev_sn_guarded(float* p, float* g, float* m, float* v, float* ema, int64_t n, float lr, double beta1,
                                           double beta2, float eps, float* step_state, float grad_scale, float ema_decay,
                                           int32_t zero_grads, const void* map, const void* table, int32_t n_entries,
                                           const float* kvec, const float* scal, const float* u, const float* vv,
                                           const int32_t* verdict, void* stream) {
    return launch_adam_flat({p, g, m, v, ema, n, lr, beta1, beta2, eps, step_state, grad_scale, ema_decay, stream, zero_grads, map, table,
                             n_entries, kvec, scal, u, vv, true, verdict});
}

// ---- the scheduled forms (config.lr_schedule, config.ema_ramp, ...; libml/opt_schedule.py): the entry points above without `lr` and
// `ema_decay`, which adam_advance_sched_kernel derives from `sched` and Adam's t on the device.  `verdict` may be NULL: the
// unguarded form.
extern "C" int xmc_adam_ema_dev_sched(float* p, const float* g, float* m, float* v, float* ema, int64_t n, double beta1, double beta2,
                                      float eps, float* step_state, float grad_scale, const xmc_opt_schedule* sched,
                                      const int32_t* verdict, void* stream) {
    AdamFlatArgs a = {p, const_cast<float*>(g), m, v, ema, n, 0.f, beta1, beta2, eps, step_state, grad_scale, 0.f, stream};
    a.guarded = verdict != nullptr;
    a.verdict = verdict;
    a.scheduled = true;
    a.sched = sched;
    return launch_adam_flat(a);
}

extern "C" int xmc_adam_ema_dev_sn_sched(float* p, float* g, float* m, float* v, float* ema, int64_t n, double beta1, double beta2,
                                         float eps, float* step_state, float grad_scale, int32_t zero_grads, const void* map,
                                         const void* table, int32_t n_entries, const float* kvec, const float* scal, const float* u,
                                         const float* vv, const xmc_opt_schedule* sched, const int32_t* verdict, void* stream) {
    AdamFlatArgs a = {p, g, m, v, ema, n, 0.f, beta1, beta2, eps, step_state, grad_scale, 0.f, stream, zero_grads, map, table,
                      n_entries, kvec, scal, u, vv, verdict != nullptr, verdict};
    a.scheduled = true;
    a.sched = sched;
    return launch_adam_flat(a);
}

// Running sums of a step's scalar metrics, kept on the device so that a replayed training graph needs no host read per step
// (train_utils.MetricAccumulator).  The n <= 8 input pointers travel by value in the kernel arguments; ONE thread adds
// *vals[i] to sums[i] in float64 in index order, counts the call in info[0] and records in info[1] the (1-based) first call
// that saw a non-finite value.  Plain loads and stores: launches on one stream are ordered, nothing else touches the buffers.
struct metric_ptrs { const float* p[8]; };

// GUARD (xmc_metrics_accum_if): a skipped half step (verdict[0] != 0) adds nothing and is not counted as a call.
template <bool GUARD = false>
__global__ void metrics_accum_kernel(metric_ptrs v, int n, double* sums, int* info, const int* verdict = nullptr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if constexpr (GUARD) {
        if (verdict[0] != 0) return;
    }
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < n) {
            const float x = *v.p[i];
            sums[i] += (double)x;
            bad = bad || !(fabsf(x) <= 3.402823466e+38f);      // NaN and +-inf both fail the comparison
        }
    }
    const int call = info[0] + 1;
    info[0] = call;
    if (bad && info[1] == 0) info[1] = call;
}

extern "C" int xmc_metrics_accum(const float* const* vals, int32_t n, double* sums, int32_t* info, void* stream) {
    XMC_REQUIRE(vals && sums && info && n >= 1 && n <= 8);
    XMC_REQUIRE(((uintptr_t)sums % 8) == 0 && ((uintptr_t)info % 4) == 0);
    metric_ptrs v;
    for (int i = 0; i < 8; ++i) {
        v.p[i] = i < n ? vals[i] : nullptr;
        XMC_REQUIRE(i >= n || (v.p[i] && ((uintptr_t)v.p[i] % 4) == 0));
    }
    hipLaunchKernelGGL((metrics_accum_kernel<false>), dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), v, (int)n, sums, info,
                       (const int*)nullptr);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_metrics_accum_if(const float* const* vals, int32_t n, double* sums, int32_t* info, const int32_t* verdict,
                                    void* stream) {
    XMC_REQUIRE(vals && sums && info && n >= 1 && n <= 8 && verdict);
    XMC_REQUIRE(((uintptr_t)sums % 8) == 0 && ((uintptr_t)info % 4) == 0 && ((uintptr_t)verdict % 4) == 0);
    metric_ptrs v;
    for (int i = 0; i < 8; ++i) {
        v.p[i] = i < n ? vals[i] : nullptr;
        XMC_REQUIRE(i >= n || (v.p[i] && ((uintptr_t)v.p[i] % 4) == 0));
    }
    hipLaunchKernelGGL((metrics_accum_kernel<true>), dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), v, (int)n, sums, info,
                       static_cast<const int*>(verdict));
    XMC_LAUNCH_RET();
}

extern "C" int xmc_abi_version(void) { return XMC_ABI_VERSION; }
