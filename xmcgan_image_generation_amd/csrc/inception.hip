// Inception-v3 feature path for FID / Inception Score (xmcgan/utils/inception_arch.py, eval_metrics.py).
//
// xmc_inception_conv: general implicit-GEMM NHWC convolution, kh, kw in 1..7, stride 1 or 2, explicit top / left zero
// padding, any map size, bias + ReLU epilogue (eval-mode BatchNorm folded into w / bias by the caller).  The input may be
// a channel slice of a wider row (ldx, x_off) and the output is written into a channel slice of a wider row (ldy, y_off),
// so Inception's four-way concatenations are free.  Generalises conv_igemm.hip (same 128-pixel x 128-channel tile, same
// LDS staging and CT<float> / CT<bf16_t> split):
//   D[cout][pixel] += W[cout][k] * A[pixel][k],  k = (tap, cin),  A gathered on the fly
// on v_mfma_f32_32x32x16_bf16 (bf16, fp32 accumulation) or v_mfma_f32_32x32x2_f32 (exact fp32).  There is no split-K
// and the tile shape is fixed, so the K order of every output is the tap-major / channel-minor order of its own pixel:
// an image's features do not depend on the batch size or on which images share the launch.
// The first layer (cin = 3, K = 27, VALID) has its own scalar gather that applies clip(2x - 1, -1, 1) as it loads.
//
// xmc_maxpool3x3s2_valid / xmc_avgpool3x3_same / xmc_mean_hw: the pools (VALID 3x3 stride-2 max into a channel slice,
// TF-style 3x3 SAME average whose divisor counts the in-bounds taps, and the per-image global mean in a fixed order).
#include "common.h"

namespace {

constexpr int BM = 128;   // pixels per tile
constexpr int BN = 128;   // output channels per tile

template <typename T> struct CT;
template <> struct CT<bf16_t> {
    static constexpr int VE = 8;      // elements per 16-byte vector
    static constexpr int BK = 32;     // K elements per LDS tile row (64 bytes)
    static constexpr int PITCH = 40;  // 80-byte rows: ds_read_b128 conflict-free
    using VT = uint4;
};
template <> struct CT<float> {
    static constexpr int VE = 4;
    static constexpr int BK = 16;
    static constexpr int PITCH = 17;  // odd pitch: ds_read_b32 of 32 consecutive rows conflict-free
    using VT = float4;
};

struct IconvArgs {
    const void* x; const void* w; const float* bias; void* y;
    int N, Hi, Wi, Cin, Ho, Wo, Cout;
    int kh, kw, stride, pad_t, pad_l;
    int ldx, x_off, ldy, y_off;
    int relu;
    int M, cchunks, ktiles, tiles_m, tiles_n, K;
};

template <typename T> struct Stage;
template <> struct Stage<bf16_t> { uint4 a[2], b[2]; };
template <> struct Stage<float> { float4 a[2], b[2]; };

__device__ __forceinline__ void zero_vec(uint4& v) { v = make_uint4(0, 0, 0, 0); }
__device__ __forceinline__ void zero_vec(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void set_elem(uint4& v, int e, bf16_t x) {
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
    w[e >> 1] |= ((uint32_t)x) << ((e & 1) * 16);
}
__device__ __forceinline__ void set_elem(float4& v, int e, float x) { reinterpret_cast<float*>(&v)[e] = x; }

// FIRST: the network's first layer -- scalar gather over k = tap * Cin + c (Cin = 3), clip(2x - 1, -1, 1) applied to
// every loaded pixel value (no zero padding in a VALID layer, so no padded tap would see the transform)
template <typename T, bool FIRST>
__global__ __launch_bounds__(256) void inception_conv_kernel(const IconvArgs p) {
    using C = CT<T>;
    using VT = typename C::VT;
    constexpr int VE = C::VE, BK = C::BK, PITCH = C::PITCH;
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * 128 * PITCH];   // [buf][A|B][row][PITCH]
    T* const As = lds;
    T* const Bs = lds + 2 * 128 * PITCH;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
    const int tn = tile / p.tiles_m, tm = tile - tn * p.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;

    const T* __restrict__ x = static_cast<const T*>(p.x);
    const T* __restrict__ w = static_cast<const T*>(p.w);

    // loader geometry: thread -> (row, 16-byte slot) of the K row; the top-left input corner of its two pixels
    const int lrow = tid >> 2, kv = tid & 3;
    int iy0[2], ix0[2];
    size_t nb[2];
    bool pv[2];
    const int howo = p.Ho * p.Wo;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int pix = m0 + lrow + 64 * r;
        pv[r] = pix < p.M;
        const int pp = pv[r] ? pix : 0;
        const int n = pp / howo, rem = pp - n * howo;
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        iy0[r] = oy * p.stride - p.pad_t;
        ix0[r] = ox * p.stride - p.pad_l;
        nb[r] = (size_t)n * p.Hi * p.Wi;
    }

    auto load_tile = [&](int kt, Stage<T>& s) {
        if constexpr (FIRST) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                zero_vec(s.a[r]);
                zero_vec(s.b[r]);
                const int nrow = n0 + lrow + 64 * r;
                for (int e = 0; e < VE; ++e) {
                    const int j = kt * BK + kv * VE + e;
                    if (j >= p.K) break;
                    const int tp = j / p.Cin, cc = j - tp * p.Cin;
                    const int ty = tp / p.kw, tx = tp - ty * p.kw;
                    const int iy = iy0[r] + ty, ix = ix0[r] + tx;
                    if (pv[r] && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi) {
                        const float v = to_f<T>(x[(nb[r] + (size_t)iy * p.Wi + ix) * p.ldx + p.x_off + cc]);
                        set_elem(s.a[r], e, from_f<T>(fminf(fmaxf(2.f * v - 1.f, -1.f), 1.f)));
                    }
                    if (nrow < p.Cout) set_elem(s.b[r], e, w[(size_t)nrow * p.K + j]);
                }
            }
            return;
        }
        const int tap = kt / p.cchunks;
        const int c = (kt - tap * p.cchunks) * BK + kv * VE;     // Cin % 8 == 0: a vector is all in or all out
        const int ty = tap / p.kw, tx = tap - ty * p.kw;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            zero_vec(s.a[r]);
            const int iy = iy0[r] + ty, ix = ix0[r] + tx;
            if (pv[r] && c < p.Cin && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi)
                s.a[r] = *reinterpret_cast<const VT*>(x + (nb[r] + (size_t)iy * p.Wi + ix) * p.ldx + p.x_off + c);
            zero_vec(s.b[r]);
            const int nrow = n0 + lrow + 64 * r;
            if (nrow < p.Cout && c < p.Cin)
                s.b[r] = *reinterpret_cast<const VT*>(w + ((size_t)nrow * (p.kh * p.kw) + tap) * p.Cin + c);
        }
    };
    auto store_tile = [&](int buf, const Stage<T>& s) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            T* da = As + (buf * 128 + lrow + 64 * r) * PITCH + kv * VE;
            T* db = Bs + (buf * 128 + lrow + 64 * r) * PITCH + kv * VE;
            if constexpr (sizeof(T) == 2) {
                *reinterpret_cast<uint4*>(da) = s.a[r];
                *reinterpret_cast<uint4*>(db) = s.b[r];
            } else {
                const float* fa = reinterpret_cast<const float*>(&s.a[r]);
                const float* fb = reinterpret_cast<const float*>(&s.b[r]);
#pragma unroll
                for (int e = 0; e < 4; ++e) { da[e] = fa[e]; db[e] = fb[e]; }
            }
        }
    };

    // wave -> 64 (cout) x 64 (pixel) sub-tile, as 2 x 2 MFMA 32x32 blocks
    const int wp = wave & 1, wc = wave >> 1;
    const int l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    auto compute = [&](int buf) {
        const T* a_base = As + (buf * 128 + wp * 64 + l31) * PITCH;
        const T* b_base = Bs + (buf * 128 + wc * 64 + l31) * PITCH;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 wf[2], xf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    wf[i] = *reinterpret_cast<const bf16x8*>(b_base + i * 32 * PITCH + kk * 16 + lhi * 8);
                    xf[i] = *reinterpret_cast<const bf16x8*>(a_base + i * 32 * PITCH + kk * 16 + lhi * 8);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                float wf[2], xf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    wf[i] = b_base[i * 32 * PITCH + kk * 2 + lhi];
                    xf[i] = a_base[i * 32 * PITCH + kk * 2 + lhi];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[i], xf[j], acc[i][j], 0, 0, 0);
            }
        }
    };

    // main loop: register-staged double buffering, one barrier per K tile
    Stage<T> st;
    load_tile(0, st);
    store_tile(0, st);
    __syncthreads();
    for (int kt = 0; kt < p.ktiles; ++kt) {
        const int buf = kt & 1;
        const bool more = kt + 1 < p.ktiles;
        if (more) load_tile(kt + 1, st);
        compute(buf);
        if (more) store_tile(buf ^ 1, st);
        __syncthreads();
    }

    // epilogue.  C/D map of the 32x32 MFMA: col = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    // (cout): registers 4g .. 4g+3 are 4 consecutive output channels (Cout % 8 == 0: all four valid together)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int pix = m0 + wp * 64 + j * 32 + l31;
        if (pix >= p.M) continue;
        const size_t obase = (size_t)pix * p.ldy + p.y_off;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = n0 + wc * 64 + i * 32 + g * 8 + lhi * 4;
                if (c0 >= p.Cout) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = acc[i][j][g * 4 + e];
                    if (p.bias) v[e] += p.bias[c0 + e];
                    if (p.relu) v[e] = fmaxf(v[e], 0.f);
                }
                if constexpr (sizeof(T) == 4) {
                    *reinterpret_cast<float4*>(static_cast<float*>(p.y) + obase + c0) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    *reinterpret_cast<uint2*>(static_cast<bf16_t*>(p.y) + obase + c0) =
                        make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
                }
            }
        }
    }
}

// one thread per (output pixel, 8-channel group): 3x3 stride-2 VALID max pool into the channel slice [y_off, y_off + c)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_valid_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int hi, int wi,
                                                            int c, int ho, int wo, int ldy, int y_off) {
    const int cg = c >> 3;
    const long long total = (long long)n * ho * wo * cg;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % cg);
    const long long pix = t / cg;
    const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho), b = (int)(pix / ((long long)wo * ho));
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
            const T* src = x + (((size_t)b * hi + 2 * oy + dy) * wi + 2 * ox + dx) * c + g * 8;
#pragma unroll
            for (int h = 0; h < 8 / Vec<T>::N; ++h) {
                Vec<T> v;
                v.load(src + h * Vec<T>::N);
                float f[Vec<T>::N];
                v.get(f);
#pragma unroll
                for (int e = 0; e < Vec<T>::N; ++e) m[h * Vec<T>::N + e] = fmaxf(m[h * Vec<T>::N + e], f[e]);
            }
        }
    T* dst = y + (size_t)pix * ldy + y_off + g * 8;
#pragma unroll
    for (int h = 0; h < 8 / Vec<T>::N; ++h) {
        Vec<T> v;
        v.set(m + h * Vec<T>::N);          // max of bf16 values is a bf16 value: the round trip is exact
        v.store(dst + h * Vec<T>::N);
    }
}

// one thread per (pixel, 8-channel group): 3x3 stride-1 SAME average, divisor = in-bounds taps (TF's avg_pool; the
// reference's tensorflow_style_avg_pooling), fp32 sums in row-major tap order
template <typename T>
__global__ __launch_bounds__(256) void avgpool_same_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int h, int w, int c) {
    const int cg = c >> 3;
    const long long total = (long long)n * h * w * cg;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % cg);
    const long long pix = t / cg;
    const int px = (int)(pix % w), py = (int)((pix / w) % h), b = (int)(pix / ((long long)w * h));
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    int cnt = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int iy = py + dy;
        if ((unsigned)iy >= (unsigned)h) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int ix = px + dx;
            if ((unsigned)ix >= (unsigned)w) continue;
            ++cnt;
            const T* src = x + (((size_t)b * h + iy) * w + ix) * c + g * 8;
#pragma unroll
            for (int hh = 0; hh < 8 / Vec<T>::N; ++hh) {
                Vec<T> v;
                v.load(src + hh * Vec<T>::N);
                float f[Vec<T>::N];
                v.get(f);
#pragma unroll
                for (int e = 0; e < Vec<T>::N; ++e) s[hh * Vec<T>::N + e] += f[e];
            }
        }
    }
    const float inv = 1.f / (float)cnt;
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] *= inv;
    T* dst = y + (size_t)pix * c + g * 8;
#pragma unroll
    for (int hh = 0; hh < 8 / Vec<T>::N; ++hh) {
        Vec<T> v;
        v.set(s + hh * Vec<T>::N);
        v.store(dst + hh * Vec<T>::N);
    }
}

// one thread per (image, channel): the mean over the hw pixels of that image, summed in pixel order (float32 out)
template <typename T>
__global__ __launch_bounds__(256) void mean_hw_kernel(const T* __restrict__ x, float* __restrict__ y, int n, int hw, int c) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * c) return;
    const int ch = (int)(t % c), b = (int)(t / c);
    const T* src = x + (size_t)b * hw * c + ch;
    float s = 0.f;
    for (int i = 0; i < hw; ++i) s += to_f<T>(src[(size_t)i * c]);
    y[t] = s / (float)hw;
}

inline unsigned blocks_for(long long threads) { return (unsigned)((threads + 255) / 256); }
inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int xmc_inception_conv(const xmc_iconv_desc* d, const void* x, const void* w, const float* bias, void* y,
                                  void* stream) {
    XMC_REQUIRE(d && x && w && y);
    XMC_REQUIRE(d->dtype == XMC_F32 || d->dtype == XMC_BF16);
    XMC_REQUIRE(d->n > 0 && d->hi > 0 && d->wi > 0 && d->cin > 0 && d->ho > 0 && d->wo > 0 && d->cout > 0);
    XMC_REQUIRE(d->kh >= 1 && d->kh <= 7 && d->kw >= 1 && d->kw <= 7 && (d->stride == 1 || d->stride == 2));
    XMC_REQUIRE(d->pad_t >= 0 && d->pad_l >= 0 && d->pad_t < d->kh && d->pad_l < d->kw);
    // every output window must start inside the padded input (no output reads only padding past the bottom / right)
    XMC_REQUIRE((long long)(d->ho - 1) * d->stride - d->pad_t < d->hi && (long long)(d->wo - 1) * d->stride - d->pad_l < d->wi);
    XMC_REQUIRE(d->cout % 8 == 0 && d->ldy % 8 == 0 && d->y_off % 8 == 0 && d->y_off >= 0 && d->y_off + d->cout <= d->ldy);
    XMC_REQUIRE(d->x_off >= 0 && d->x_off + d->cin <= d->ldx);
    if (d->first) {
        // the first layer: tiny cin, contiguous input, VALID (the clip(2x - 1) transform must not meet a padded tap)
        XMC_REQUIRE(d->cin < 8 && d->x_off == 0 && d->ldx == d->cin && d->pad_t == 0 && d->pad_l == 0);
    } else {
        XMC_REQUIRE(d->cin % 8 == 0 && d->ldx % 8 == 0 && d->x_off % 8 == 0);
        XMC_REQUIRE(aligned16(x) && aligned16(w));
    }
    XMC_REQUIRE(aligned16(y));
    const long long m = (long long)d->n * d->ho * d->wo;
    const long long rows_in = (long long)d->n * d->hi * d->wi;
    XMC_REQUIRE(m < (1ll << 31) && m * d->ldy < (1ll << 40) && rows_in * d->ldx < (1ll << 40));
    IconvArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.N = d->n; a.Hi = d->hi; a.Wi = d->wi; a.Cin = d->cin; a.Ho = d->ho; a.Wo = d->wo; a.Cout = d->cout;
    a.kh = d->kh; a.kw = d->kw; a.stride = d->stride; a.pad_t = d->pad_t; a.pad_l = d->pad_l;
    a.ldx = d->ldx; a.x_off = d->x_off; a.ldy = d->ldy; a.y_off = d->y_off; a.relu = d->relu;
    a.M = (int)m;
    const int bk = d->dtype == XMC_BF16 ? CT<bf16_t>::BK : CT<float>::BK;
    a.K = d->kh * d->kw * d->cin;
    a.cchunks = (d->cin + bk - 1) / bk;
    a.ktiles = d->first ? (a.K + bk - 1) / bk : d->kh * d->kw * a.cchunks;
    a.tiles_m = (int)((m + BM - 1) / BM);
    a.tiles_n = (d->cout + BN - 1) / BN;
    dim3 grid(a.tiles_m * a.tiles_n), block(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d->dtype == XMC_BF16) {
        if (d->first) hipLaunchKernelGGL((inception_conv_kernel<bf16_t, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((inception_conv_kernel<bf16_t, false>), grid, block, 0, s, a);
    } else {
        if (d->first) hipLaunchKernelGGL((inception_conv_kernel<float, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((inception_conv_kernel<float, false>), grid, block, 0, s, a);
    }
    XMC_LAUNCH_RET();
}

extern "C" int xmc_maxpool3x3s2_valid(const void* x, void* y, int32_t n, int32_t hi, int32_t wi, int32_t c, int32_t ldy,
                                      int32_t y_off, int32_t dtype, void* stream) {
    XMC_REQUIRE(x && y && n > 0 && hi >= 3 && wi >= 3 && c > 0 && c % 8 == 0);
    XMC_REQUIRE(ldy % 8 == 0 && y_off % 8 == 0 && y_off >= 0 && y_off + c <= ldy);
    XMC_REQUIRE(aligned16(x) && aligned16(y));
    const int ho = (hi - 3) / 2 + 1, wo = (wi - 3) / 2 + 1;
    const long long threads = (long long)n * ho * wo * (c / 8);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == XMC_BF16)
        hipLaunchKernelGGL((maxpool_valid_kernel<bf16_t>), dim3(blocks_for(threads)), dim3(256), 0, s,
                           static_cast<const bf16_t*>(x), static_cast<bf16_t*>(y), n, hi, wi, c, ho, wo, ldy, y_off);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((maxpool_valid_kernel<float>), dim3(blocks_for(threads)), dim3(256), 0, s,
                           static_cast<const float*>(x), static_cast<float*>(y), n, hi, wi, c, ho, wo, ldy, y_off);
    else
        return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

extern "C" int xmc_avgpool3x3_same(const void* x, void* y, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype,
                                   void* stream) {
    XMC_REQUIRE(x && y && x != y && n > 0 && h > 0 && w > 0 && c > 0 && c % 8 == 0);
    XMC_REQUIRE(aligned16(x) && aligned16(y));
    const long long threads = (long long)n * h * w * (c / 8);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == XMC_BF16)
        hipLaunchKernelGGL((avgpool_same_kernel<bf16_t>), dim3(blocks_for(threads)), dim3(256), 0, s,
                           static_cast<const bf16_t*>(x), static_cast<bf16_t*>(y), n, h, w, c);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((avgpool_same_kernel<float>), dim3(blocks_for(threads)), dim3(256), 0, s,
                           static_cast<const float*>(x), static_cast<float*>(y), n, h, w, c);
    else
        return XMC_EINVAL;
    XMC_LAUNCH_RET();
}

extern "C" int xmc_mean_hw(const void* x, float* y, int32_t n, int32_t hw, int32_t c, int32_t dtype, void* stream) {
    XMC_REQUIRE(x && y && n > 0 && hw > 0 && c > 0);
    const long long threads = (long long)n * c;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == XMC_BF16)
        hipLaunchKernelGGL((mean_hw_kernel<bf16_t>), dim3(blocks_for(threads)), dim3(256), 0, s,
                           static_cast<const bf16_t*>(x), y, n, hw, c);
    else if (dtype == XMC_F32)
        hipLaunchKernelGGL((mean_hw_kernel<float>), dim3(blocks_for(threads)), dim3(256), 0, s,
                           static_cast<const float*>(x), y, n, hw, c);
    else
        return XMC_EINVAL;
    XMC_LAUNCH_RET();
}
