// Differentiable augmentation of the discriminator's inputs (libml/diff_augment.py is the specification; config.diff_augment).
// Per sample an affine map: brightness / saturation / contrast, an integer translation with zero fill, a cutout box.  The forward
// kernel writes D's (2B, H, W, 3) input directly from the real and the generated half (no concatenation copy); the backward
// kernel is the exact transpose on the generated half.  The random parameters come from a plan of eight float32 per sample
// {b, s, k, ty, tx, y0, x0, c} that the host drew.
//
// Float32 arithmetic, one rounding on store.  The only reduction -- the per-sample mean of the contrast step -- is fixed-order:
// a thread's units in index order, a wave butterfly, the workgroup's four waves in order, one partial per workgroup in the
// caller's workspace, and the second launch adds a sample's partials with another wave butterfly.  No atomics: two launches on
// the same input give the same bits.  Every output element has exactly one writer, the zeros of the border and the box included.
#include "common.h"

#include <cmath>

namespace {

constexpr int DA_THREADS = 256;
constexpr int DA_MAX_PARTS = 64;         // partial sums per sample: one wave adds them
constexpr int DA_UNITS_PER_THREAD = 4;   // units a thread of the reduction adds before the tree (12 KiB per workgroup and pass)
constexpr int DA_MAX_BLOCKS = 4096;
constexpr int DA_MAX_SIDE = 16384;
constexpr int DA_BOX_LIM = 1 << 20;

struct da_args {
    const void* src0;                    // samples [0, n0)
    const void* src1;                    // samples [n0, n): forward only (the generated half)
    const float* plan;                   // [n][8]
    void* out;                           // [n][h][w][3]
    float* part;                         // [n][nparts], contrast only
    int n0, h, w, nparts, flags, vec;
};

struct da_row {
    float b, s, k;
    int ty, tx, y0, x0, y1, x1;
};

// float -> int inside [-lim, lim]; a NaN gives -lim (fmaxf returns its other operand)
__device__ __forceinline__ int da_int(float v, int lim) { return (int)fminf(fmaxf(v, -(float)lim), (float)lim); }

// the launch validated the caller's HOST copy of the plan; whatever the device copy holds, the shifts stay inside the image
// (and every load below is bounds-checked on its own), the box is only ever compared with
__device__ __forceinline__ da_row da_load_row(const float* __restrict__ p, int h, int w) {
    da_row r;
    r.b = p[0], r.s = p[1], r.k = p[2];
    r.ty = da_int(p[3], h - 1), r.tx = da_int(p[4], w - 1);
    r.y0 = da_int(p[5], DA_BOX_LIM), r.x0 = da_int(p[6], DA_BOX_LIM);
    const int c = max(da_int(p[7], DA_BOX_LIM), 0);
    r.y1 = r.y0 + c, r.x1 = r.x0 + c;
    return r;
}

__device__ __forceinline__ bool da_in_box(const da_row& r, int y, int x) { return y >= r.y0 && y < r.y1 && x >= r.x0 && x < r.x1; }

// the Vec<T>::N pixels (sy, sx0 ..) of one sample as 3 N floats; a pixel outside the image reads as zeros.  Three 16-byte loads
// when the run is whole and starts on a 16-byte boundary (vec: rows are multiples of 16 bytes from an aligned base, so that is
// sx0 % N == 0), element loads otherwise
template <typename T>
__device__ __forceinline__ void da_gather(const T* __restrict__ s, int h, int w, int sy, int sx0, bool vec, float* v) {
    constexpr int N = Vec<T>::N;
    if (sy < 0 || sy >= h) {
#pragma unroll
        for (int i = 0; i < 3 * N; ++i) v[i] = 0.f;
        return;
    }
    const T* __restrict__ row = s + (size_t)sy * (3 * w);
    if (vec && sx0 >= 0 && sx0 + N <= w && (sx0 % N) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Vec<T> q;
            q.load(row + 3 * sx0 + i * N);
            q.get(v + i * N);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int x = sx0 + j;
        const bool ok = x >= 0 && x < w;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * j + c] = ok ? to_f<T>(row[3 * x + c]) : 0.f;
    }
}

template <typename T> __device__ __forceinline__ const T* da_sample(const da_args& a, int n) {
    const size_t elems = (size_t)a.h * a.w * 3;
    return n < a.n0 ? static_cast<const T*>(a.src0) + (size_t)n * elems : static_cast<const T*>(a.src1) + (size_t)(n - a.n0) * elems;
}

// grid (nparts, n).  Forward: the plain sum of sample n.  Backward: the sum of g over the pixels p that step 1 of the adjoint
// keeps -- p outside the box with p - t inside the image -- which is the sum of the shifted, masked gradient.
template <typename T, bool BWD> __global__ __launch_bounds__(DA_THREADS) void da_reduce_kernel(da_args a) {
    constexpr int N = Vec<T>::N;
    const int n = blockIdx.y, H = a.h, W = a.w, chunks = (W + N - 1) / N, units = H * chunks;
    const da_row r = da_load_row(a.plan + (size_t)n * 8, H, W);
    const T* __restrict__ s = da_sample<T>(a, n);
    float acc = 0.f;
    for (int u = blockIdx.x * DA_THREADS + threadIdx.x; u < units; u += gridDim.x * DA_THREADS) {
        const int y = u / chunks, x0 = (u - y * chunks) * N;
        float v[3 * N];
        da_gather<T>(s, H, W, y, x0, a.vec, v);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int x = x0 + j;
            bool keep = true;                                    // (columns past the row read as zeros)
            if (BWD) {
                const int qy = y - r.ty, qx = x - r.tx;
                keep = !da_in_box(r, y, x) && qy >= 0 && qy < H && qx >= 0 && qx < W;
            }
            if (keep) acc += (v[3 * j] + v[3 * j + 1]) + v[3 * j + 2];
        }
    }
    acc = wave_sum(acc);
    __shared__ float red[DA_THREADS / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.part[(size_t)n * a.nparts + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (x, n): a unit is N pixels of one output row, 48 bytes in and out
template <typename T, bool BWD> __global__ __launch_bounds__(DA_THREADS) void da_apply_kernel(da_args a) {
    constexpr int N = Vec<T>::N;
    const int n = blockIdx.y, H = a.h, W = a.w, chunks = (W + N - 1) / N, units = H * chunks;
    const da_row r = da_load_row(a.plan + (size_t)n * 8, H, W);
    const bool bright = a.flags & 1, sat = a.flags & 2, con = a.flags & 4;
    float mean = 0.f;
    if (con) {                                                   // (uniform: every lane of every wave is here)
        const int lane = threadIdx.x & 63;
        const float p = lane < a.nparts ? a.part[(size_t)n * a.nparts + lane] : 0.f;
        mean = wave_sum(p) / (float)((size_t)H * W * 3);
        if (!BWD && bright) mean += r.b;                         // mean(u) = mean(x) + b: saturation keeps a pixel's channel mean
    }
    const T* __restrict__ s = da_sample<T>(a, n);
    T* __restrict__ o = static_cast<T*>(a.out) + (size_t)n * H * W * 3;
    const float third = 1.f / 3.f;
    for (int u = blockIdx.x * DA_THREADS + threadIdx.x; u < units; u += gridDim.x * DA_THREADS) {
        const int y = u / chunks, x0 = (u - y * chunks) * N;
        // forward: y[p] = u[p - t]; backward: h[q] = g[q + t]
        const int sy = BWD ? y + r.ty : y - r.ty, sx0 = BWD ? x0 + r.tx : x0 - r.tx;
        float v[3 * N];
        da_gather<T>(s, H, W, sy, sx0, a.vec, v);
        const bool rowok = sy >= 0 && sy < H;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int x = x0 + j, sx = sx0 + j;
            // the box is a set of pixels of the AUGMENTED image: the output pixel going forward, the source pixel going back
            const bool keep = rowok && sx >= 0 && sx < W && !(BWD ? da_in_box(r, sy, sx) : da_in_box(r, y, x));
            float c0 = v[3 * j], c1 = v[3 * j + 1], c2 = v[3 * j + 2];
            if (!BWD) {
                if (bright) c0 += r.b, c1 += r.b, c2 += r.b;
                if (sat) {
                    const float m = ((c0 + c1) + c2) * third;
                    c0 = fmaf(c0 - m, r.s, m), c1 = fmaf(c1 - m, r.s, m), c2 = fmaf(c2 - m, r.s, m);
                }
                if (con) c0 = fmaf(c0 - mean, r.k, mean), c1 = fmaf(c1 - mean, r.k, mean), c2 = fmaf(c2 - mean, r.k, mean);
                if (!keep) c0 = c1 = c2 = 0.f;
            } else {
                if (!keep) c0 = c1 = c2 = 0.f;
                if (con) {
                    const float add = (1.f - r.k) * mean;
                    c0 = fmaf(r.k, c0, add), c1 = fmaf(r.k, c1, add), c2 = fmaf(r.k, c2, add);
                }
                if (sat) {
                    const float add = (1.f - r.s) * (((c0 + c1) + c2) * third);
                    c0 = fmaf(r.s, c0, add), c1 = fmaf(r.s, c1, add), c2 = fmaf(r.s, c2, add);
                }
            }
            v[3 * j] = c0, v[3 * j + 1] = c1, v[3 * j + 2] = c2;
        }
        T* __restrict__ orow = o + (size_t)y * (3 * W) + 3 * x0;
        if (a.vec) {                                             // (W % N == 0: every unit is whole)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                Vec<T> q;
                q.set(v + i * N);
                q.store(orow + i * N);
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (x0 + j < W) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) orow[3 * j + c] = from_f<T>(v[3 * j + c]);
                }
        }
    }
}

bool da_aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

int da_plan_check(const float* ph, int rows, int h, int w) {
    XMC_REQUIRE(ph != nullptr);
    for (int i = 0; i < rows; ++i) {
        const float* p = ph + (size_t)i * 8;
        for (int k = 0; k < 8; ++k) XMC_REQUIRE(std::isfinite(p[k]));
        XMC_REQUIRE(fabsf(p[3]) < (float)h && fabsf(p[4]) < (float)w && p[7] >= 0.f);
    }
    return XMC_OK;
}

int da_units(int h, int w, int n_vec) { return h * ((w + n_vec - 1) / n_vec); }

int da_parts(int units) {
    const int per = DA_THREADS * DA_UNITS_PER_THREAD;
    const int g = (units + per - 1) / per;
    return g < 1 ? 1 : (g > DA_MAX_PARTS ? DA_MAX_PARTS : g);
}

template <typename T, bool BWD> int da_launch(da_args a, int n, hipStream_t stream) {
    const int units = da_units(a.h, a.w, Vec<T>::N);
    a.vec = a.vec && (a.w % Vec<T>::N) == 0;
    a.nparts = da_parts(units);
    if (a.flags & 4) {
        hipLaunchKernelGGL((da_reduce_kernel<T, BWD>), dim3((unsigned)a.nparts, (unsigned)n), dim3(DA_THREADS), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return xmc_hip_err(e);
    }
    int gx = (units + DA_THREADS - 1) / DA_THREADS;
    const int cap = DA_MAX_BLOCKS / n > 0 ? DA_MAX_BLOCKS / n : 1;
    gx = gx < cap ? gx : cap;
    hipLaunchKernelGGL((da_apply_kernel<T, BWD>), dim3((unsigned)gx, (unsigned)n), dim3(DA_THREADS), 0, stream, a);
    XMC_LAUNCH_RET();
}

int da_common_check(int32_t b, int32_t h, int32_t w, int32_t flags, int32_t dtype) {
    XMC_REQUIRE(b >= 1 && 2 * (int64_t)b <= 65535 && h >= 1 && w >= 1 && h <= DA_MAX_SIDE && w <= DA_MAX_SIDE);
    XMC_REQUIRE((int64_t)h * w * 3 < (1LL << 31));               // per-sample offsets are ints; sample bases are 64-bit
    XMC_REQUIRE(flags >= 0 && flags <= 7 && (dtype == XMC_F32 || dtype == XMC_BF16));
    return XMC_OK;
}

}  // namespace

extern "C" int64_t xmc_diffaug_workspace_bytes(int32_t b, int32_t h, int32_t w) {
    if (da_common_check(b, h, w, 0, XMC_F32) != XMC_OK) return XMC_EINVAL;
    return (int64_t)2 * b * DA_MAX_PARTS * (int64_t)sizeof(float);
}

extern "C" int xmc_diffaug_fwd(const void* real, const void* fake, const float* plan, const float* plan_host, void* out, int32_t b,
                               int32_t h, int32_t w, int32_t flags, int32_t dtype, void* workspace, void* stream) {
    XMC_REQUIRE(real && fake && plan && plan_host && out);
    XMC_REQUIRE(da_common_check(b, h, w, flags, dtype) == XMC_OK);
    XMC_REQUIRE(!(flags & 4) || (workspace && da_aligned(workspace, 4)));
    const size_t el = dtype == XMC_F32 ? 4 : 2;
    XMC_REQUIRE(da_aligned(real, el) && da_aligned(fake, el) && da_aligned(out, el) && da_aligned(plan, 4));
    XMC_REQUIRE(da_plan_check(plan_host, 2 * b, h, w) == XMC_OK);
    da_args a;
    a.src0 = real, a.src1 = fake, a.plan = plan, a.out = out, a.part = static_cast<float*>(workspace);
    a.n0 = b, a.h = h, a.w = w, a.nparts = 1, a.flags = flags;
    a.vec = da_aligned(real, 16) && da_aligned(fake, 16) && da_aligned(out, 16);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == XMC_F32 ? da_launch<float, false>(a, 2 * b, st) : da_launch<bf16_t, false>(a, 2 * b, st);
}

extern "C" int xmc_diffaug_bwd(const void* g, const float* plan, const float* plan_host, void* dimg, int32_t b, int32_t h, int32_t w,
                               int32_t flags, int32_t dtype, void* workspace, void* stream) {
    XMC_REQUIRE(g && plan && plan_host && dimg && g != dimg);
    XMC_REQUIRE(da_common_check(b, h, w, flags, dtype) == XMC_OK);
    XMC_REQUIRE(!(flags & 4) || (workspace && da_aligned(workspace, 4)));
    const size_t el = dtype == XMC_F32 ? 4 : 2;
    XMC_REQUIRE(da_aligned(g, el) && da_aligned(dimg, el) && da_aligned(plan, 4));
    XMC_REQUIRE(da_plan_check(plan_host, b, h, w) == XMC_OK);
    da_args a;
    a.src0 = g, a.src1 = nullptr, a.plan = plan, a.out = dimg, a.part = static_cast<float*>(workspace);
    a.n0 = b, a.h = h, a.w = w, a.nparts = 1, a.flags = flags;
    a.vec = da_aligned(g, 16) && da_aligned(dimg, 16);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == XMC_F32 ? da_launch<float, true>(a, b, st) : da_launch<bf16_t, true>(a, b, st);
}
