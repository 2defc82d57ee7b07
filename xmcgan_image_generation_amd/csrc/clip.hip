// CLIP dual encoder (transformers.CLIPModel layout: ViT image tower + causal text tower, pre-LN blocks, QuickGELU) and the two
// text-image alignment scores built on it (utils/clip_utils.py, utils/alignment_metrics.py): every kernel that is not a dense
// product.  Activations are float32 [rows = n * t][h]; the dense layers run on xmc_gemm_f32 / xmc_gemm_f32_bf16mfma and their
// biases are added HERE, by the kernel that consumes the product.
//
//   xmc_clip_preprocess    (n, H, W, 3) in [0, 1] -> cubic resize to S x S, (v - mean) / std, patch rows (c, ky, kx)   one workgroup per output row
//   xmc_clip_vision_embed  y[i, j] = LN((j ? patch[i, j - 1] : cls) + pos[j])                                       one wave per row
//   xmc_clip_text_embed    x[r] = tok[ids[r]] + pos[r mod t]                                                          one wave per row
//   xmc_bias_add_ln        s = x + bias + res,  y = LN(s) * gamma + beta                                              one wave per row
//   xmc_bias_quick_gelu    y = v sigmoid(1.702 v), v = x + bias                                                        16 bytes per lane
//   xmc_mha_attention      ctx = softmax_{j < len [, j <= i]}((q + b_q)(k + b_k)^T / 8)(v + b_v), t <= 128              one workgroup per (sequence, head)
//   xmc_gather_rows_ln     y[i] = LN(x[i t + idx[i]]) * gamma + beta                                                   one wave per row
//   xmc_pair_cosine        cos[i] = a[i].b[i] / (|a[i]| |b[i]|), float64                                                one wave per row
//   xmc_rprecision_hits    hit[i] = cos(img[i], txt[truth[i]]) > cos(img[i], txt[cand[i, j]]) for every j              one wave per image
//
// The row kernels hold the whole row in registers (16 bytes per lane per access, h <= 1024) and take the variance as
// mean((v - mean)^2) of the held values, as bert.hip does.  float32 arithmetic throughout (float64 in the two cosine kernels and
// inside QuickGELU), every cross-lane reduction a fixed xor tree, no atomics: two launches on the same inputs give the same bits,
// and no sequence's result depends on what shares its launch.
#include "common.h"
#include "clip_taps.h"

namespace {

constexpr int LN_MAXV = 4;     // float4 per lane: rows of up to 64 * 4 * 4 = 1024 floats
constexpr int DH = 64;         // head dimension
constexpr int KP = 68;         // LDS pitch of the k / v rows: 16-byte aligned, 16 rows cover the 64 banks once (ds_read_b128)
constexpr int MHA_MAX_T = 128;
constexpr int PRE_MIN_HW = 32, PRE_MAX_HW = 512, PRE_MAX_S = 448;

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// v = a + b + c over one row (b, c may be NULL: wave-uniform), held by the wave; columns >= H hold zeros
__device__ __forceinline__ void row_load(float4 (&v)[LN_MAXV], const float* a, const float* b, const float* c, int H, int lane) {
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < H) {
            v[j] = *reinterpret_cast<const float4*>(a + col);
            if (b) v[j] = add4(v[j], *reinterpret_cast<const float4*>(b + col));
            if (c) v[j] = add4(v[j], *reinterpret_cast<const float4*>(c + col));
        }
    }
}

__device__ __forceinline__ void row_store(const float4 (&v)[LN_MAXV], float* y, int H, int lane) {
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        if (col < H) *reinterpret_cast<float4*>(y + col) = v[j];
    }
}

// y = (v - mean) / sqrt(var + eps) * gamma + beta; two passes over the registers
__device__ __forceinline__ void row_ln_store(float4 (&v)[LN_MAXV], const float* __restrict__ gamma, const float* __restrict__ beta,
                                             float* y, int H, int lane, float eps) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);          // (columns >= H hold zeros)
    const float inv_h = 1.f / (float)H;
    const float mean = wave_sum(s) * inv_h;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        if (col < H) {
            v[j] = make_float4(v[j].x - mean, v[j].y - mean, v[j].z - mean, v[j].w - mean);
            q = fmaf(v[j].x, v[j].x, q); q = fmaf(v[j].y, v[j].y, q);
            q = fmaf(v[j].z, v[j].z, q); q = fmaf(v[j].w, v[j].w, q);
        }
    }
    const float var = wave_sum(q) * inv_h;           // biased
    const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        if (col < H) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + col);
            const float4 be = *reinterpret_cast<const float4*>(beta + col);
            *reinterpret_cast<float4*>(y + col) = make_float4(fmaf(v[j].x * rstd, g.x, be.x), fmaf(v[j].y * rstd, g.y, be.y),
                                                              fmaf(v[j].z * rstd, g.z, be.z), fmaf(v[j].w * rstd, g.w, be.w));
        }
    }
}

enum { ROW_VISION = 0, ROW_TEXT = 1, ROW_ADD_LN = 2, ROW_GATHER_LN = 3 };

struct RowArgs {
    const float* x;  const float* bias;  const float* res;      // ROW_ADD_LN (bias, res may be NULL); x: ROW_GATHER_LN
    const float* patch;  const float* cls;  const float* pos;    // ROW_VISION; pos: ROW_TEXT too
    const float* tok;  const int32_t* ids;                       // ROW_TEXT; ids: the row index of ROW_GATHER_LN (may be NULL: 0)
    const float* gamma;  const float* beta;
    float* s;  float* y;                                         // s: ROW_ADD_LN's sum (may be NULL)
    int rows, T, H, V;
    float eps;
};

template <int MODE>
__global__ __launch_bounds__(256) void clip_row_kernel(const RowArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= p.rows) return;                       // wave-uniform; no barrier in this kernel
    const int H = p.H;
    float4 v[LN_MAXV];
    if constexpr (MODE == ROW_VISION) {
        const int i = row / p.T, j = row - i * p.T;
        const float* a = j ? p.patch + ((size_t)i * (p.T - 1) + (j - 1)) * H : p.cls;
        row_load(v, a, p.pos + (size_t)j * H, nullptr, H, lane);
        row_ln_store(v, p.gamma, p.beta, p.y + (size_t)row * H, H, lane, p.eps);
    } else if constexpr (MODE == ROW_TEXT) {
        int id = p.ids[row];
        id = id < 0 ? 0 : (id >= p.V ? p.V - 1 : id);        // the host rejects such ids; the table is never read outside
        row_load(v, p.tok + (size_t)id * H, p.pos + (size_t)(row % p.T) * H, nullptr, H, lane);
        row_store(v, p.y + (size_t)row * H, H, lane);
    } else if constexpr (MODE == ROW_ADD_LN) {
        row_load(v, p.x + (size_t)row * H, p.bias, p.res ? p.res + (size_t)row * H : nullptr, H, lane);
        if (p.s) row_store(v, p.s + (size_t)row * H, H, lane);       // (s may be res: every lane has read what it overwrites)
        row_ln_store(v, p.gamma, p.beta, p.y + (size_t)row * H, H, lane, p.eps);
    } else {
        int j = p.ids ? p.ids[row] : 0;
        j = j < 0 ? 0 : (j >= p.T ? p.T - 1 : j);            // validated on the host copy; clamped into the sequence
        row_load(v, p.x + ((size_t)row * p.T + j) * H, nullptr, nullptr, H, lane);
        row_ln_store(v, p.gamma, p.beta, p.y + (size_t)row * H, H, lane, p.eps);
    }
}

// QuickGELU in DOUBLE, rounded once: v / (1 + exp(-1.702 v)); in float32 the product 1.702 v alone carries an error of
// 1.7 |v| u in the exponent (4e-6 relative at v = -40)
__device__ __forceinline__ float qgelu1(float x, float b) {
    const double v = (double)(x + b);
    return (float)(v / (1.0 + exp(-1.702 * v)));
}

// one workgroup per 256 float4 of one row (blockIdx.x = row * blocks-per-row + column block)
__global__ __launch_bounds__(256) void bias_quick_gelu_kernel(const float* x, const float* __restrict__ bias, float* y, int f4,
                                                              int bpr) {      // (y may be x: each lane reads its 16 bytes, then writes them)
    const int row = blockIdx.x / bpr;
    const int c = (blockIdx.x - row * bpr) * 256 + threadIdx.x;
    if (c >= f4) return;
    const size_t t = (size_t)row * f4 + c;
    const float4 a = reinterpret_cast<const float4*>(x)[t];
    const float4 b = reinterpret_cast<const float4*>(bias)[c];
    reinterpret_cast<float4*>(y)[t] = make_float4(qgelu1(a.x, b.x), qgelu1(a.y, b.y), qgelu1(a.z, b.z), qgelu1(a.w, b.w));
}

// 1 <= T <= 128: one 256-thread workgroup per (sequence, head).  LDS: the k and v rows [T][KP] with their biases added, then the
// probabilities [T][T + 1] (135,680 bytes at T = 128: one workgroup per CU; 37.4 KiB at the 50 tokens of ViT-B/32: four).  The
// query row of a wave stays in registers, one element per lane, and is broadcast with v_readlane.  A wave owns one query row per
// pass, lane j the keys j and j + 64; 16 lanes x 16 bytes finish one context row, 16 rows per pass.  Keys that are masked
// (j >= len, or j > i when causal) get probability exactly 0; the live ones are added in ascending order.
__global__ __launch_bounds__(256) void mha_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                           const int32_t* __restrict__ len, float* __restrict__ ctx, int T, int H,
                                                           int causal) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const K = lds;
    float* const V = K + T * KP;
    float* const P = V + T * KP;
    const int PPT = T + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int heads = H / DH;
    const int n = blockIdx.x / heads, hd = blockIdx.x - n * heads;
    int ml = len[n];
    ml = ml < 1 ? 1 : (ml > T ? T : ml);             // validated on the host copy; clamped so that no index can leave the tile
    const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;       // 16 rows per pass, 16 lanes x 16 bytes per row
    const float* const base = qkv + (size_t)n * T * (3 * (size_t)H) + hd * DH;

    {
        const float4 bk = *reinterpret_cast<const float4*>(bias + H + hd * DH + c4);
        const float4 bv = *reinterpret_cast<const float4*>(bias + 2 * H + hd * DH + c4);
        for (int t = r; t < T; t += 16) {
            const float* row = base + (size_t)t * (3 * (size_t)H) + c4;
            *reinterpret_cast<float4*>(K + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + H), bk);
            *reinterpret_cast<float4*>(V + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + 2 * H), bv);
        }
    }
    __syncthreads();

    {
        const int j0 = lane, j1 = lane + 64;
        const int jr0 = j0 < T ? j0 : T - 1, jr1 = j1 < T ? j1 : T - 1;
        const float bq = bias[hd * DH + lane];
        for (int i = wave; i < T; i += 4) {          // wave-uniform
            const int qi = __float_as_int(base[(size_t)i * (3 * (size_t)H) + lane] + bq);      // q[i][lane]
            const int lim = causal ? (i + 1 < ml ? i + 1 : ml) : ml;                           // keys j < lim are live (lim >= 1)
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const float q0 = __int_as_float(__builtin_amdgcn_readlane(qi, d)), q1 = __int_as_float(__builtin_amdgcn_readlane(qi, d + 1));
                const float q2 = __int_as_float(__builtin_amdgcn_readlane(qi, d + 2)), q3 = __int_as_float(__builtin_amdgcn_readlane(qi, d + 3));
                const float4 ka = *reinterpret_cast<const float4*>(K + jr0 * KP + d);
                const float4 kb = *reinterpret_cast<const float4*>(K + jr1 * KP + d);
                s0 = fmaf(q0, ka.x, s0); s0 = fmaf(q1, ka.y, s0); s0 = fmaf(q2, ka.z, s0); s0 = fmaf(q3, ka.w, s0);
                s1 = fmaf(q0, kb.x, s1); s1 = fmaf(q1, kb.y, s1); s1 = fmaf(q2, kb.z, s1); s1 = fmaf(q3, kb.w, s1);
            }
            const bool live0 = j0 < lim, live1 = j1 < lim;
            s0 = live0 ? s0 * 0.125f : -INFINITY;
            s1 = live1 ? s1 * 0.125f : -INFINITY;
            const float m = wave_max(fmaxf(s0, s1));                 // key 0 is always live: m is finite
            const float e0 = live0 ? expf(s0 - m) : 0.f, e1 = live1 ? expf(s1 - m) : 0.f;
            const float sum = wave_sum(e0 + e1);
            if (j0 < T) P[i * PPT + j0] = e0 / sum;
            if (j1 < T) P[i * PPT + j1] = e1 / sum;
        }
    }
    __syncthreads();

    for (int i = r; i < T; i += 16) {                // ctx[i][d] = sum over the live keys of p[i][j] v[j][d], j ascending
        const int lim = causal ? (i + 1 < ml ? i + 1 : ml) : ml;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < lim; ++j) {
            const float pj = P[i * PPT + j];
            const float4 vv = *reinterpret_cast<const float4*>(V + j * KP + c4);
            acc.x = fmaf(pj, vv.x, acc.x); acc.y = fmaf(pj, vv.y, acc.y);
            acc.z = fmaf(pj, vv.z, acc.z); acc.w = fmaf(pj, vv.w, acc.w);
        }
        *reinterpret_cast<float4*>(ctx + ((size_t)n * T + i) * H + hd * DH + c4) = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------ preprocessing
template <typename T> __device__ __forceinline__ float px(const T* p, size_t i);
template <> __device__ __forceinline__ float px<float>(const float* p, size_t i) { return p[i]; }
template <> __device__ __forceinline__ float px<bf16_t>(const bf16_t* p, size_t i) { return bf2f(p[i]); }

struct PreArgs {
    const void* x;  float* y;
    int n, hw, S, P, ksize;
    float mean[3], rstd[3];
};

// one workgroup per (image, output row oy).  LDS: the horizontal taps of every output column [S][ksize] with their window starts and
// counts, the vertical taps of this row, and the vertically resampled input row [hw][3].  The vertical pass runs first (rows of
// the input are read once, coalesced), the horizontal one from LDS; both in float32, taps in ascending order.
template <typename T>
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const PreArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = p.S, hw = p.hw, ks = p.ksize;
    float* const wx = lds;                                           // [S][ks]
    float* const wy = wx + S * ks;                                   // [ks]
    float* const tmp = wy + ks;                                      // [hw * 3]
    int* const xlo = reinterpret_cast<int*>(tmp + hw * 3);           // [S]
    int* const xcnt = xlo + S;                                       // [S]
    int* const yinfo = xcnt + S;                                     // [2]
    const int img = blockIdx.x / S, oy = blockIdx.x - img * S;
    const int tid = threadIdx.x;

    for (int ox = tid; ox < S; ox += 256) {
        int lo;
        xcnt[ox] = cubic_taps(ox, hw, S, ks, wx + ox * ks, &lo);
        xlo[ox] = lo;
    }
    if (tid == 0) {
        int lo;
        yinfo[1] = cubic_taps(oy, hw, S, ks, wy, &lo);
        yinfo[0] = lo;
    }
    __syncthreads();

    const int ylo = yinfo[0], ycnt = yinfo[1];                       // ylo + ycnt <= hw
    const T* const src = static_cast<const T*>(p.x) + (size_t)img * hw * hw * 3;
    for (int e = tid; e < hw * 3; e += 256) {                        // element e of an input row: (x, c) interleaved, contiguous
        float acc = 0.f;
        for (int k = 0; k < ycnt; ++k) acc = fmaf(wy[k], px<T>(src, (size_t)(ylo + k) * hw * 3 + e), acc);
        tmp[e] = acc;
    }
    __syncthreads();

    const int G = S / p.P, PP2 = p.P * p.P;
    const int gy = oy / p.P, ky = oy - gy * p.P;
    for (int e = tid; e < S * 3; e += 256) {
        const int c = e / S, ox = e - c * S;                         // a run of lanes shares c: contiguous kx in the patch row
        const int lo = xlo[ox], cnt = xcnt[ox];                      // lo + cnt <= hw
        float acc = 0.f;
        for (int k = 0; k < cnt; ++k) acc = fmaf(wx[ox * ks + k], tmp[(lo + k) * 3 + c], acc);
        const int gx = ox / p.P, kx = ox - gx * p.P;
        p.y[((size_t)img * G * G + (size_t)gy * G + gx) * (3 * PP2) + c * PP2 + ky * p.P + kx] = (acc - p.mean[c]) * p.rstd[c];
    }
}

// --------------------------------------------------------------------------------------------------------------- the scores
// cos(a, b) in float64: lane l adds the products of elements l, l + 64, ... in index order (float32 values multiplied in float64),
// then a fixed xor tree; every lane returns the same value.  A zero row gives 0.
__device__ __forceinline__ double wave_cosine(const float* __restrict__ a, const float* __restrict__ b, int d, int lane) {
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int i = lane; i < d; i += 64) {
        const double x = (double)a[i], y = (double)b[i];
        ab = fma(x, y, ab); aa = fma(x, x, aa); bb = fma(y, y, bb);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ab += __shfl_xor(ab, o); aa += __shfl_xor(aa, o); bb += __shfl_xor(bb, o);
    }
    const double den = sqrt(aa) * sqrt(bb);
    return den > 0.0 ? ab / den : 0.0;
}

__global__ __launch_bounds__(256) void pair_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int d,
                                                         double* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;                                            // whole waves leave
    const double c = wave_cosine(a + (size_t)row * d, b + (size_t)row * d, d, lane);
    if (lane == 0) out[row] = c;
}

__global__ __launch_bounds__(256) void rprecision_hits_kernel(const float* __restrict__ img, const float* __restrict__ txt,
                                                             const int32_t* __restrict__ truth, const int32_t* __restrict__ cand,
                                                             int n, int m, int d, int c, uint8_t* __restrict__ hit) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    auto clampm = [m](int v) { return v < 0 ? 0 : (v >= m ? m - 1 : v); };      // validated on the host copy
    const float* const a = img + (size_t)row * d;
    const double own = wave_cosine(a, txt + (size_t)clampm(truth[row]) * d, d, lane);
    bool ok = true;
    for (int j = 0; j < c; ++j) {                                    // wave-uniform: every lane holds the same cosines
        const double other = wave_cosine(a, txt + (size_t)clampm(cand[(size_t)row * c + j]) * d, d, lane);
        ok = ok && own > other;                                      // STRICTLY greater: a duplicate of the true caption is a miss
    }
    if (lane == 0) hit[row] = ok ? 1 : 0;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
inline bool ln_row_ok(int h) { return h > 0 && h % 4 == 0 && h <= 64 * 4 * LN_MAXV; }
inline unsigned row_blocks(int rows) { return (unsigned)((rows + 3) / 4); }
inline int pre_ksize(int hw, int S) {
    const double scale = (double)hw / (double)S;
    return (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
inline size_t mha_lds(int t) { return (size_t)(2 * t * KP + t * (t + 1)) * sizeof(float); }

}  // namespace

extern "C" int xmc_clip_preprocess(const void* images, float* patches, int32_t n, int32_t hw, int32_t s, int32_t p, const float* mean3,
                                   const float* std3, int32_t dtype, void* stream) {
    XMC_REQUIRE(images && patches && mean3 && std3);
    XMC_REQUIRE(dtype == XMC_F32 || dtype == XMC_BF16);
    XMC_REQUIRE(n > 0 && hw >= PRE_MIN_HW && hw <= PRE_MAX_HW && p > 0 && s >= p && s <= PRE_MAX_S && s % p == 0);
    XMC_REQUIRE((long long)n * s < (1ll << 31));
    XMC_REQUIRE(aligned16(images) && aligned16(patches));
    PreArgs a{};
    a.x = images; a.y = patches; a.n = n; a.hw = hw; a.S = s; a.P = p; a.ksize = pre_ksize(hw, s);
    for (int c = 0; c < 3; ++c) {
        XMC_REQUIRE(std3[c] > 0.f && std3[c] == std3[c] && mean3[c] == mean3[c]);      // host arrays, passed to the kernel by value
        a.mean[c] = mean3[c]; a.rstd[c] = 1.f / std3[c];
    }
    const size_t lds = ((size_t)s * a.ksize + a.ksize + (size_t)hw * 3) * sizeof(float) + ((size_t)2 * s + 2) * sizeof(int);
    XMC_REQUIRE(lds <= 64 * 1024);                                   // (<= 26.7 KiB over the whole domain)
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == XMC_F32) hipLaunchKernelGGL(clip_preprocess_kernel<float>, dim3((unsigned)(n * s)), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(clip_preprocess_kernel<bf16_t>, dim3((unsigned)(n * s)), dim3(256), lds, st, a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_clip_vision_embed(const float* patch, const float* cls, const float* pos, const float* gamma, const float* beta,
                                     float* y, int32_t n, int32_t t, int32_t h, float eps, void* stream) {
    XMC_REQUIRE(patch && cls && pos && gamma && beta && y);
    XMC_REQUIRE(n > 0 && t >= 2 && ln_row_ok(h) && eps >= 0.f && (long long)n * t < (1ll << 31));
    XMC_REQUIRE(aligned16(patch) && aligned16(cls) && aligned16(pos) && aligned16(gamma) && aligned16(beta) && aligned16(y));
    RowArgs a{};
    a.patch = patch; a.cls = cls; a.pos = pos; a.gamma = gamma; a.beta = beta; a.y = y;
    a.rows = n * t; a.T = t; a.H = h; a.V = 1; a.eps = eps;
    hipLaunchKernelGGL(clip_row_kernel<ROW_VISION>, dim3(row_blocks(a.rows)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_clip_text_embed(const int32_t* ids, const float* tok, const float* pos, float* x, int32_t rows, int32_t t,
                                   int32_t h, int32_t vocab, int32_t npos, void* stream) {
    XMC_REQUIRE(ids && tok && pos && x);
    XMC_REQUIRE(rows > 0 && t > 0 && t <= npos && vocab > 0 && ln_row_ok(h));
    XMC_REQUIRE(aligned16(tok) && aligned16(pos) && aligned16(x));
    RowArgs a{};
    a.ids = ids; a.tok = tok; a.pos = pos; a.y = x;
    a.rows = rows; a.T = t; a.H = h; a.V = vocab;
    hipLaunchKernelGGL(clip_row_kernel<ROW_TEXT>, dim3(row_blocks(rows)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bias_add_ln(const float* x, const float* bias, const float* res, const float* gamma, const float* beta, float* s,
                               float* y, int32_t rows, int32_t h, float eps, void* stream) {
    XMC_REQUIRE(x && gamma && beta && y);
    XMC_REQUIRE(rows > 0 && ln_row_ok(h) && eps >= 0.f);
    XMC_REQUIRE(aligned16(x) && aligned16(bias) && aligned16(res) && aligned16(gamma) && aligned16(beta) && aligned16(s) && aligned16(y));
    XMC_REQUIRE(y != s);                                             // (s == res, y == x are fine: a lane overwrites what it has read)
    RowArgs a{};
    a.x = x; a.bias = bias; a.res = res; a.gamma = gamma; a.beta = beta; a.s = s; a.y = y;
    a.rows = rows; a.T = 1; a.H = h; a.V = 1; a.eps = eps;
    hipLaunchKernelGGL(clip_row_kernel<ROW_ADD_LN>, dim3(row_blocks(rows)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bias_quick_gelu(const float* x, const float* bias, float* y, int32_t rows, int32_t f, void* stream) {
    XMC_REQUIRE(x && bias && y && rows > 0 && f > 0 && f % 4 == 0);
    XMC_REQUIRE(aligned16(x) && aligned16(bias) && aligned16(y));
    const int f4 = f / 4, bpr = (f4 + 255) / 256;
    XMC_REQUIRE((long long)rows * bpr < (1ll << 31));
    hipLaunchKernelGGL(bias_quick_gelu_kernel, dim3((unsigned)(rows * bpr)), dim3(256), 0, static_cast<hipStream_t>(stream), x, bias,
                       y, f4, bpr);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_mha_attention(const float* qkv, const float* bias_qkv, const int32_t* len, const int32_t* len_host, float* ctx,
                                 int32_t n, int32_t t, int32_t h, int32_t causal, void* stream) {
    XMC_REQUIRE(qkv && bias_qkv && len && len_host && ctx);
    XMC_REQUIRE(n > 0 && t >= 1 && t <= MHA_MAX_T && h >= DH && h % DH == 0);
    XMC_REQUIRE((long long)n * (h / DH) < (1ll << 31));
    XMC_REQUIRE(aligned16(qkv) && aligned16(bias_qkv) && aligned16(ctx));
    for (int i = 0; i < n; ++i) XMC_REQUIRE(len_host[i] >= 1 && len_host[i] <= t);
    static XmcLdsOptIn opt_in;                                       // 135,680 bytes at t = 128: above the 64 KiB default
    if (!opt_in.ensure({reinterpret_cast<const void*>(&mha_attention_kernel)}, (int)mha_lds(MHA_MAX_T))) return XMC_EINVAL;
    hipLaunchKernelGGL(mha_attention_kernel, dim3((unsigned)(n * (h / DH))), dim3(256), mha_lds(t), static_cast<hipStream_t>(stream),
                       qkv, bias_qkv, len, ctx, t, h, causal != 0);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_gather_rows_ln(const float* x, const int32_t* idx, const int32_t* idx_host, const float* gamma, const float* beta,
                                  float* y, int32_t n, int32_t t, int32_t h, float eps, void* stream) {
    XMC_REQUIRE(x && gamma && beta && y && (idx == nullptr) == (idx_host == nullptr));
    XMC_REQUIRE(n > 0 && t > 0 && ln_row_ok(h) && eps >= 0.f);
    XMC_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(y));
    if (idx_host)
        for (int i = 0; i < n; ++i) XMC_REQUIRE(idx_host[i] >= 0 && idx_host[i] < t);
    RowArgs a{};
    a.x = x; a.ids = idx; a.gamma = gamma; a.beta = beta; a.y = y;
    a.rows = n; a.T = t; a.H = h; a.V = 1; a.eps = eps;
    hipLaunchKernelGGL(clip_row_kernel<ROW_GATHER_LN>, dim3(row_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_pair_cosine(const float* a, const float* b, double* cos, int32_t n, int32_t d, void* stream) {
    XMC_REQUIRE(a && b && cos && n > 0 && d > 0);
    XMC_REQUIRE(aligned16(a) && aligned16(b) && aligned16(cos));
    hipLaunchKernelGGL(pair_cosine_kernel, dim3(row_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, n, d, cos);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_rprecision_hits(const float* img, const float* txt, const int32_t* truth, const int32_t* truth_host,
                                   const int32_t* cand, const int32_t* cand_host, uint8_t* hit, int32_t n, int32_t m, int32_t d,
                                   int32_t c, void* stream) {
    XMC_REQUIRE(img && txt && truth && truth_host && cand && cand_host && hit);
    XMC_REQUIRE(n > 0 && m > 0 && d > 0 && c > 0);
    XMC_REQUIRE(aligned16(img) && aligned16(txt) && aligned16(hit));
    for (int i = 0; i < n; ++i) XMC_REQUIRE(truth_host[i] >= 0 && truth_host[i] < m);
    for (long long i = 0; i < (long long)n * c; ++i) XMC_REQUIRE(cand_host[i] >= 0 && cand_host[i] < m);
    hipLaunchKernelGGL(rprecision_hits_kernel, dim3(row_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), img, txt, truth,
                       cand, n, m, d, c, hit);
    XMC_LAUNCH_RET();
}
