// BERT-base caption encoder (preprocess_data.py:36-58, get_bert_for_captions): every kernel of the frozen text network that is
// not a dense product.  Activations are float32 [rows = N * T][.]; all T positions of every caption are computed, padding
// included (the reference's sentence embedding sums over them and caption/embedding stores them).  The dense layers run on
// xmc_gemm_f32 / xmc_gemm_f32_bf16mfma (gemm_f32.hip); their biases are added HERE, by the kernel that consumes the product.
//
//   xmc_bert_embed_ln     y[r] = LN(word[ids[r]] + pos[r mod T] + type[0])           one wave per row
//   xmc_bias_residual_ln  y[r] = LN(x[r] + bias + res[r]) * gamma + beta             one wave per row
//   xmc_bias_gelu         y = 0.5 v (1 + erf(v / sqrt 2)), v = x + bias              16 bytes per lane
//   xmc_bert_attention    ctx = softmax_{j < max_len}((q + b_q)(k + b_k)^T / 8)(v + b_v)   one wave per (caption, head)
//   xmc_bert_attention_long  the same for 2 <= T <= 64                                  one workgroup per (caption, head)
//   xmc_bert_sentence     out[n] = sum_{t < T} emb[n][t] / max_len[n]                fixed order
//
// The row kernels hold the whole row in registers (16 bytes per lane per access, H <= 1024): the mean, then the variance as
// mean((v - mean)^2) of the held values -- two passes over registers, one over memory.  LayerNorm's eps is 1e-12 here, so the
// one-pass E[v^2] - mean^2 returns variance 0 (or less) for a near-constant row and the row explodes; the two-pass form does not.
// Nothing in this file depends on which rows share a launch: a caption's result is the same alone and inside any chunk.
#include "common.h"

namespace {

constexpr int LN_MAXV = 4;     // float4 per lane: rows of up to 64 * 4 * 4 = 1024 floats
constexpr int DH = 64;         // head dimension
constexpr int KP = 68;         // LDS pitch of the q / k / v rows: 16-byte aligned, 16 rows cover the 64 banks once (ds_read_b128)
constexpr int PP = 33;         // LDS pitch of the probabilities
constexpr int ATT_MAX_T = 32;
constexpr int PP_LONG = 65;    // LDS pitch of the probabilities, T <= 64
constexpr int ATT_MAX_T_LONG = 64;

struct RowLnArgs {
    const int32_t* ids; const float* word; const float* pos; const float* type;      // EMBED
    const float* x; const float* bias; const float* res;                             // !EMBED
    const float* gamma; const float* beta; float* y;
    int rows, T, H, V;
    float eps;
};

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <bool EMBED>
__global__ __launch_bounds__(256) void row_ln_kernel(const RowLnArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= p.rows) return;                       // wave-uniform; no barrier in this kernel
    const int H = p.H;
    const float* a;
    const float* b;
    const float* c;
    if constexpr (EMBED) {
        int id = p.ids[row];
        id = id < 0 ? 0 : (id >= p.V ? p.V - 1 : id);        // the host rejects such ids; the table is never read outside
        a = p.word + (size_t)id * H;
        b = p.pos + (size_t)(row % p.T) * H;
        c = p.type;
    } else {
        a = p.x + (size_t)row * H;
        b = p.bias;
        c = p.res + (size_t)row * H;
    }
    float4 v[LN_MAXV];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < H) {
            v[j] = add4(add4(*reinterpret_cast<const float4*>(a + col), *reinterpret_cast<const float4*>(b + col)),
                        *reinterpret_cast<const float4*>(c + col));
            s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        }
    }
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
    const float rstd = 1.f / sqrtf(var + p.eps);
    float* y = p.y + (size_t)row * H;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        if (col < H) {
            const float4 g = *reinterpret_cast<const float4*>(p.gamma + col);
            const float4 be = *reinterpret_cast<const float4*>(p.beta + col);
            *reinterpret_cast<float4*>(y + col) = make_float4(fmaf(v[j].x * rstd, g.x, be.x), fmaf(v[j].y * rstd, g.y, be.y),
                                                              fmaf(v[j].z * rstd, g.z, be.z), fmaf(v[j].w * rstd, g.w, be.w));
        }
    }
}

// Exact-erf GELU in DOUBLE, rounded once: in float32, 1 + erf(x) cancels for x < 0 (gelu(-5) keeps 3 bits) and erfc(x)
// magnifies the rounding of v / sqrt 2 by 2 x^2; gfx950's float64 vector rate makes the exact form a few percent of a layer.
__device__ __forceinline__ float gelu1(float x, float b) {
    const double v = (double)(x + b);
    return (float)(0.5 * v * erfc(-v * 0.70710678118654752440));
}

// one workgroup per 256 float4 of one row (blockIdx.x = row * blocks-per-row + column block): no 64-bit index arithmetic per lane
__global__ __launch_bounds__(256) void bias_gelu_kernel(const float* x, const float* __restrict__ bias, float* y, int f4,
                                                        int bpr) {      // (y may be x: each lane reads its 16 bytes, then writes them)
    const int row = blockIdx.x / bpr;
    const int c = (blockIdx.x - row * bpr) * 256 + threadIdx.x;
    if (c >= f4) return;
    const size_t t = (size_t)row * f4 + c;
    const float4 a = reinterpret_cast<const float4*>(x)[t];
    const float4 b = reinterpret_cast<const float4*>(bias)[c];
    reinterpret_cast<float4*>(y)[t] = make_float4(gelu1(a.x, b.x), gelu1(a.y, b.y), gelu1(a.z, b.z), gelu1(a.w, b.w));
}

// one wave per (caption, head).  LDS: q, k, v rows [T][KP] with their biases added, then the probabilities [T][PP]; no T x T
// matrix leaves the CU.  Keys j >= max_len get probability 0 exactly (in float32 exp(-10000 + s - m) is 0 too).
__global__ __launch_bounds__(64) void bert_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                            const int32_t* __restrict__ max_len, float* __restrict__ ctx, int T,
                                                            int H) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const Q = lds;
    float* const K = Q + T * KP;
    float* const V = K + T * KP;
    float* const P = V + T * KP;
    const int lane = threadIdx.x;
    const int heads = H / DH;
    const int n = blockIdx.x / heads, hd = blockIdx.x - n * heads;
    int ml = max_len[n];
    ml = ml < 1 ? 1 : (ml > T ? T : ml);             // validated on the host copy; clamped so that no index can leave the tile

    {   // 16 lanes x 16 bytes per 64-float head row, four rows per pass
        const int r = lane >> 4, c4 = (lane & 15) * 4;
        const float4 bq = *reinterpret_cast<const float4*>(bias + hd * DH + c4);
        const float4 bk = *reinterpret_cast<const float4*>(bias + H + hd * DH + c4);
        const float4 bv = *reinterpret_cast<const float4*>(bias + 2 * H + hd * DH + c4);
        for (int t0 = 0; t0 < T; t0 += 4) {
            const int t = t0 + r;
            if (t < T) {
                const float* row = qkv + ((size_t)n * T + t) * (3 * (size_t)H) + hd * DH + c4;
                *reinterpret_cast<float4*>(Q + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row), bq);
                *reinterpret_cast<float4*>(K + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + H), bk);
                *reinterpret_cast<float4*>(V + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + 2 * H), bv);
            }
        }
    }
    __syncthreads();

    {   // scores and softmax: each 32-lane half owns one query row per pass, lane j of the half owns key j
        const int half = lane >> 5, j = lane & 31;
        const int jr = j < T ? j : T - 1;
        const bool live = j < ml;
        for (int i0 = 0; i0 < T; i0 += 2) {
            const int i = i0 + half;
            const int ir = i < T ? i : T - 1;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const float4 qv = *reinterpret_cast<const float4*>(Q + ir * KP + d);
                const float4 kv = *reinterpret_cast<const float4*>(K + jr * KP + d);
                s = fmaf(qv.x, kv.x, s); s = fmaf(qv.y, kv.y, s); s = fmaf(qv.z, kv.z, s); s = fmaf(qv.w, kv.w, s);
            }
            s = live ? s * 0.125f : -INFINITY;
            float m = s;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));      // stays inside the aligned 32-lane half
            const float e = live ? expf(s - m) : 0.f;
            float sum = e;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            if (i < T && j < T) P[i * PP + j] = e / sum;
        }
    }
    __syncthreads();

    {   // ctx[i][d] = sum_{j < max_len} p[i][j] v[j][d], j ascending: 16 lanes x 16 bytes per row, four query rows per pass
        const int r = lane >> 4, d4 = (lane & 15) * 4;
        for (int i = r; i < T; i += 4) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = 0; j < ml; ++j) {
                const float pj = P[i * PP + j];
                const float4 vv = *reinterpret_cast<const float4*>(V + j * KP + d4);
                acc.x = fmaf(pj, vv.x, acc.x); acc.y = fmaf(pj, vv.y, acc.y);
                acc.z = fmaf(pj, vv.z, acc.z); acc.w = fmaf(pj, vv.w, acc.w);
            }
            *reinterpret_cast<float4*>(ctx + ((size_t)n * T + i) * H + hd * DH + d4) = acc;
        }
    }
}

// 2 <= T <= 64 (Localized Narratives, 64-token captions): one 256-thread workgroup per (caption, head).  The same LDS image as
// above with the probabilities at pitch 65 (<= 67.3 KiB: two workgroups per CU); a wave owns one query row per pass and lane j
// key j, so the softmax reductions span the wave; 16 lanes x 16 bytes finish one context row, 16 rows per pass.  float32
// throughout, the keys added in ascending order, keys j >= max_len at probability exactly 0.
__global__ __launch_bounds__(256) void bert_attention_long_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                                 const int32_t* __restrict__ max_len, float* __restrict__ ctx,
                                                                 int T, int H) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const Q = lds;
    float* const K = Q + T * KP;
    float* const V = K + T * KP;
    float* const P = V + T * KP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int heads = H / DH;
    const int n = blockIdx.x / heads, hd = blockIdx.x - n * heads;
    int ml = max_len[n];
    ml = ml < 1 ? 1 : (ml > T ? T : ml);             // validated on the host copy; clamped so that no index can leave the tile
    const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;       // 16 rows per pass, 16 lanes x 16 bytes per row

    {
        const float4 bq = *reinterpret_cast<const float4*>(bias + hd * DH + c4);
        const float4 bk = *reinterpret_cast<const float4*>(bias + H + hd * DH + c4);
        const float4 bv = *reinterpret_cast<const float4*>(bias + 2 * H + hd * DH + c4);
        for (int t = r; t < T; t += 16) {
            const float* row = qkv + ((size_t)n * T + t) * (3 * (size_t)H) + hd * DH + c4;
            *reinterpret_cast<float4*>(Q + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row), bq);
            *reinterpret_cast<float4*>(K + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + H), bk);
            *reinterpret_cast<float4*>(V + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + 2 * H), bv);
        }
    }
    __syncthreads();

    {
        const int j = lane;
        const int jr = j < T ? j : T - 1;
        const bool live = j < ml;
        for (int i = wave; i < T; i += 4) {          // wave-uniform
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const float4 qv = *reinterpret_cast<const float4*>(Q + i * KP + d);
                const float4 kv = *reinterpret_cast<const float4*>(K + jr * KP + d);
                s = fmaf(qv.x, kv.x, s); s = fmaf(qv.y, kv.y, s); s = fmaf(qv.z, kv.z, s); s = fmaf(qv.w, kv.w, s);
            }
            s = live ? s * 0.125f : -INFINITY;
            const float m = wave_max(s);
            const float e = live ? expf(s - m) : 0.f;
            const float sum = wave_sum(e);
            if (j < T) P[i * PP_LONG + j] = e / sum;
        }
    }
    __syncthreads();

    for (int i = r; i < T; i += 16) {                // ctx[i][d] = sum_{j < max_len} p[i][j] v[j][d], j ascending
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < ml; ++j) {
            const float pj = P[i * PP_LONG + j];
            const float4 vv = *reinterpret_cast<const float4*>(V + j * KP + c4);
            acc.x = fmaf(pj, vv.x, acc.x); acc.y = fmaf(pj, vv.y, acc.y);
            acc.z = fmaf(pj, vv.z, acc.z); acc.w = fmaf(pj, vv.w, acc.w);
        }
        *reinterpret_cast<float4*>(ctx + ((size_t)n * T + i) * H + hd * DH + c4) = acc;
    }
}

// one thread per (caption, four channels): the T rows added in order, then divided by max_len (the reference divides the sum over
// ALL T positions, padding included, by the number of real tokens)
__global__ __launch_bounds__(256) void bert_sentence_kernel(const float* __restrict__ emb, const int32_t* __restrict__ max_len,
                                                            float* __restrict__ out, int N, int T, int h4) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * h4) return;
    const int n = (int)(t / h4), c = (int)(t - (long long)n * h4);
    const float4* src = reinterpret_cast<const float4*>(emb) + (size_t)n * T * h4 + c;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0; i < T; ++i) acc = add4(acc, src[(size_t)i * h4]);
    const float d = (float)max_len[n];
    reinterpret_cast<float4*>(out)[t] = make_float4(acc.x / d, acc.y / d, acc.z / d, acc.w / d);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
inline bool ln_row_ok(int h) { return h > 0 && h % 4 == 0 && h <= 64 * 4 * LN_MAXV; }

}  // namespace

extern "C" int xmc_bert_embed_ln(const int32_t* ids, const float* word, const float* pos, const float* type, const float* gamma,
                                 const float* beta, float* y, int32_t rows, int32_t t, int32_t h, int32_t vocab, int32_t npos,
                                 float eps, void* stream) {
    XMC_REQUIRE(ids && word && pos && type && gamma && beta && y);
    XMC_REQUIRE(rows > 0 && t > 0 && t <= npos && vocab > 0 && ln_row_ok(h) && eps >= 0.f);
    XMC_REQUIRE(aligned16(word) && aligned16(pos) && aligned16(type) && aligned16(gamma) && aligned16(beta) && aligned16(y));
    RowLnArgs a{};
    a.ids = ids; a.word = word; a.pos = pos; a.type = type; a.gamma = gamma; a.beta = beta; a.y = y;
    a.rows = rows; a.T = t; a.H = h; a.V = vocab; a.eps = eps;
    hipLaunchKernelGGL(row_ln_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bias_residual_ln(const float* x, const float* bias, const float* res, const float* gamma, const float* beta,
                                    float* y, int32_t rows, int32_t h, float eps, void* stream) {
    XMC_REQUIRE(x && bias && res && gamma && beta && y);
    XMC_REQUIRE(rows > 0 && ln_row_ok(h) && eps >= 0.f);
    XMC_REQUIRE(aligned16(x) && aligned16(bias) && aligned16(res) && aligned16(gamma) && aligned16(beta) && aligned16(y));
    RowLnArgs a{};
    a.x = x; a.bias = bias; a.res = res; a.gamma = gamma; a.beta = beta; a.y = y;
    a.rows = rows; a.T = 1; a.H = h; a.V = 1; a.eps = eps;
    hipLaunchKernelGGL(row_ln_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bias_gelu(const float* x, const float* bias, float* y, int32_t rows, int32_t f, void* stream) {
    XMC_REQUIRE(x && bias && y && rows > 0 && f > 0 && f % 4 == 0);
    XMC_REQUIRE(aligned16(x) && aligned16(bias) && aligned16(y));
    const int f4 = f / 4, bpr = (f4 + 255) / 256;
    XMC_REQUIRE((long long)rows * bpr < (1ll << 31));
    hipLaunchKernelGGL(bias_gelu_kernel, dim3((unsigned)(rows * bpr)), dim3(256), 0, static_cast<hipStream_t>(stream), x, bias, y,
                       f4, bpr);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bert_attention(const float* qkv, const float* bias_qkv, const int32_t* max_len, const int32_t* max_len_host,
                                  float* ctx, int32_t n, int32_t t, int32_t h, void* stream) {
    XMC_REQUIRE(qkv && bias_qkv && max_len && max_len_host && ctx);
    XMC_REQUIRE(n > 0 && t >= 2 && t <= ATT_MAX_T && h >= DH && h % DH == 0);
    XMC_REQUIRE((long long)n * (h / DH) < (1ll << 31));
    XMC_REQUIRE(aligned16(qkv) && aligned16(bias_qkv) && aligned16(ctx));
    for (int i = 0; i < n; ++i) XMC_REQUIRE(max_len_host[i] >= 2 && max_len_host[i] <= t);
    const size_t lds = (size_t)(3 * t * KP + t * PP) * sizeof(float);          // <= 30.3 KiB
    hipLaunchKernelGGL(bert_attention_kernel, dim3((unsigned)(n * (h / DH))), dim3(64), lds, static_cast<hipStream_t>(stream), qkv,
                       bias_qkv, max_len, ctx, t, h);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bert_attention_long(const float* qkv, const float* bias_qkv, const int32_t* max_len, const int32_t* max_len_host,
                                       float* ctx, int32_t n, int32_t t, int32_t h, void* stream) {
    XMC_REQUIRE(qkv && bias_qkv && max_len && max_len_host && ctx);
    XMC_REQUIRE(n > 0 && t >= 2 && t <= ATT_MAX_T_LONG && h >= DH && h % DH == 0);
    XMC_REQUIRE((long long)n * (h / DH) < (1ll << 31));
    XMC_REQUIRE(aligned16(qkv) && aligned16(bias_qkv) && aligned16(ctx));
    for (int i = 0; i < n; ++i) XMC_REQUIRE(max_len_host[i] >= 2 && max_len_host[i] <= t);
    const size_t lds = (size_t)(3 * t * KP + t * PP_LONG) * sizeof(float);     // <= 67.3 KiB: above the 64 KiB default
    static XmcLdsOptIn opt_in;
    if (!opt_in.ensure({reinterpret_cast<const void*>(&bert_attention_long_kernel)}, 3 * ATT_MAX_T_LONG * KP * 4 + ATT_MAX_T_LONG * PP_LONG * 4))
        return XMC_EINVAL;
    hipLaunchKernelGGL(bert_attention_long_kernel, dim3((unsigned)(n * (h / DH))), dim3(256), lds, static_cast<hipStream_t>(stream),
                       qkv, bias_qkv, max_len, ctx, t, h);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bert_sentence(const float* emb, const int32_t* max_len, float* out, int32_t n, int32_t t, int32_t h,
                                 void* stream) {
    XMC_REQUIRE(emb && max_len && out && n > 0 && t > 0 && h > 0 && h % 4 == 0);
    XMC_REQUIRE(aligned16(emb) && aligned16(out));
    const long long threads = (long long)n * (h / 4);
    hipLaunchKernelGGL(bert_sentence_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), emb, max_len, out, n, t, h / 4);
    XMC_LAUNCH_RET();
}
