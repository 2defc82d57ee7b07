// Data gradient of the CLIP image tower (config.clip_guidance_weight; utils/clip_utils.ClipEncoder.image_backward): the adjoint of
// every kernel of clip.hip that the pullback crosses.  The weights are frozen: no weight gradient.  The dense adjoints dX = dY W
// and the patch "convolution" run on xmc_gemm_f32 / xmc_gemm_f32_bf16mfma.  Specification: utils/clip_grad.py (NumPy float64).
//
//   xmc_mha_attention_bwd     dqkv from dctx; the probabilities are recomputed in LDS from qkv       one workgroup per (sequence, head)
//   xmc_ln_bwd_add            dx = LN-backward(x, gamma, dy) (+ dres), three row maps                one wave per row
//   xmc_bias_quick_gelu_bwd   dv = dy (s + 1.702 v s (1 - s)), v = x + bias, s = sigmoid(1.702 v)     16 bytes per lane
//   xmc_clip_preprocess_bwd   the transpose of xmc_clip_preprocess, in gather form                    one workgroup per (image, input row)
//
// float32 arithmetic (float64 inside the QuickGELU derivative, as in its forward twin), every cross-lane reduction a fixed xor
// tree, every sum in ascending index order, no float atomics: two launches on the same inputs give the same bits.
#include "common.h"
#include "clip_taps.h"

namespace {

constexpr int LN_MAXV = 4;     // float4 per lane: rows of up to 1024 floats (as clip.hip)
constexpr int DH = 64;         // head dimension
constexpr int KP = 68;         // LDS pitch of the 64-float rows (as clip.hip)
constexpr int MHA_MAX_T = 128;
constexpr int QC = 32;         // query rows per pass of the attention backward
constexpr int PRE_MIN_HW = 32, PRE_MAX_HW = 512, PRE_MAX_S = 448;

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ void fma4(float4& acc, float s, float4 v) {
    acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}

// ------------------------------------------------------------------------------------------------------- attention backward
// 1 <= T <= 128.  LDS: the k and v rows [T][KP] with their biases added (69,632 bytes at T = 128), one pass's QC = 32 query rows
// q + b_q and dctx [QC][KP] each (17,408), and that pass's probabilities P and score gradients dS [QC][T + 1] each (33,024):
// 120,064 bytes at T = 128 (one workgroup per CU), 57,664 at the 50 tokens of ViT-B/32 (two).  Storing q and dctx for all T rows
// beside the T x T probabilities, as the forward kernel's layout would suggest, needs 205 KB: the CU has 160.
// Per pass: a wave owns one query row at a time and recomputes its probabilities exactly as the forward kernel does (lane j the
// keys j and j + 64, q broadcast with v_readlane), then dP = dctx . v_j, delta = sum_j p_j dP_j (xor tree), dS = p (dP - delta) / 8.
// After a barrier 16 lanes x 16 bytes finish one row: dQ of the pass's rows (sum over the keys, ascending) goes to memory, dK and
// dV of key rows r, r + 16, .. stay in registers and take the pass's query rows in ascending order.  Masked keys have P = dS = 0
// exactly; dQ skips them as the forward's context sum does.
__global__ __launch_bounds__(256) void mha_attention_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                               const int32_t* __restrict__ len, const float* __restrict__ dctx,
                                                               float* __restrict__ dqkv, int T, int H, int causal) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const K = lds;
    float* const V = K + T * KP;
    float* const Q = V + T * KP;              // [QC][KP]
    float* const DO = Q + QC * KP;            // [QC][KP]
    float* const P = DO + QC * KP;            // [QC][T + 1]
    const int PPT = T + 1;
    float* const DS = P + QC * PPT;           // [QC][T + 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int heads = H / DH;
    const int n = blockIdx.x / heads, hd = blockIdx.x - n * heads;
    int ml = len[n];
    ml = ml < 1 ? 1 : (ml > T ? T : ml);             // validated on the host copy; clamped so that no index can leave the tile
    const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;       // 16 rows per pass, 16 lanes x 16 bytes per row
    const size_t H3 = 3 * (size_t)H;
    const float* const base = qkv + (size_t)n * T * H3 + hd * DH;
    const float* const dbase = dctx + (size_t)n * T * H + hd * DH;
    float* const obase = dqkv + (size_t)n * T * H3 + hd * DH;

    {
        const float4 bk = *reinterpret_cast<const float4*>(bias + H + hd * DH + c4);
        const float4 bv = *reinterpret_cast<const float4*>(bias + 2 * H + hd * DH + c4);
        for (int t = r; t < T; t += 16) {
            const float* row = base + (size_t)t * H3 + c4;
            *reinterpret_cast<float4*>(K + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + H), bk);
            *reinterpret_cast<float4*>(V + t * KP + c4) = add4(*reinterpret_cast<const float4*>(row + 2 * H), bv);
        }
    }
    const float4 bq = *reinterpret_cast<const float4*>(bias + hd * DH + c4);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dk[MHA_MAX_T / 16], dv[MHA_MAX_T / 16];   // key rows r + 16 m
#pragma unroll
    for (int m = 0; m < MHA_MAX_T / 16; ++m) dk[m] = dv[m] = zero4;

    for (int i0 = 0; i0 < T; i0 += QC) {             // workgroup-uniform
        const int rows = T - i0 < QC ? T - i0 : QC;
        __syncthreads();                             // the previous pass has read Q, DO, P, DS (first pass: K, V are written)
        for (int ii = r; ii < rows; ii += 16) {
            *reinterpret_cast<float4*>(Q + ii * KP + c4) =
                add4(*reinterpret_cast<const float4*>(base + (size_t)(i0 + ii) * H3 + c4), bq);
            *reinterpret_cast<float4*>(DO + ii * KP + c4) = *reinterpret_cast<const float4*>(dbase + (size_t)(i0 + ii) * H + c4);
        }
        __syncthreads();

        {
            const int j0 = lane, j1 = lane + 64;
            const int jr0 = j0 < T ? j0 : T - 1, jr1 = j1 < T ? j1 : T - 1;
            for (int ii = wave; ii < rows; ii += 4) {    // wave-uniform
                const int i = i0 + ii;
                const int qi = __float_as_int(Q[ii * KP + lane]);
                const int gi = __float_as_int(DO[ii * KP + lane]);
                const int lim = causal ? (i + 1 < ml ? i + 1 : ml) : ml;                       // keys j < lim are live (lim >= 1)
                float s0 = 0.f, s1 = 0.f, p0 = 0.f, p1 = 0.f;
#pragma unroll
                for (int d = 0; d < DH; d += 4) {
                    const float q0 = __int_as_float(__builtin_amdgcn_readlane(qi, d)), q1 = __int_as_float(__builtin_amdgcn_readlane(qi, d + 1));
                    const float q2 = __int_as_float(__builtin_amdgcn_readlane(qi, d + 2)), q3 = __int_as_float(__builtin_amdgcn_readlane(qi, d + 3));
                    const float g0 = __int_as_float(__builtin_amdgcn_readlane(gi, d)), g1 = __int_as_float(__builtin_amdgcn_readlane(gi, d + 1));
                    const float g2 = __int_as_float(__builtin_amdgcn_readlane(gi, d + 2)), g3 = __int_as_float(__builtin_amdgcn_readlane(gi, d + 3));
                    const float4 ka = *reinterpret_cast<const float4*>(K + jr0 * KP + d);
                    const float4 kb = *reinterpret_cast<const float4*>(K + jr1 * KP + d);
                    const float4 va = *reinterpret_cast<const float4*>(V + jr0 * KP + d);
                    const float4 vb = *reinterpret_cast<const float4*>(V + jr1 * KP + d);
                    s0 = fmaf(q0, ka.x, s0); s0 = fmaf(q1, ka.y, s0); s0 = fmaf(q2, ka.z, s0); s0 = fmaf(q3, ka.w, s0);
                    s1 = fmaf(q0, kb.x, s1); s1 = fmaf(q1, kb.y, s1); s1 = fmaf(q2, kb.z, s1); s1 = fmaf(q3, kb.w, s1);
                    p0 = fmaf(g0, va.x, p0); p0 = fmaf(g1, va.y, p0); p0 = fmaf(g2, va.z, p0); p0 = fmaf(g3, va.w, p0);
                    p1 = fmaf(g0, vb.x, p1); p1 = fmaf(g1, vb.y, p1); p1 = fmaf(g2, vb.z, p1); p1 = fmaf(g3, vb.w, p1);
                }
                const bool live0 = j0 < lim, live1 = j1 < lim;
                s0 = live0 ? s0 * 0.125f : -INFINITY;
                s1 = live1 ? s1 * 0.125f : -INFINITY;
                const float mx = wave_max(fmaxf(s0, s1));                // key 0 is always live: mx is finite
                const float e0 = live0 ? expf(s0 - mx) : 0.f, e1 = live1 ? expf(s1 - mx) : 0.f;
                const float sum = wave_sum(e0 + e1);
                const float pr0 = e0 / sum, pr1 = e1 / sum;              // (the forward kernel's probabilities, bit for bit)
                const float delta = wave_sum(fmaf(pr0, live0 ? p0 : 0.f, pr1 * (live1 ? p1 : 0.f)));
                const float ds0 = live0 ? pr0 * (p0 - delta) * 0.125f : 0.f;
                const float ds1 = live1 ? pr1 * (p1 - delta) * 0.125f : 0.f;
                if (j0 < T) { P[ii * PPT + j0] = pr0; DS[ii * PPT + j0] = ds0; }
                if (j1 < T) { P[ii * PPT + j1] = pr1; DS[ii * PPT + j1] = ds1; }
            }
        }
        __syncthreads();

        for (int ii = r; ii < rows; ii += 16) {      // dQ[i] = sum over the live keys of dS[i][j] k[j], j ascending
            const int i = i0 + ii;
            const int lim = causal ? (i + 1 < ml ? i + 1 : ml) : ml;
            float4 acc = zero4;
            for (int j = 0; j < lim; ++j) fma4(acc, DS[ii * PPT + j], *reinterpret_cast<const float4*>(K + j * KP + c4));
            *reinterpret_cast<float4*>(obase + (size_t)i * H3 + c4) = acc;
        }
#pragma unroll
        for (int m = 0; m < MHA_MAX_T / 16; ++m) {   // dK[j] += sum_i dS[i][j] q[i], dV[j] += sum_i P[i][j] dctx[i], i ascending
            const int j = r + 16 * m;
            if (j < T) {
                for (int ii = 0; ii < rows; ++ii) {
                    fma4(dk[m], DS[ii * PPT + j], *reinterpret_cast<const float4*>(Q + ii * KP + c4));
                    fma4(dv[m], P[ii * PPT + j], *reinterpret_cast<const float4*>(DO + ii * KP + c4));
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MHA_MAX_T / 16; ++m) {
        const int j = r + 16 * m;
        if (j < T) {
            *reinterpret_cast<float4*>(obase + (size_t)j * H3 + H + c4) = dk[m];
            *reinterpret_cast<float4*>(obase + (size_t)j * H3 + 2 * H + c4) = dv[m];
        }
    }
}

// ------------------------------------------------------------------------------------------------------- LayerNorm backward
enum { LNB_ROWS = XMC_LN_BWD_ROWS, LNB_GATHER = XMC_LN_BWD_GATHER, LNB_VISION = XMC_LN_BWD_VISION };

struct LnBwdArgs {
    const float* x;  const float* pos;  const float* gamma;  const float* dy;  const float* dres;
    float* dx;
    int rows, T, H;
    float eps;
};

// One wave per OUTPUT row.  x row (+ pos row) and dy row in registers; mean and variance in two passes as the forward kernels; with
// g = dy gamma: dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres).
//   LNB_ROWS    row r of x, dy, dres, dx
//   LNB_GATHER  dx is the stream (n T, H); row i T takes LN-backward(x[i T], dy[i]) (dy is (n, H)), every other row 0; (+ dres)
//   LNB_VISION  dx is (n (T - 1), H); row (i, j - 1) takes LN-backward(x[i, j - 1] + pos[j], dy[i T + j]), j >= 1: the class row drops
template <int MODE>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnBwdArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= p.rows) return;                       // wave-uniform; no barrier in this kernel
    const int H = p.H;
    const float* xr = p.x + (size_t)row * H;
    const float* dyr = p.dy + (size_t)row * H;
    const float* posr = nullptr;
    bool active = true;
    if constexpr (MODE == LNB_GATHER) {
        const int i = row / p.T;
        active = row == i * p.T;                     // wave-uniform
        dyr = p.dy + (size_t)i * H;                  // (inside dy for every row; read only when active)
    } else if constexpr (MODE == LNB_VISION) {
        const int i = row / (p.T - 1), j = row - i * (p.T - 1) + 1;
        dyr = p.dy + ((size_t)i * p.T + j) * H;
        posr = p.pos + (size_t)j * H;
    }
    const float* dr = p.dres ? p.dres + (size_t)row * H : nullptr;
    float* out = p.dx + (size_t)row * H;
    float4 v[LN_MAXV], g[LN_MAXV];
    if (!active) {                                   // LNB_GATHER, rows 1 .. T - 1: 0 (+ dres)
#pragma unroll
        for (int j = 0; j < LN_MAXV; ++j) {
            const int col = (lane + 64 * j) * 4;
            if (col < H) *reinterpret_cast<float4*>(out + col) = dr ? *reinterpret_cast<const float4*>(dr + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        v[j] = g[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < H) {
            v[j] = *reinterpret_cast<const float4*>(xr + col);
            if (posr) v[j] = add4(v[j], *reinterpret_cast<const float4*>(posr + col));
            const float4 d = *reinterpret_cast<const float4*>(dyr + col);
            const float4 ga = *reinterpret_cast<const float4*>(p.gamma + col);
            g[j] = make_float4(d.x * ga.x, d.y * ga.y, d.z * ga.z, d.w * ga.w);
        }
        s += (v[j].x + v[j].y) + (v[j].z + v[j].w);                                       // (columns >= H hold zeros)
    }
    const float inv_h = 1.f / (float)H;
    const float mean = wave_sum(s) * inv_h;
    float q = 0.f, sg = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        if (col < H) {
            v[j] = make_float4(v[j].x - mean, v[j].y - mean, v[j].z - mean, v[j].w - mean);
            q = fmaf(v[j].x, v[j].x, q); q = fmaf(v[j].y, v[j].y, q);
            q = fmaf(v[j].z, v[j].z, q); q = fmaf(v[j].w, v[j].w, q);
        }
        sg += (g[j].x + g[j].y) + (g[j].z + g[j].w);
    }
    const float var = wave_sum(q) * inv_h;           // biased
    const float rstd = 1.f / sqrtf(var + p.eps);
    float sgx = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {              // v <- xhat (columns >= H: 0)
        v[j] = make_float4(v[j].x * rstd, v[j].y * rstd, v[j].z * rstd, v[j].w * rstd);
        sgx = fmaf(g[j].x, v[j].x, sgx); sgx = fmaf(g[j].y, v[j].y, sgx);
        sgx = fmaf(g[j].z, v[j].z, sgx); sgx = fmaf(g[j].w, v[j].w, sgx);
    }
    const float mg = wave_sum(sg) * inv_h, mgx = wave_sum(sgx) * inv_h;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int col = (lane + 64 * j) * 4;
        if (col < H) {
            float4 o = make_float4(rstd * ((g[j].x - mg) - v[j].x * mgx), rstd * ((g[j].y - mg) - v[j].y * mgx),
                                   rstd * ((g[j].z - mg) - v[j].z * mgx), rstd * ((g[j].w - mg) - v[j].w * mgx));
            if (dr) o = add4(o, *reinterpret_cast<const float4*>(dr + col));      // (dres may be dx: a lane reads what it overwrites)
            *reinterpret_cast<float4*>(out + col) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- QuickGELU backward
// d/dv [v s(1.702 v)] = s + 1.702 v s (1 - s) in DOUBLE, times dy, rounded once (the forward twin evaluates in double too)
__device__ __forceinline__ float qgelu_bwd1(float x, float b, float dy) {
    const double v = (double)(x + b);
    const double s = 1.0 / (1.0 + exp(-1.702 * v));
    return (float)((double)dy * (s + 1.702 * v * s * (1.0 - s)));
}

__global__ __launch_bounds__(256) void bias_quick_gelu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                                  const float* dy, float* dv, int f4, int bpr) {   // (dv may be dy)
    const int row = blockIdx.x / bpr;
    const int c = (blockIdx.x - row * bpr) * 256 + threadIdx.x;
    if (c >= f4) return;
    const size_t t = (size_t)row * f4 + c;
    const float4 a = reinterpret_cast<const float4*>(x)[t];
    const float4 b = reinterpret_cast<const float4*>(bias)[c];
    const float4 d = reinterpret_cast<const float4*>(dy)[t];
    reinterpret_cast<float4*>(dv)[t] = make_float4(qgelu_bwd1(a.x, b.x, d.x), qgelu_bwd1(a.y, b.y, d.y), qgelu_bwd1(a.z, b.z, d.z),
                                                   qgelu_bwd1(a.w, b.w, d.w));
}

// ----------------------------------------------------------------------------------------------------- preprocessing backward
template <typename T> __device__ __forceinline__ void put(T* p, size_t i, float v);
template <> __device__ __forceinline__ void put<float>(float* p, size_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void put<bf16_t>(bf16_t* p, size_t i, float v) { p[i] = f2bf(v); }

struct PreBwdArgs {
    const float* dy;  void* dx;
    int n, hw, S, P, ksize;
    float rstd[3];
};

// The forward is y = (Ry X Rx^T - mean) / std per channel with R the (S, hw) matrix of cubic_taps; this is dX = Ry^T (dY / std) Rx.
// One workgroup per (image, INPUT row iy).  LDS: the taps of every output index [S][ksize] with window starts and counts (the image is
// square: one table serves both axes), per input index the first and last output index whose window holds it (integer min / max:
// the windows' ends are monotone, so those form a range), and the vertically gathered row [S][3].  Both passes GATHER: an element
// adds the outputs of its range in ascending order; an output of the range whose window does not hold the element (none, by the
// monotonicity; kept so that no assumption indexes the table) gets weight 0 at a clamped index.
template <typename T>
__global__ __launch_bounds__(256) void clip_preprocess_bwd_kernel(const PreBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = p.S, hw = p.hw, ks = p.ksize;
    float* const w = lds;                                            // [S][ks]
    float* const tmp = w + S * ks;                                   // [S * 3]: (c, ox)
    int* const lo = reinterpret_cast<int*>(tmp + S * 3);             // [S]
    int* const cnt = lo + S;                                         // [S]
    int* const first = cnt + S;                                      // [hw]
    int* const last = first + hw;                                    // [hw]
    const int img = blockIdx.x / hw, iy = blockIdx.x - img * hw;
    const int tid = threadIdx.x;

    for (int i = tid; i < hw; i += 256) { first[i] = S; last[i] = -1; }
    for (int o = tid; o < S; o += 256) {
        int l;
        cnt[o] = cubic_taps(o, hw, S, ks, w + o * ks, &l);
        lo[o] = l;
    }
    __syncthreads();
    for (int o = tid; o < S; o += 256) {
        const int l = lo[o], c = cnt[o];                             // l + c <= hw
        for (int k = 0; k < c; ++k) {
            atomicMin(&first[l + k], o);                             // (integers: the result does not depend on the order)
            atomicMax(&last[l + k], o);
        }
    }
    __syncthreads();

    const int G = S / p.P, PP2 = p.P * p.P;
    const float* const src = p.dy + (size_t)img * G * G * (3 * PP2);
    {
        const int o_lo = first[iy], o_hi = last[iy];                 // workgroup-uniform; empty range: S, -1
        for (int e = tid; e < S * 3; e += 256) {
            const int c = e / S, ox = e - c * S;                     // a run of lanes shares c: contiguous kx in the patch row
            const int gx = ox / p.P, kx = ox - gx * p.P;
            float acc = 0.f;
            for (int oy = o_lo; oy <= o_hi; ++oy) {
                const int k = iy - lo[oy];
                const bool in = k >= 0 && k < cnt[oy];
                const float wv = in ? w[oy * ks + (k < 0 ? 0 : (k >= ks ? ks - 1 : k))] : 0.f;
                const int gy = oy / p.P, ky = oy - gy * p.P;
                acc = fmaf(wv, src[((size_t)gy * G + gx) * (3 * PP2) + c * PP2 + ky * p.P + kx], acc);
            }
            tmp[e] = acc;
        }
    }
    __syncthreads();

    T* const dst = static_cast<T*>(p.dx) + ((size_t)img * hw + iy) * hw * 3;
    for (int e = tid; e < hw * 3; e += 256) {                        // element e of the input row: (x, c) interleaved, contiguous
        const int ix = e / 3, c = e - ix * 3;
        const int o_lo = first[ix], o_hi = last[ix];
        float acc = 0.f;
        for (int ox = o_lo; ox <= o_hi; ++ox) {
            const int k = ix - lo[ox];
            const bool in = k >= 0 && k < cnt[ox];
            const float wv = in ? w[ox * ks + (k < 0 ? 0 : (k >= ks ? ks - 1 : k))] : 0.f;
            acc = fmaf(wv, tmp[c * S + ox], acc);
        }
        put<T>(dst, e, acc * p.rstd[c]);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
inline bool ln_row_ok(int h) { return h > 0 && h % 4 == 0 && h <= 64 * 4 * LN_MAXV; }
inline unsigned row_blocks(int rows) { return (unsigned)((rows + 3) / 4); }
inline int pre_ksize(int hw, int S) {
    const double scale = (double)hw / (double)S;
    return (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
inline size_t mha_bwd_lds(int t) { return (size_t)(2 * t * KP + 2 * QC * KP + 2 * QC * (t + 1)) * sizeof(float); }

}  // namespace

extern "C" int xmc_mha_attention_bwd(const float* qkv, const float* bias_qkv, const int32_t* len, const int32_t* len_host,
                                     const float* dctx, float* dqkv, int32_t n, int32_t t, int32_t h, int32_t causal, void* stream) {
    XMC_REQUIRE(qkv && bias_qkv && len && len_host && dctx && dqkv);
    XMC_REQUIRE(n > 0 && t >= 1 && t <= MHA_MAX_T && h >= DH && h % DH == 0);
    XMC_REQUIRE((long long)n * (h / DH) < (1ll << 31));
    XMC_REQUIRE(aligned16(qkv) && aligned16(bias_qkv) && aligned16(dctx) && aligned16(dqkv));
    XMC_REQUIRE(dqkv != qkv);
    for (int i = 0; i < n; ++i) XMC_REQUIRE(len_host[i] >= 1 && len_host[i] <= t);
    static XmcLdsOptIn opt_in;                                       // 120,064 bytes at t = 128: above the 64 KiB default
    if (!opt_in.ensure({reinterpret_cast<const void*>(&mha_attention_bwd_kernel)}, (int)mha_bwd_lds(MHA_MAX_T))) return XMC_EINVAL;
    hipLaunchKernelGGL(mha_attention_bwd_kernel, dim3((unsigned)(n * (h / DH))), dim3(256), mha_bwd_lds(t),
                       static_cast<hipStream_t>(stream), qkv, bias_qkv, len, dctx, dqkv, t, h, causal != 0);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_ln_bwd_add(const float* x, const float* pos, const float* gamma, const float* dy, const float* dres, float* dx,
                              int32_t rows, int32_t t, int32_t h, float eps, int32_t mode, void* stream) {
    XMC_REQUIRE(x && gamma && dy && dx);
    XMC_REQUIRE(mode == LNB_ROWS || mode == LNB_GATHER || mode == LNB_VISION);
    XMC_REQUIRE(rows > 0 && ln_row_ok(h) && eps >= 0.f);
    XMC_REQUIRE(aligned16(x) && aligned16(pos) && aligned16(gamma) && aligned16(dy) && aligned16(dres) && aligned16(dx));
    XMC_REQUIRE(dx != x && dx != dy);                                // (dres == dx is fine: a lane overwrites what it has read)
    LnBwdArgs a{};
    a.x = x; a.pos = pos; a.gamma = gamma; a.dy = dy; a.dres = dres; a.dx = dx;
    a.rows = rows; a.T = t; a.H = h; a.eps = eps;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == LNB_ROWS) {
        XMC_REQUIRE(pos == nullptr && t == 1);
        hipLaunchKernelGGL(ln_bwd_kernel<LNB_ROWS>, dim3(row_blocks(rows)), dim3(256), 0, st, a);
    } else if (mode == LNB_GATHER) {
        XMC_REQUIRE(pos == nullptr && t >= 1 && rows % t == 0);      // rows = n t stream rows; dy (n, h)
        hipLaunchKernelGGL(ln_bwd_kernel<LNB_GATHER>, dim3(row_blocks(rows)), dim3(256), 0, st, a);
    } else {
        XMC_REQUIRE(pos != nullptr && dres == nullptr && t >= 2 && rows % (t - 1) == 0);      // rows = n (t - 1) patch rows; dy (n t, h)
        hipLaunchKernelGGL(ln_bwd_kernel<LNB_VISION>, dim3(row_blocks(rows)), dim3(256), 0, st, a);
    }
    XMC_LAUNCH_RET();
}

extern "C" int xmc_bias_quick_gelu_bwd(const float* x, const float* bias, const float* dy, float* dv, int32_t rows, int32_t f,
                                       void* stream) {
    XMC_REQUIRE(x && bias && dy && dv && rows > 0 && f > 0 && f % 4 == 0);
    XMC_REQUIRE(aligned16(x) && aligned16(bias) && aligned16(dy) && aligned16(dv));
    XMC_REQUIRE(dv != x);
    const int f4 = f / 4, bpr = (f4 + 255) / 256;
    XMC_REQUIRE((long long)rows * bpr < (1ll << 31));
    hipLaunchKernelGGL(bias_quick_gelu_bwd_kernel, dim3((unsigned)(rows * bpr)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       bias, dy, dv, f4, bpr);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_clip_preprocess_bwd(const float* dpatches, void* dimages, int32_t n, int32_t hw, int32_t s, int32_t p,
                                       const float* std3, int32_t dtype, void* stream) {
    XMC_REQUIRE(dpatches && dimages && std3);
    XMC_REQUIRE(dtype == XMC_F32 || dtype == XMC_BF16);
    XMC_REQUIRE(n > 0 && hw >= PRE_MIN_HW && hw <= PRE_MAX_HW && p > 0 && s >= p && s <= PRE_MAX_S && s % p == 0);
    XMC_REQUIRE((long long)n * hw < (1ll << 31));
    XMC_REQUIRE(aligned16(dpatches) && aligned16(dimages));
    PreBwdArgs a{};
    a.dy = dpatches; a.dx = dimages; a.n = n; a.hw = hw; a.S = s; a.P = p; a.ksize = pre_ksize(hw, s);
    for (int c = 0; c < 3; ++c) {
        XMC_REQUIRE(std3[c] > 0.f && std3[c] == std3[c]);            // a host array, passed to the kernel by value
        a.rstd[c] = 1.f / std3[c];
    }
    const size_t lds = ((size_t)s * a.ksize + (size_t)s * 3) * sizeof(float) + ((size_t)2 * s + (size_t)2 * hw) * sizeof(int);
    XMC_REQUIRE(lds <= 64 * 1024);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == XMC_F32) hipLaunchKernelGGL(clip_preprocess_bwd_kernel<float>, dim3((unsigned)(n * hw)), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(clip_preprocess_bwd_kernel<bf16_t>, dim3((unsigned)(n * hw)), dim3(256), lds, st, a);
    XMC_LAUNCH_RET();
}
