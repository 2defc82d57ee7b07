// Pairwise sample metrics over two pools of Inception features (utils/sample_metrics.py is the specification): k-NN radii and ball
// membership of improved precision / recall, and the cubic-kernel sums of KID.  One kernel, three epilogues:
//   a workgroup owns 128 rows of the "row" pool and walks ALL 128-row tiles of the "column" pool; per tile the 128 x 128 dot
//   products run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: one rounding per product, as gemm_f32.hip), the tile goes to LDS
//   in two 64-column halves, and thread r < 128 scans row r of it in column order, keeping that row's state in registers -- its 8
//   smallest squared distances, its hit flag, or its float64 partial sum.  No n x m matrix exists anywhere, no workgroup depends on
//   another, and nothing is accumulated with atomics: two launches on the same inputs write the same bits.
// Everything after the dot product is float64: dist = max(0, |a|^2 + |b|^2 - 2 (double)dot) with the squared norms float64 sums of
// the float32 squares (sm_sqnorm_kernel), the comparison with the radius, (dot / d + 1)^3 and every sum.
#include "common.h"

namespace {

constexpr int SM_T = 128;                 // rows of the row block = rows of a column tile
constexpr int SM_BK = 32;                 // k per staged tile (d % 32 == 0: no ragged k)
constexpr int SM_P = SM_T + 1;            // pitch of the [k][row] staging images (conflict-free one-element-per-lane fragments)
constexpr int SM_HP = SM_T / 2 + 1;       // pitch of the [row][64 columns] half tile a row's thread scans
constexpr int SM_STAGE = 2 * SM_BK * SM_P, SM_HALF = SM_T * SM_HP;
constexpr int SM_LDS = SM_STAGE > SM_HALF ? SM_STAGE : SM_HALF;      // the half tile reuses the staging floats
constexpr int SM_KMAX = 8;

enum { SM_KNN = 0, SM_HITS = 1, SM_POLY3 = 2 };

struct sm_args {
    const float* a;                       // row pool [.][d]
    const float* b;                       // column pool [.][d]
    const int32_t* ai;                    // SM_POLY3: [subsets][n] rows of `a` (blockIdx.y = subset); else NULL: row r is a[r]
    const int32_t* bi;                    //           [subsets][m] rows of `b`
    const double* na;                     // squared norms of a's rows (SM_KNN, SM_HITS)
    const double* nb;                     // ... of b's rows
    const double* rb;                     // SM_HITS: squared radius of every row of b
    double* out;                          // SM_KNN: radii2[n]; SM_POLY3: partial sums [subsets][gridDim.x]
    uint8_t* hit;                         // SM_HITS: [n]
    int n, m, d, k;                       // rows, columns, features, neighbour rank
    int pool_a, pool_b;                   // SM_POLY3: rows of the pools (what the device copy of an index is clamped to)
    int same;                             // rows and columns are the same set: the pair (r, r) is left out
};

// |x_r|^2 = sum of (double)x^2: one wave per row, lane l adds elements l, l + 64, ... in order, then a fixed xor tree
__global__ __launch_bounds__(256) void sm_sqnorm_kernel(const float* __restrict__ x, int n, int d, double* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;                                    // whole waves leave
    const float* __restrict__ r = x + (long long)row * d;
    double s = 0.0;
    for (int i = lane; i < d; i += 64) { const double v = (double)r[i]; s = fma(v, v, s); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[row] = s;
}

// v into the ascending list of the 8 smallest values seen
__device__ __forceinline__ void sm_insert(double (&best)[SM_KMAX], double v) {
    if (v < best[SM_KMAX - 1]) {
#pragma unroll
        for (int q = 0; q < SM_KMAX; ++q) {
            const double lo = fmin(best[q], v);
            v = fmax(best[q], v);
            best[q] = lo;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void sm_pair_kernel(const sm_args p) {
    __shared__ __attribute__((aligned(16))) float lds[SM_LDS];
    __shared__ double cn[SM_T], cr[SM_T];                    // the column tile's squared norms and radii; the final row sums
    float* const As = lds;
    float* const Bs = lds + SM_BK * SM_P;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhi = lane >> 5;
    const int m0 = blockIdx.x * SM_T;
    const int32_t* __restrict__ ai = MODE == SM_POLY3 ? p.ai + (long long)blockIdx.y * p.n : nullptr;
    const int32_t* __restrict__ bi = MODE == SM_POLY3 ? p.bi + (long long)blockIdx.y * p.m : nullptr;

    // staging: thread (lr = tid >> 3, kq = tid & 7) moves k 4 kq .. 4 kq + 3 of rows lr + 32 e -- eight lanes read the 128
    // contiguous bytes of one row's k-tile.  A row past the end reads row 0 instead: its products land in accumulator rows /
    // columns that no scan looks at, so nothing has to be zeroed and no load sits under a per-lane condition.
    const int kq = tid & 7, lr = tid >> 3;
    auto row_ptr = [&](const float* base, const int32_t* idx, int r, int rows, int pool) {
        long long src = 0;
        if (r < rows) {
            src = r;
            if (MODE == SM_POLY3) { const int v = idx[r]; src = v < 0 ? 0 : (v >= pool ? pool - 1 : v); }
        }
        return base + src * p.d + kq * 4;
    };
    const float* pa[4];
    const float* pb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) pa[e] = row_ptr(p.a, ai, m0 + lr + 32 * e, p.n, p.pool_a);

    // the scanning thread's row and its state
    const int srow = m0 + tid;
    const bool scans = tid < SM_T && srow < p.n;
    double my_n = 0.0, sum = 0.0, best[SM_KMAX];
    bool hit = false;
    if (MODE != SM_POLY3 && scans) my_n = p.na[srow];
#pragma unroll
    for (int q = 0; q < SM_KMAX; ++q) best[q] = __builtin_inf();
    const double dd = (double)p.d;

    float4 ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ra[e] = *reinterpret_cast<const float4*>(pa[e] + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[e] = *reinterpret_cast<const float4*>(pb[e] + k0);
    };
    auto store = [&]() {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float* da = As + (kq * 4) * SM_P + lr + 32 * e;
            float* db = Bs + (kq * 4) * SM_P + lr + 32 * e;
            da[0] = ra[e].x, da[SM_P] = ra[e].y, da[2 * SM_P] = ra[e].z, da[3 * SM_P] = ra[e].w;
            db[0] = rb[e].x, db[SM_P] = rb[e].y, db[2 * SM_P] = rb[e].z, db[3 * SM_P] = rb[e].w;
        }
    };

    const int nkt = p.d / SM_BK;
    for (int n0 = 0; n0 < p.m; n0 += SM_T) {
#pragma unroll
        for (int e = 0; e < 4; ++e) pb[e] = row_ptr(p.b, bi, n0 + lr + 32 * e, p.m, p.pool_b);
        __syncthreads();                                     // the previous tile's scans have read cn / cr
        if (MODE != SM_POLY3 && tid < SM_T) {                // read by the scans below, behind at least two barriers
            const int c = n0 + tid;
            cn[tid] = c < p.m ? p.nb[c] : 0.0;
            if (MODE == SM_HITS) cr[tid] = c < p.m ? p.rb[c] : 0.0;
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        load(0);
        for (int kt = 0; kt < nkt; ++kt) {
            __syncthreads();                                 // the previous k-tile's fragments / the previous scan are read
            store();
            __syncthreads();
            if (kt + 1 < nkt) load((kt + 1) * SM_BK);        // in flight while this k-tile multiplies
#pragma unroll
            for (int kk = 0; kk < SM_BK / 2; ++kk) {
                const int k = kk * 2 + lhi;                  // A[i = lane & 31][k = lane >> 5], B[k][j = lane & 31]
                float af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = As[k * SM_P + wm * 64 + i * 32 + l31];
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = Bs[k * SM_P + wn * 64 + j * 32 + l31];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }

        // the tile, 64 columns at a time: the waves of column half h write [row][column] (D: column = lane & 31, row =
        // (e & 3) + 8 (e >> 2) + 4 (lane >> 5)), then thread r scans row r in column order
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __syncthreads();
            if (wn == h) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e)
                            lds[(wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhi) * SM_HP + j * 32 + l31] = acc[i][j][e];
            }
            __syncthreads();
            if (scans) {
                const int c0 = n0 + h * 64;
                const int cend = p.m - c0 < 64 ? p.m - c0 : 64;
                for (int c = 0; c < cend; ++c) {
                    if (p.same && c0 + c == srow) continue;
                    const double dot = (double)lds[tid * SM_HP + c];
                    if (MODE == SM_POLY3) {
                        const double v = dot / dd + 1.0;
                        sum += v * v * v;
                    } else {
                        const double dist = fmax(0.0, my_n + cn[h * 64 + c] - 2.0 * dot);
                        if (MODE == SM_KNN) sm_insert(best, dist);
                        else hit = hit || dist <= cr[h * 64 + c];
                    }
                }
            }
        }
        if (MODE == SM_HITS) {                               // every row of the block is inside some ball: the rest cannot change it
            if (__syncthreads_and(hit || !scans)) break;
        }
    }

    if (MODE == SM_KNN && scans) {
        double r = best[0];
#pragma unroll
        for (int q = 1; q < SM_KMAX; ++q) r = (q == p.k - 1) ? best[q] : r;
        p.out[srow] = r;
    }
    if (MODE == SM_HITS && scans) p.hit[srow] = hit ? 1 : 0;
    if (MODE == SM_POLY3) {                                  // the block's 128 row sums, added in row order by one thread
        __syncthreads();
        if (tid < SM_T) cn[tid] = scans ? sum : 0.0;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int r = 0; r < SM_T; ++r) t += cn[r];
            p.out[(long long)blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    }
}

// sums[s][w] = the nblk partials of (sum w, subset s) in block order
__global__ __launch_bounds__(256) void sm_poly3_finish_kernel(const double* __restrict__ part, int subsets, int nblk,
                                                             double* __restrict__ sums) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= subsets * 3) return;
    const int s = t / 3, w = t - 3 * s;
    const double* __restrict__ src = part + ((long long)w * subsets + s) * nblk;
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) acc += src[b];
    sums[t] = acc;
}

bool sm_al16(const void* p) { return ((uintptr_t)p % 16) == 0; }
int sm_blocks(int rows) { return (rows + SM_T - 1) / SM_T; }

void sm_sqnorm(const float* x, int n, int d, double* out, hipStream_t s) {
    hipLaunchKernelGGL(sm_sqnorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, n, d, out);
}

}  // namespace

extern "C" int64_t xmc_sample_metrics_ws_bytes(int32_t n, int32_t m, int32_t d, int32_t subsets) {
    if (n < 1 || m < 0 || d < 32 || d % 32 != 0 || subsets < 0 || subsets > 65535) return XMC_EINVAL;
    const int64_t norms = (int64_t)n + m;
    const int64_t parts = 3 * (int64_t)subsets * sm_blocks(n > m ? n : m);
    return (((norms > parts ? norms : parts) * 8) + 15) & ~(int64_t)15;
}

extern "C" int xmc_knn_radii(const float* x, int32_t n, int32_t d, int32_t k, double* radii2, void* ws, void* stream) {
    XMC_REQUIRE(x && radii2 && ws);
    XMC_REQUIRE(n >= 1 && d >= 32 && d % 32 == 0 && k >= 1 && k <= SM_KMAX && k < n);
    XMC_REQUIRE(sm_al16(x) && sm_al16(radii2) && sm_al16(ws));
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* norms = static_cast<double*>(ws);
    sm_sqnorm(x, n, d, norms, s);
    sm_args a{};
    a.a = x, a.b = x, a.na = norms, a.nb = norms, a.out = radii2;
    a.n = n, a.m = n, a.d = d, a.k = k, a.same = 1;
    hipLaunchKernelGGL(sm_pair_kernel<SM_KNN>, dim3((unsigned)sm_blocks(n)), dim3(256), 0, s, a);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_ball_hits(const float* a, int32_t n, const float* b, const double* radii2_b, int32_t m, int32_t d,
                             uint8_t* hit, void* ws, void* stream) {
    XMC_REQUIRE(a && b && radii2_b && hit && ws);
    XMC_REQUIRE(n >= 1 && m >= 1 && d >= 32 && d % 32 == 0);
    XMC_REQUIRE(sm_al16(a) && sm_al16(b) && sm_al16(radii2_b) && sm_al16(hit) && sm_al16(ws));
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* norms = static_cast<double*>(ws);
    sm_sqnorm(a, n, d, norms, s);
    sm_sqnorm(b, m, d, norms + n, s);
    sm_args g{};
    g.a = a, g.b = b, g.na = norms, g.nb = norms + n, g.rb = radii2_b, g.hit = hit;
    g.n = n, g.m = m, g.d = d;
    hipLaunchKernelGGL(sm_pair_kernel<SM_HITS>, dim3((unsigned)sm_blocks(n)), dim3(256), 0, s, g);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_poly3_sums(const float* x, int32_t nx, const int32_t* xi, const float* y, int32_t ny, const int32_t* yi,
                              int32_t subsets, int32_t msub, int32_t d, double* sums, void* ws, void* stream) {
    XMC_REQUIRE(x && xi && y && yi && sums && ws);
    XMC_REQUIRE(nx >= 1 && ny >= 1 && subsets >= 1 && subsets <= 65535 && msub >= 2 && d >= 32 && d % 32 == 0);
    XMC_REQUIRE(sm_al16(x) && sm_al16(y) && sm_al16(xi) && sm_al16(yi) && sm_al16(sums) && sm_al16(ws));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = sm_blocks(msub);
    double* part = static_cast<double*>(ws);
    for (int w = 0; w < 3; ++w) {                            // sum over p != q of k(x, x), of k(y, y); sum over all p, q of k(x, y)
        sm_args g{};
        g.a = w == 1 ? y : x, g.ai = w == 1 ? yi : xi, g.pool_a = w == 1 ? ny : nx;
        g.b = w == 0 ? x : y, g.bi = w == 0 ? xi : yi, g.pool_b = w == 0 ? nx : ny;
        g.out = part + (long long)w * subsets * nblk;
        g.n = msub, g.m = msub, g.d = d, g.same = w < 2;
        hipLaunchKernelGGL(sm_pair_kernel<SM_POLY3>, dim3((unsigned)nblk, (unsigned)subsets), dim3(256), 0, s, g);
    }
    hipLaunchKernelGGL(sm_poly3_finish_kernel, dim3((unsigned)((subsets * 3 + 255) / 256)), dim3(256), 0, s, (const double*)part,
                       (int)subsets, nblk, sums);
    XMC_LAUNCH_RET();
}
