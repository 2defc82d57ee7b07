// In-graph training statistics (train_statistics.TrainStatistics, config.train_statistics): per-tensor sums of squares of the
// parameter / gradient arenas and the per-step scalar vector (head statistics, logit summary, global norms, sigma extrema).
// Both entry points are plain kernel launches on the caller's stream: a captured training step replays them.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------- xmc_segment_sumsq
// Stage 1: every segment is cut into pieces of SEG_PIECE elements; the pieces of all segments are numbered in table order and
// dealt round-robin to the workgroups, so that one 20 M-element convolution kernel and three hundred 64-element biases both
// spread over the chip.  A piece's 256 threads each own a fixed set of its elements (products and adds in float64, in a fixed
// order), the 256 partial sums meet in a fixed shuffle tree, and the piece's (sum, non-finite count) goes to its own slot of the
// workspace.  Stage 2: one wave per segment adds the segment's slots, again in a fixed order.  No atomics anywhere: two runs over
// the same buffer and table are bit-identical.
constexpr int SEG_PIECE = 8192;          // = SEG_THREADS * SEG_VECS * 4
constexpr int SEG_THREADS = 256;
constexpr int SEG_VECS = 8;              // 16-byte loads in flight per thread
constexpr int SEG_GRID = 1024;           // 4 workgroups per CU

struct seg_partial {
    double sum;
    long long bad;
};

__device__ __forceinline__ bool not_finite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }      // NaN and +-inf

__device__ __forceinline__ void clamp_segment(const long long* __restrict__ segs, int s, long long n, long long& off, long long& len) {
    off = segs[2 * s];
    len = segs[2 * s + 1];
    // the launch validated the caller's HOST copy of the table; a device copy that differs must not index outside the buffer
    off = off < 0 ? 0 : (off > n ? n : off);
    len = len < 0 ? 0 : (len > n - off ? n - off : len);
}

__global__ __launch_bounds__(SEG_THREADS) void segment_sumsq_pieces_kernel(const float* __restrict__ x, long long n,
                                                                           const long long* __restrict__ segs, int nseg,
                                                                           seg_partial* __restrict__ ws, long long npieces) {
    __shared__ double s_sum[SEG_THREADS / 64];
    __shared__ long long s_bad[SEG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long grid = gridDim.x;
    long long base = 0;                                      // pieces of the segments in front of this one
    for (int s = 0; s < nseg; ++s) {
        long long off, len;
        clamp_segment(segs, s, n, off, len);
        const long long pieces = (len + SEG_PIECE - 1) / SEG_PIECE;
        // this workgroup's pieces of the segment: base + p = blockIdx.x (mod grid)
        long long p = ((long long)blockIdx.x - base % grid + grid) % grid;
        for (; p < pieces && base + p < npieces; p += grid) {
            const long long lo = off + p * SEG_PIECE;
            const long long hi = (lo + SEG_PIECE < off + len) ? lo + SEG_PIECE : off + len;
            long long a = (lo + 3) & ~3LL;                   // first 16-byte boundary of the buffer inside the piece
            if (a > hi) a = hi;
            const long long nvec = (hi - a) >> 2;            // <= SEG_THREADS * SEG_VECS
            const float4* __restrict__ body = reinterpret_cast<const float4*>(x + a);
            float4 v[SEG_VECS];
#pragma unroll
            for (int i = 0; i < SEG_VECS; ++i) {
                const long long idx = tid + (long long)i * SEG_THREADS;
                v[i] = idx < nvec ? body[idx] : make_float4(0.f, 0.f, 0.f, 0.f);      // (0 * 0 adds nothing, exactly)
            }
            double acc = 0.0;
            long long bad = 0;
            if (lo + tid < a) {                              // up to 3 elements in front of the boundary
                const float e = x[lo + tid];
                acc = fma((double)e, (double)e, acc);
                bad += not_finite(e);
            }
#pragma unroll
            for (int i = 0; i < SEG_VECS; ++i) {
                const float e[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc = fma((double)e[j], (double)e[j], acc);
                    bad += not_finite(e[j]);
                }
            }
            const long long tail = a + (nvec << 2);          // up to 3 elements behind the last whole vector
            if (tail + tid < hi) {
                const float e = x[tail + tid];
                acc = fma((double)e, (double)e, acc);
                bad += not_finite(e);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {               // fixed tree inside the wave
                acc += __shfl_down(acc, o, 64);
                bad += __shfl_down(bad, o, 64);
            }
            if (lane == 0) {
                s_sum[wave] = acc;
                s_bad[wave] = bad;
            }
            __syncthreads();
            if (tid == 0) {
                seg_partial r;
                r.sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
                r.bad = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
                ws[base + p] = r;
            }
            __syncthreads();                                 // the next piece reuses s_sum / s_bad
        }
        base += pieces;
    }
}

__global__ __launch_bounds__(64) void segment_sumsq_final_kernel(const long long* __restrict__ segs, int nseg, long long n,
                                                                 const seg_partial* __restrict__ ws, long long npieces,
                                                                 double* __restrict__ sumsq, int* __restrict__ nonfinite) {
    const int s = blockIdx.x, lane = threadIdx.x;
    long long before = 0;                                    // integer adds: any order gives the same number
    for (int i = lane; i < s; i += 64) {
        long long off, len;
        clamp_segment(segs, i, n, off, len);
        before += (len + SEG_PIECE - 1) / SEG_PIECE;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    long long off, len;
    clamp_segment(segs, s, n, off, len);
    const long long pieces = (len + SEG_PIECE - 1) / SEG_PIECE;
    double acc = 0.0;
    long long bad = 0;
    for (long long p = lane; p < pieces && before + p < npieces; p += 64) {
        const seg_partial r = ws[before + p];
        acc += r.sum;
        bad += r.bad;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_down(acc, o, 64);
        bad += __shfl_down(bad, o, 64);
    }
    if (lane == 0) {
        sumsq[s] = acc;
        nonfinite[s] = bad > 2147483647LL ? 2147483647 : (int)bad;
    }
}

// total number of stage-1 pieces of a HOST table, or -1 when an entry is negative
long long host_pieces(const int64_t* segs_host, int32_t nseg, long long n) {
    long long total = 0;
    for (int s = 0; s < nseg; ++s) {
        const long long off = segs_host[2 * s], len = segs_host[2 * s + 1];
        if (off < 0 || len < 0) return -1;
        if (n >= 0 && (off > n || len > n - off)) return -1;
        total += (len + SEG_PIECE - 1) / SEG_PIECE;
    }
    return total;
}

// ---------------------------------------------------------------------------------------------------- xmc_train_stats
// One workgroup.  A few threads of wave 0 each produce one group of the XMC_TRAIN_STATS_N scalars (head statistics, logit
// summary, sigma extrema, one global norm each) with plain serial float64 sums; behind a barrier the vector is stored, added to
// the float64 running sums, the per-tensor tables are added to the window tables (one thread per tensor) and the call is
// counted.  Plain loads and stores: launches on one stream are ordered and nothing else touches the buffers.
__global__ __launch_bounds__(256) void train_stats_kernel(xmc_train_stats_args a) {
    __shared__ float s_vec[XMC_TRAIN_STATS_N];
    __shared__ int s_first[256];
    const int tid = threadIdx.x;
    if (tid < 5) {                                           // loss, accuracy, entropy of head `tid` (xmc_net.LOSS_SLOTS order)
        s_vec[3 * tid] = a.loss_vec[tid];
        s_vec[3 * tid + 1] = a.head_stats[2 * tid];
        s_vec[3 * tid + 2] = a.head_stats[2 * tid + 1];
    } else if (tid == 5) {                                   // D's logits: the real ones first
        double rs = 0.0, fs = 0.0;
        int rm = 0, fm = 0;
        for (int i = 0; i < a.b; ++i) {
            const float r = a.logits[i], f = a.logits[a.b + i];
            rs += (double)r;
            fs += (double)f;
            rm += r < 1.f;
            fm += f > -1.f;
        }
        s_vec[15] = (float)(rs / a.b);
        s_vec[16] = (float)(fs / a.b);
        s_vec[17] = (float)rm / (float)a.b;
        s_vec[18] = (float)fm / (float)a.b;
    } else if (tid == 6) {                                   // sigma of every spectrally-normalised weight: scal = {sigma, 1 / (sigma + eps)} pairs
        float lo = 0.f, hi = 0.f;
        for (int i = 0; i < a.n_sigma; ++i) {
            const float sg = a.scal[2 * i];
            lo = (i == 0 || sg < lo) ? sg : lo;
            hi = (i == 0 || sg > hi) ? sg : hi;
        }
        s_vec[23] = lo;
        s_vec[24] = hi;
    } else if (tid < 11) {                                   // 7: |grad D|, 8: |grad G|, 9: |param D|, 10: |param G|
        const int k = tid - 7;
        const double* t = k < 2 ? a.leaf_gsq : a.leaf_psq;
        const int lo = (k & 1) ? a.n_d : 0, hi = (k & 1) ? a.n_leaves : a.n_d;
        double sum = 0.0;
        for (int i = lo; i < hi; ++i) sum += t[i];
        const double scale = k == 0 ? (double)a.d_grad_scale : k == 1 ? (double)a.g_grad_scale : 1.0;
        s_vec[19 + k] = (float)(sqrt(sum) * fabs(scale));
    }
    int first = 0x7fffffff;
    for (int i = tid; i < a.n_leaves; i += 256) {
        const double sc = i < a.n_d ? (double)a.d_grad_scale : (double)a.g_grad_scale;
        const int bad = a.leaf_bad[i];
        a.win_gsq[i] += a.leaf_gsq[i] * (sc * sc);
        a.win_psq[i] += a.leaf_psq[i];
        a.win_bad[i] += (long long)bad;
        if (bad != 0 && i < first) first = i;
    }
    s_first[tid] = first;
    __syncthreads();
    if (tid < XMC_TRAIN_STATS_N) {
        const float x = s_vec[tid];
        a.vec[tid] = x;
        a.sums[tid] += (double)x;
    }
    if (tid == 0) {
        const int call = a.info[0] + 1;
        a.info[0] = call;
        if (a.info[1] == 0) {                                // the first call of the window whose gradients held a non-finite value
            int f = 0x7fffffff;
            for (int i = 0; i < 256; ++i) f = s_first[i] < f ? s_first[i] : f;
            if (f != 0x7fffffff) {
                a.info[1] = call;
                a.info[2] = f;
            }
        }
    }
}

}  // namespace

extern "C" int64_t xmc_segment_sumsq_ws_bytes(const int64_t* segs_host, int32_t nseg) {
    XMC_REQUIRE(segs_host && nseg >= 1);
    const long long total = host_pieces(segs_host, nseg, -1);
    XMC_REQUIRE(total >= 0);
    return (int64_t)sizeof(seg_partial) * (total > 0 ? total : 1);
}

extern "C" int xmc_segment_sumsq(const float* x, int64_t n, const int64_t* segs, const int64_t* segs_host, int32_t nseg,
                                 double* sumsq, int32_t* nonfinite, void* ws, int64_t ws_bytes, void* stream) {
    XMC_REQUIRE(x && n >= 0 && segs && segs_host && nseg >= 1 && sumsq && nonfinite && ws);
    XMC_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)segs % 8) == 0 && ((uintptr_t)sumsq % 8) == 0 &&
                ((uintptr_t)nonfinite % 4) == 0 && ((uintptr_t)ws % 16) == 0);
    const long long total = host_pieces(segs_host, nseg, n);             // every segment lies inside [0, n)
    XMC_REQUIRE(total >= 0 && ws_bytes >= (int64_t)sizeof(seg_partial) * (total > 0 ? total : 1));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (total > 0) {
        const int grid = total < SEG_GRID ? (int)total : SEG_GRID;
        hipLaunchKernelGGL(segment_sumsq_pieces_kernel, dim3(grid), dim3(SEG_THREADS), 0, s, x, (long long)n,
                           reinterpret_cast<const long long*>(segs), (int)nseg, static_cast<seg_partial*>(ws), total);
    }
    hipLaunchKernelGGL(segment_sumsq_final_kernel, dim3(nseg), dim3(64), 0, s, reinterpret_cast<const long long*>(segs), (int)nseg,
                       (long long)n, static_cast<const seg_partial*>(ws), total, sumsq, nonfinite);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_train_stats(const xmc_train_stats_args* a, void* stream) {
    XMC_REQUIRE(a && a->logits && a->b >= 1 && a->loss_vec && a->head_stats && a->n_sigma >= 0 && (a->scal || a->n_sigma == 0));
    XMC_REQUIRE(a->n_leaves >= 1 && a->n_d >= 0 && a->n_d <= a->n_leaves && a->leaf_gsq && a->leaf_psq && a->leaf_bad);
    XMC_REQUIRE(a->vec && a->sums && a->info && a->win_gsq && a->win_psq && a->win_bad);
    XMC_REQUIRE(((uintptr_t)a->leaf_gsq % 8) == 0 && ((uintptr_t)a->leaf_psq % 8) == 0 && ((uintptr_t)a->sums % 8) == 0 &&
                ((uintptr_t)a->win_gsq % 8) == 0 && ((uintptr_t)a->win_psq % 8) == 0 && ((uintptr_t)a->win_bad % 8) == 0);
    XMC_REQUIRE(((uintptr_t)a->logits % 4) == 0 && ((uintptr_t)a->scal % 4) == 0 && ((uintptr_t)a->loss_vec % 4) == 0 &&
                ((uintptr_t)a->head_stats % 4) == 0 && ((uintptr_t)a->leaf_bad % 4) == 0 && ((uintptr_t)a->vec % 4) == 0 &&
                ((uintptr_t)a->info % 4) == 0);
    hipLaunchKernelGGL(train_stats_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
    XMC_LAUNCH_RET();
}
