// config.skip_nonfinite_updates: the verdict of a half step -- does anything it is about to commit (gradient arenas, the new
// u0, the new BatchNorm running statistics) hold a NaN or an infinity? -- and the conditional copy that commits the small
// state buffers.  The guarded optimiser and accumulator launches read verdict[0] (pointwise.hip, spectral_batched.hip).
// With data-parallel replicas each rank's scan writes a LOCAL verdict, the locals are all-gathered, and
// xmc_verdict_merge turns the same rows into the same verdict and the same counters on every rank.
// Plain kernel launches on the caller's stream: a captured training step replays them, and the host never reads the verdict.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------- xmc_nonfinite_verdict
// Stage 1: every segment is cut into chunks of NFG_CHUNK elements; the chunks of all segments are numbered in table order and
// dealt round-robin to the workgroups (the pattern of xmc_segment_sumsq, train_stats.hip).  Segment bases are 16-byte aligned, so
// every chunk starts on a 16-byte boundary: 8 16-byte loads in flight per thread, and only a segment's last chunk has a scalar
// tail of up to 3 elements.  A workgroup counts the bad elements of ALL its chunks and remembers the first segment that held
// one; the pair goes to the workgroup's own slot of the workspace.  Stage 2: one workgroup adds the slots (integer adds and a
// minimum: any order gives the same bits), writes the verdict and advances the counters.  No atomics.
constexpr int NFG_THREADS = 256;
constexpr int NFG_VECS = 8;                              // 16-byte loads in flight per thread
constexpr int NFG_CHUNK = NFG_THREADS * NFG_VECS * 4;    // elements per workgroup trip
constexpr int NFG_GRID = 1024;                           // 4 workgroups per CU
constexpr int NFG_NONE = 0x7fffffff;

struct nfg_table {
    const uint32_t* p[XMC_NONFINITE_MAX_SEGMENTS];
    long long n[XMC_NONFINITE_MAX_SEGMENTS];
};

struct nfg_partial {
    long long bad;
    long long first;                                     // index of the first segment with a bad element, or NFG_NONE
};

// exponent bits all ones: NaN, +inf, -inf
__device__ __forceinline__ int bad_bits(uint32_t x) { return (x & 0x7f800000u) == 0x7f800000u; }

// the persistent counters behind a verdict: [0] skipped in total, [1] the current run, [2] the longest run (all saturating)
__device__ __forceinline__ void advance_counters(bool bad, int* __restrict__ counters) {
    if (bad) {
        const int total = counters[0], run = counters[1];
        counters[0] = total < 2147483647 ? total + 1 : total;
        const int r = run < 2147483647 ? run + 1 : run;
        counters[1] = r;
        if (r > counters[2]) counters[2] = r;
    } else {
        counters[1] = 0;
    }
}

__global__ __launch_bounds__(NFG_THREADS) void nonfinite_scan_kernel(nfg_table t, int nseg, nfg_partial* __restrict__ ws) {
    __shared__ long long s_bad[NFG_THREADS / 64];
    __shared__ int s_first[NFG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long grid = gridDim.x;
    long long bad = 0;
    int first = NFG_NONE;
    long long base = 0;                                  // chunks of the segments in front of this one
    for (int s = 0; s < nseg; ++s) {
        const uint32_t* __restrict__ x = t.p[s];
        const long long len = t.n[s];
        const long long chunks = (len + NFG_CHUNK - 1) / NFG_CHUNK;
        int seg_bad = 0;
        // this workgroup's chunks of the segment: base + c = blockIdx.x (mod grid)
        for (long long c = ((long long)blockIdx.x - base % grid + grid) % grid; c < chunks; c += grid) {
            const long long lo = c * NFG_CHUNK;
            const long long hi = lo + NFG_CHUNK < len ? lo + NFG_CHUNK : len;
            const long long nvec = (hi - lo) >> 2;       // <= NFG_THREADS * NFG_VECS
            const uint4* __restrict__ body = reinterpret_cast<const uint4*>(x + lo);
            uint4 v[NFG_VECS];
#pragma unroll
            for (int i = 0; i < NFG_VECS; ++i) {
                const long long idx = tid + (long long)i * NFG_THREADS;
                v[i] = idx < nvec ? body[idx] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int i = 0; i < NFG_VECS; ++i) seg_bad += bad_bits(v[i].x) + bad_bits(v[i].y) + bad_bits(v[i].z) + bad_bits(v[i].w);
            const long long tail = lo + (nvec << 2);     // up to 3 elements behind the last whole vector
            if (tail + tid < hi) seg_bad += bad_bits(x[tail + tid]);
        }
        if (seg_bad) {
            bad += seg_bad;
            first = s < first ? s : first;
        }
        base += chunks;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_down(bad, o, 64);
        const int f = __shfl_down(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_bad[wave] = bad;
        s_first[wave] = first;
    }
    __syncthreads();
    if (tid == 0) {
        nfg_partial r;
        r.bad = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
        int f = s_first[0];
        for (int w = 1; w < NFG_THREADS / 64; ++w) f = s_first[w] < f ? s_first[w] : f;
        r.first = f;
        ws[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(NFG_THREADS) void nonfinite_finish_kernel(const nfg_partial* __restrict__ ws, int nparts,
                                                                       int* __restrict__ verdict, int* __restrict__ counters) {
    __shared__ long long s_bad[NFG_THREADS / 64];
    __shared__ int s_first[NFG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long bad = 0;
    int first = NFG_NONE;
    for (int i = tid; i < nparts; i += NFG_THREADS) {
        const nfg_partial r = ws[i];
        bad += r.bad;
        first = (int)r.first < first ? (int)r.first : first;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_down(bad, o, 64);
        const int f = __shfl_down(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_bad[wave] = bad;
        s_first[wave] = first;
    }
    __syncthreads();
    if (tid == 0) {
        bad = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
        first = s_first[0];
        for (int w = 1; w < NFG_THREADS / 64; ++w) first = s_first[w] < first ? s_first[w] : first;
        verdict[0] = bad > 0 ? 1 : 0;
        verdict[1] = bad > 2147483647LL ? 2147483647 : (int)bad;
        verdict[2] = bad > 0 ? first : -1;
        verdict[3] = 0;
        advance_counters(bad > 0, counters);
    }
}

// ---------------------------------------------------------------------------------------------- xmc_verdict_merge
// One workgroup over the all-gathered local verdicts rows[w][4] of the replicas: every rank reads the same rows
// and writes the same verdict and the same counters.  Integer adds and a minimum: any order gives the same bits.  No atomics.
__global__ __launch_bounds__(NFG_THREADS) void verdict_merge_kernel(const int* __restrict__ rows, int w, int* __restrict__ verdict,
                                                                    int* __restrict__ counters) {
    __shared__ long long s_bad[NFG_THREADS / 64];
    __shared__ int s_first[NFG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long bad = 0;                                   // sum of the ranks' counts: w < 2^29 values below 2^31
    int first = NFG_NONE;                                // the lowest rank with a bad verdict
    for (int r = tid; r < w; r += NFG_THREADS) {
        bad += rows[4 * (long long)r + 1];
        if (rows[4 * (long long)r] != 0 && r < first) first = r;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_down(bad, o, 64);
        const int f = __shfl_down(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_bad[wave] = bad;
        s_first[wave] = first;
    }
    __syncthreads();
    if (tid == 0) {
        bad = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
        first = s_first[0];
        for (int k = 1; k < NFG_THREADS / 64; ++k) first = s_first[k] < first ? s_first[k] : first;
        const bool any = first != NFG_NONE;
        verdict[0] = any ? 1 : 0;
        verdict[1] = bad > 2147483647LL ? 2147483647 : (int)bad;
        verdict[2] = any ? rows[4 * (long long)first + 2] : -1;
        verdict[3] = any ? first : 0;
        advance_counters(any, counters);
    }
}

// total number of stage-1 chunks of a HOST length table, or -1 when a length is negative
long long host_chunks(const int64_t* n_host, int32_t nseg) {
    long long total = 0;
    for (int s = 0; s < nseg; ++s) {
        if (n_host[s] < 0) return -1;
        total += ((long long)n_host[s] + NFG_CHUNK - 1) / NFG_CHUNK;
    }
    return total;
}

inline int grid_of(long long chunks) { return chunks < 1 ? 1 : (chunks < NFG_GRID ? (int)chunks : NFG_GRID); }

// ------------------------------------------------------------------------------------------------------ xmc_commit_if
template <bool VEC>
__global__ __launch_bounds__(256) void commit_if_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n,
                                                        const int* __restrict__ verdict) {
    if (verdict[0] != 0) return;                         // the half step is skipped: dst keeps what it held
    const long long stride = (long long)gridDim.x * 256;
    if constexpr (VEC) {
        const long long n4 = n >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride)
            reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
        if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[(n4 << 2) + threadIdx.x] = src[(n4 << 2) + threadIdx.x];
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = src[i];
    }
}

}  // namespace

extern "C" int64_t xmc_nonfinite_verdict_workspace_bytes(const int64_t* n_host, int32_t nseg) {
    XMC_REQUIRE(n_host && nseg >= 1 && nseg <= XMC_NONFINITE_MAX_SEGMENTS);
    const long long total = host_chunks(n_host, nseg);
    XMC_REQUIRE(total >= 0);
    return (int64_t)sizeof(nfg_partial) * grid_of(total);
}

extern "C" int xmc_nonfinite_verdict(const float* const* ptrs, const int64_t* n_host, int32_t nseg, int32_t* verdict,
                                     int32_t* counters, void* ws, int64_t ws_bytes, void* stream) {
    XMC_REQUIRE(ptrs && n_host && nseg >= 1 && nseg <= XMC_NONFINITE_MAX_SEGMENTS && verdict && counters && ws);
    XMC_REQUIRE(((uintptr_t)verdict % 4) == 0 && ((uintptr_t)counters % 4) == 0 && ((uintptr_t)ws % 16) == 0);
    const long long total = host_chunks(n_host, nseg);
    XMC_REQUIRE(total >= 0);
    nfg_table t;
    for (int s = 0; s < XMC_NONFINITE_MAX_SEGMENTS; ++s) {
        t.p[s] = s < nseg ? reinterpret_cast<const uint32_t*>(ptrs[s]) : nullptr;
        t.n[s] = s < nseg ? (long long)n_host[s] : 0;
        XMC_REQUIRE(s >= nseg || n_host[s] == 0 || (ptrs[s] && ((uintptr_t)ptrs[s] % 16) == 0));
    }
    const int grid = grid_of(total);
    XMC_REQUIRE(ws_bytes >= (int64_t)sizeof(nfg_partial) * grid);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nonfinite_scan_kernel, dim3(grid), dim3(NFG_THREADS), 0, s, t, (int)nseg, static_cast<nfg_partial*>(ws));
    hipLaunchKernelGGL(nonfinite_finish_kernel, dim3(1), dim3(NFG_THREADS), 0, s, static_cast<const nfg_partial*>(ws), grid, verdict,
                       counters);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_verdict_merge(const int32_t* rows, int32_t w, int32_t* verdict, int32_t* counters, void* stream) {
    XMC_REQUIRE(rows && verdict && counters && w >= 1 && 4 * (int64_t)w <= 2147483647LL);
    XMC_REQUIRE(((uintptr_t)rows % 4) == 0 && ((uintptr_t)verdict % 4) == 0 && ((uintptr_t)counters % 4) == 0);
    hipLaunchKernelGGL(verdict_merge_kernel, dim3(1), dim3(NFG_THREADS), 0, static_cast<hipStream_t>(stream), rows, (int)w, verdict,
                       counters);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_commit_if(float* dst, const float* src, int64_t n, const int32_t* verdict, void* stream) {
    XMC_REQUIRE(dst && src && n > 0 && verdict && ((uintptr_t)verdict % 4) == 0);
    XMC_REQUIRE(((uintptr_t)dst % 4) == 0 && ((uintptr_t)src % 4) == 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec = ((uintptr_t)dst % 16) == 0 && ((uintptr_t)src % 16) == 0;
    const long long work = vec ? n / 4 + 1 : (long long)n;
    long long blocks = (work + 255) / 256;
    blocks = blocks > 4096 ? 4096 : blocks;
    if (vec)
        hipLaunchKernelGGL((commit_if_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, s, dst, src, (long long)n, verdict);
    else
        hipLaunchKernelGGL((commit_if_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, s, dst, src, (long long)n, verdict);
    XMC_LAUNCH_RET();
}
