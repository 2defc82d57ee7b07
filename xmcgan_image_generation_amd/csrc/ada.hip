// config.ada_target: adaptive discriminator augmentation (libml/ada.py is the written specification).
//   xmc_ada_gate   -- the plan rows config.diff_augment applies in this half step: part g of a row keeps the drawn values iff
//                     its uniform is below p, which the kernel reads from the controller's state in device memory
//   xmc_ada_update -- the controller: counts the signs of D's real logits and, every `interval` half steps, moves p
//   xmc_ada_update_rows -- the controller with data-parallel replicas: the same update over the real halves of
//                     the all-gathered logit rows of every rank, so that every rank computes the same p
// Plain kernel launches on the caller's stream: a captured training step replays them, and the host never reads p.
// Both are exact (a select, integer counts, IEEE double arithmetic in a fixed order): bit-equal to the specification.
#include "common.h"

namespace {

constexpr int ADA_THREADS = 256;
constexpr int ADA_WAVES = ADA_THREADS / 64;

// ------------------------------------------------------------------------------------------------------- xmc_ada_gate
// One thread per output row.  Row r < b is the real row of sample r, row b + s the generated row of sample s; the plan and the
// uniforms are laid out [sample][real, generated][...].  Every output element has exactly one writer.
__global__ __launch_bounds__(ADA_THREADS) void ada_gate_kernel(const float4* __restrict__ plan, const float* __restrict__ u,
                                                               const double* __restrict__ state, float4* __restrict__ rows, int b) {
    const int r = blockIdx.x * ADA_THREADS + threadIdx.x;
    if (r >= 2 * b) return;
    const int half = r >= b ? 1 : 0;
    const int src = (r - half * b) * 2 + half;           // index of the (sample, half) pair in plan and u
    const double p = state[0];
    const float* __restrict__ uu = u + (long long)src * 5;
    const bool on0 = (double)uu[0] < p, on1 = (double)uu[1] < p, on2 = (double)uu[2] < p, on3 = (double)uu[3] < p,
               on4 = (double)uu[4] < p;
    float4 lo = plan[2 * src], hi = plan[2 * src + 1];   // [b, s, k, ty] [tx, y0, x0, c]
    lo.x = on0 ? lo.x : 0.0f;                            // IDENTITY_ROW = (0, 1, 1, 0, 0, 0, 0, 0)
    lo.y = on1 ? lo.y : 1.0f;
    lo.z = on2 ? lo.z : 1.0f;
    lo.w = on3 ? lo.w : 0.0f;
    hi.x = on3 ? hi.x : 0.0f;
    hi.y = on4 ? hi.y : 0.0f;
    hi.z = on4 ? hi.z : 0.0f;
    hi.w = on4 ? hi.w : 0.0f;
    rows[2 * r] = lo;
    rows[2 * r + 1] = hi;
}

// ----------------------------------------------------------------------------------------------------- xmc_ada_update
// One workgroup.  The three counts are integers: any reduction order gives the same bits.  Waves reduce with cross-lane moves,
// the four waves are added in index order through LDS, and lane 0 does the float64 tail.  No atomics.
// ROWS: `logit` is rows[w][2b] and the real halves rows[r][0 .. b) of all w rows are counted (n = w b <= 2^30 logits: the counts
// fit an int).  Without ROWS w is not read: one row.
template <bool ROWS>
__global__ __launch_bounds__(ADA_THREADS) void ada_update_kernel(const uint32_t* __restrict__ logit, int w, int b,
                                                                 double* __restrict__ state, double target, double images_to_full,
                                                                 int interval, double p_max) {
    __shared__ int s_pos[ADA_WAVES], s_neg[ADA_WAVES], s_fin[ADA_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = ROWS ? w * b : b;
    int pos = 0, neg = 0, fin = 0;
    for (int k = tid; k < n; k += ADA_THREADS) {         // the first b entries of a row: the real half
        const int r = ROWS ? k / b : 0;
        const uint32_t x = logit[(long long)r * 2 * b + (k - r * b)];
        const uint32_t mag = x & 0x7fffffffu;
        const int finite = mag < 0x7f800000u;            // exponent bits not all ones
        const int nonzero = finite && mag != 0u;         // (+-0 counts with sign 0; a denormal has a sign)
        fin += finite;
        pos += nonzero && !(x >> 31);
        neg += nonzero && (x >> 31);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pos += __shfl_down(pos, o, 64);
        neg += __shfl_down(neg, o, 64);
        fin += __shfl_down(fin, o, 64);
    }
    if (lane == 0) {
        s_pos[wave] = pos;
        s_neg[wave] = neg;
        s_fin[wave] = fin;
    }
    __syncthreads();
    if (tid == 0) {
        pos = neg = fin = 0;
        for (int w = 0; w < ADA_WAVES; ++w) {
            pos += s_pos[w];
            neg += s_neg[w];
            fin += s_fin[w];
        }
        double p = state[0];
        double sign_sum = state[1] + (double)(pos - neg);
        double count = state[2] + (double)fin;
        double ticks = state[3] + 1.0;
        if (ticks >= (double)interval) {
            if (count > 0.0) {
                const double r = sign_sum / count;
                const double sgn = (double)(r > target) - (double)(r < target);
                p = p + sgn * (count / images_to_full);  // (sgn is -1, 0 or 1: the product is exact, fused or not)
                p = p < 0.0 ? 0.0 : p;
                p = p > p_max ? p_max : p;
                state[0] = p;
                state[4] = r;
                state[5] = state[5] + 1.0;
            }
            sign_sum = count = ticks = 0.0;
        }
        state[1] = sign_sum;
        state[2] = count;
        state[3] = ticks;
    }
}

}  // namespace

extern "C" int xmc_ada_gate(const float* plan, const float* u, const double* state, float* rows, int32_t b, void* stream) {
    XMC_REQUIRE(plan && u && state && rows && b >= 1 && 2 * (int64_t)b <= 65535);
    XMC_REQUIRE(((uintptr_t)plan % 16) == 0 && ((uintptr_t)rows % 16) == 0 && ((uintptr_t)u % 4) == 0 && ((uintptr_t)state % 8) == 0);
    const int grid = (2 * b + ADA_THREADS - 1) / ADA_THREADS;
    hipLaunchKernelGGL(ada_gate_kernel, dim3(grid), dim3(ADA_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(plan), u, state, reinterpret_cast<float4*>(rows), (int)b);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_ada_update(const float* logit, int32_t b, double* state, double target, double images_to_full, int32_t interval,
                              double p_max, void* stream) {
    XMC_REQUIRE(logit && state && b >= 1 && interval >= 1);
    XMC_REQUIRE(((uintptr_t)logit % 4) == 0 && ((uintptr_t)state % 8) == 0);
    XMC_REQUIRE(target == target && images_to_full > 0.0 && p_max >= 0.0);
    hipLaunchKernelGGL((ada_update_kernel<false>), dim3(1), dim3(ADA_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t*>(logit), 1, (int)b, state, target, images_to_full, (int)interval, p_max);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_ada_update_rows(const float* rows, int32_t w, int32_t b, double* state, double target, double images_to_full,
                                   int32_t interval, double p_max, void* stream) {
    XMC_REQUIRE(rows && state && w >= 1 && b >= 1 && interval >= 1 && (int64_t)w * 2 * (int64_t)b <= 2147483647LL);
    XMC_REQUIRE(((uintptr_t)rows % 4) == 0 && ((uintptr_t)state % 8) == 0);
    XMC_REQUIRE(target == target && images_to_full > 0.0 && p_max >= 0.0);
    hipLaunchKernelGGL((ada_update_kernel<true>), dim3(1), dim3(ADA_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t*>(rows), (int)w, (int)b, state, target, images_to_full, (int)interval, p_max);
    XMC_LAUNCH_RET();
}
