// config.lecam_weight: the LeCam discriminator regulariser (libml/lecam.py is the written specification).
//   xmc_lecam -- one half step: adds 2 lambda / b * (logit - anchor) onto the gradient the hinge launch wrote, writes the
//                unweighted R, and moves the two anchors (moving averages of D's real / generated logits) in device memory
// A plain kernel launch on the caller's stream: a captured training step replays it, and the host never reads the anchors.
// Held BIT FOR BIT to the specification: IEEE double in a fixed order, the four sums included (lane j of 256 adds elements j,
// j + 256, ... in rising order; then the tree v[j] += v[j + s], s = 128 ... 1).  No double multiply may fuse with the add behind
// it: at -O3 hipcc contracts even __dadd_rn(__dmul_rn(a, a), b) into v_fmac_f64, so this file switches contraction off with the
// pragma below (checked in the disassembly: v_mul_f64 + v_add_f64 in the loop; the only v_fma_f64 left are the divisions' own).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LECAM_THREADS = 256;

__device__ __forceinline__ double lecam_tree(double* v, int tid) {
    __syncthreads();
#pragma unroll
    for (int s = LECAM_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) v[tid] = v[tid] + v[tid + s];
        __syncthreads();
    }
    return v[0];
}

// One workgroup.  Every lane reads the state before the first barrier; lane 0 writes it behind the last.  Element i of dld has one
// writer (lane i % 256).  No atomics.
// ROWS: `logit` is rows[w][2b]; X_R / X_F are the real / generated halves of all rows in rank order, n = w b elements each
// (element k = element k % b of row k / b), and only the elements of row `rank` have a slot in dld.  Without ROWS w and rank
// are not read: one row, n = b.
template <bool ROWS>
__global__ __launch_bounds__(LECAM_THREADS) void lecam_kernel(const float* __restrict__ logit, int w, int rank,
                                                              float* __restrict__ dld, int b, double* __restrict__ state,
                                                              float* __restrict__ loss, double lam, double decay, int start,
                                                              int one_sided) {
#pragma clang fp contract(off)
    __shared__ double s_rr[LECAM_THREADS], s_ff[LECAM_THREADS], s_r[LECAM_THREADS], s_f[LECAM_THREADS];
    __shared__ int s_bad[LECAM_THREADS];
    const int tid = threadIdx.x;
    const double a_r = state[0], a_f = state[1], ticks = state[2], updates = state[4];
    const int n = ROWS ? w * b : b;
    const double bb = (double)b, nn = (double)n;
    const bool warm = ticks < (double)start || updates == 0.0;   // (= not active: ticks >= start and updates > 0)
    const double c = (2.0 * lam) / bb;
    double rr = 0.0, ff = 0.0, sr = 0.0, sf = 0.0;
    int bad = 0;
    for (int k = tid; k < n; k += LECAM_THREADS) {
        const int r = ROWS ? k / b : 0, i = ROWS ? k - r * b : k;
        const float* __restrict__ row = logit + (long long)r * 2 * b;
        const float xr = row[i], xf = row[b + i];
        bad |= ((__float_as_uint(xr) & 0x7f800000u) == 0x7f800000u) | ((__float_as_uint(xf) & 0x7f800000u) == 0x7f800000u);
        const double real = (double)xr, fake = (double)xf;
        sr = sr + real;
        sf = sf + fake;
        if (!warm) {
            double dr = real - a_f, df = fake - a_r;
            if (one_sided) {
                dr = dr > 0.0 ? dr : 0.0;
                df = df < 0.0 ? df : 0.0;
            }
            const double pr = dr * dr, pf = df * df;
            rr = rr + pr;
            ff = ff + pf;
            if (!ROWS || r == rank) {
                const double tr = c * dr, tf = c * df;
                float gr = (float)((double)dld[i] + tr), gf = (float)((double)dld[b + i] + tf);
                gr = gr != gr ? __uint_as_float(0x7fc00000u) : gr;   // a written NaN is the canonical one
                gf = gf != gf ? __uint_as_float(0x7fc00000u) : gf;
                dld[i] = gr;
                dld[b + i] = gf;
            }
        }
    }
    s_rr[tid] = rr;
    s_ff[tid] = ff;
    s_r[tid] = sr;
    s_f[tid] = sf;
    s_bad[tid] = bad;
    const double sum_rr = lecam_tree(s_rr, tid), sum_ff = lecam_tree(s_ff, tid);
    const double sum_r = lecam_tree(s_r, tid), sum_f = lecam_tree(s_f, tid);
    if (tid == 0) {
        int any_bad = 0;
        for (int j = 0; j < LECAM_THREADS; ++j) any_bad |= s_bad[j];
        double r = 0.0;
        if (!warm) {
            r = (sum_rr + sum_ff) / nn;
            r = r != r ? __longlong_as_double(0x7ff8000000000000LL) : r;
        }
        state[3] = r;
        loss[0] = (float)r;
        if (!any_bad) {
            const double m_r = sum_r / nn, m_f = sum_f / nn;
            const double g = warm ? 0.0 : decay;
            const double k = 1.0 - g;
            const double gr = g * a_r, kr = k * m_r, gf = g * a_f, kf = k * m_f;
            state[0] = gr + kr;
            state[1] = gf + kf;
            state[4] = updates + 1.0;
        }
        state[2] = ticks + 1.0;
    }
}

}  // namespace

extern "C" int xmc_lecam(const float* logit, float* dld, int32_t b, double* state, float* loss, double lam, double decay,
                         int32_t start, int32_t one_sided, void* stream) {
    XMC_REQUIRE(logit && dld && state && loss && b >= 1 && 2 * (int64_t)b <= 2147483647LL);
    XMC_REQUIRE(((uintptr_t)logit % 4) == 0 && ((uintptr_t)dld % 4) == 0 && ((uintptr_t)loss % 4) == 0 && ((uintptr_t)state % 8) == 0);
    XMC_REQUIRE(lam >= 0.0 && lam <= 1.7976931348623157e308 && decay >= 0.0 && decay < 1.0 && start >= 0);
    XMC_REQUIRE(one_sided == 0 || one_sided == 1);
    hipLaunchKernelGGL((lecam_kernel<false>), dim3(1), dim3(LECAM_THREADS), 0, static_cast<hipStream_t>(stream), logit, 1, 0, dld,
                       (int)b, state, loss, lam, decay, (int)start, (int)one_sided);
    XMC_LAUNCH_RET();
}

extern "C" int xmc_lecam_rows(const float* rows, int32_t w, int32_t rank, float* dld, int32_t b, double* state, float* loss,
                              double lam, double decay, int32_t start, int32_t one_sided, void* stream) {
    XMC_REQUIRE(rows && dld && state && loss && w >= 1 && rank >= 0 && rank < w && b >= 1);
    XMC_REQUIRE((int64_t)w * 2 * (int64_t)b <= 2147483647LL);
    XMC_REQUIRE(((uintptr_t)rows % 4) == 0 && ((uintptr_t)dld % 4) == 0 && ((uintptr_t)loss % 4) == 0 && ((uintptr_t)state % 8) == 0);
    XMC_REQUIRE(lam >= 0.0 && lam <= 1.7976931348623157e308 && decay >= 0.0 && decay < 1.0 && start >= 0);
    XMC_REQUIRE(one_sided == 0 || one_sided == 1);
    hipLaunchKernelGGL((lecam_kernel<true>), dim3(1), dim3(LECAM_THREADS), 0, static_cast<hipStream_t>(stream), rows, (int)w,
                       (int)rank, dld, (int)b, state, loss, lam, decay, (int)start, (int)one_sided);
    XMC_LAUNCH_RET();
}
