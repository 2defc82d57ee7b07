// Device-resident dataset cache (libml/device_cache.py, config.device_dataset_cache): one launch builds a training batch from the
// resized, unflipped images and the caption tables kept in HBM, following a plan of integers the host drew -- per example: cache
// slot, caption, left-right flip, the reflect-shift (aug_dy, aug_dx) and the flip of augmentation.augment.  Pure data movement:
// every output element has exactly one writer, nothing is accumulated, no atomics; the bits are those of COCODataset.preprocess.
#include "common.h"

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_MAX_BLOCKS = 2048;      // 8 workgroups per CU; the rest of the work is walked with a grid stride

struct cg_args {
    const float* img;                    // [slots][h][w][3]
    const float* emb;                    // [slots][s][t][e]
    const float* sent;                   // [slots][s][e]
    const float* mlen;                   // [slots][s]
    const int32_t* plan;                 // [n][XMC_CACHE_PLAN_STRIDE]
    float* image;
    float* image_aug;                    // may be NULL
    float* embedding;
    float* sentence;
    float* max_len;
    long long slots;
    int h, w, s, t, e, pad;
};

// np.pad(mode="reflect") index of i in [-pad, L - 1 + pad], pad < L
__device__ __forceinline__ int reflect(int i, int L) { return i < 0 ? -i : (i >= L ? 2 * (L - 1) - i : i); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (x, n): blockIdx.y is the example; its work is cut into units of 16 bytes of OUTPUT -- four floats of an image row (the
// rows of `image`, then those of `image_aug`), one float4 of the caption's word embeddings, one of its sentence feature, and a
// last unit for max_len -- walked by the example's gridDim.x workgroups with a grid stride.  Consecutive lanes write consecutive
// float4s and read the same (mirrored: the reversed) run of the source row, so both sides are whole cache lines.  Offsets into
// the cache arrays are 64-bit (the 128-px COCO image cache is 4.07 G floats); per-example unit counts fit an int (checked on the host).
__global__ __launch_bounds__(CG_THREADS) void cache_gather_kernel(cg_args a) {
    const int n = blockIdx.y;
    const int32_t* __restrict__ p = a.plan + (long long)n * XMC_CACHE_PLAN_STRIDE;
    // the launch validated the caller's HOST copy of the plan; a device copy that differs must not index outside the cache
    long long slot = p[0];
    slot = slot < 0 ? 0 : (slot >= a.slots ? a.slots - 1 : slot);
    const int cap = clampi(p[1], 0, a.s - 1);
    const bool flip = p[2] != 0, aflip = p[5] != 0;
    const int dy = clampi(p[3], 0, 2 * a.pad) - a.pad, dx = clampi(p[4], 0, 2 * a.pad) - a.pad;

    const int H = a.h, W = a.w, rowf = 3 * W, chunks = (rowf + 3) >> 2;
    const bool vec = (rowf & 3) == 0;                        // rows start on 16-byte boundaries
    const int u_img = H * chunks, u_rows = a.image_aug ? 2 * u_img : u_img;
    const int te4 = (a.t * a.e) >> 2, e4 = a.e >> 2;
    const int u_emb = u_rows + te4, u_sent = u_emb + e4, total = u_sent + 1;
    const float* __restrict__ simg = a.img + slot * ((long long)H * rowf);
    const long long crow = slot * a.s + cap;                 // row of the caption tables

    for (int u = blockIdx.x * CG_THREADS + threadIdx.x; u < total; u += gridDim.x * CG_THREADS) {
        if (u < u_rows) {
            const bool aug = u >= u_img;
            const int v = aug ? u - u_img : u;
            const int y = v / chunks, j0 = (v - y * chunks) << 2;
            float* __restrict__ drow = (aug ? a.image_aug : a.image) + ((long long)n * H + y) * rowf;
            const float* __restrict__ srow = simg + (long long)(aug ? reflect(y + dy, H) : y) * rowf;
            float val[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec && !aug && !flip) {
                const float4 q = *reinterpret_cast<const float4*>(srow + j0);
                val[0] = q.x, val[1] = q.y, val[2] = q.z, val[3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j0 + k;
                    if (j < rowf) {
                        const int x = j / 3, c = j - 3 * x;
                        const int xi = aug ? reflect((aflip ? W - 1 - x : x) + dx, W) : x;      // column of `image`
                        val[k] = srow[(flip ? W - 1 - xi : xi) * 3 + c];
                    }
                }
            }
            if (vec) {
                *reinterpret_cast<float4*>(drow + j0) = make_float4(val[0], val[1], val[2], val[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k < rowf) drow[j0 + k] = val[k];
            }
        } else if (u < u_emb) {
            const int i = u - u_rows;
            reinterpret_cast<float4*>(a.embedding)[(long long)n * te4 + i] = reinterpret_cast<const float4*>(a.emb)[crow * te4 + i];
        } else if (u < u_sent) {
            const int i = u - u_emb;
            reinterpret_cast<float4*>(a.sentence)[(long long)n * e4 + i] = reinterpret_cast<const float4*>(a.sent)[crow * e4 + i];
        } else {
            a.max_len[n] = a.mlen[crow];
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int xmc_cache_plan_check(const int32_t* plan_host, int32_t n, int64_t slots, int32_t s, int32_t h, int32_t w, int32_t pad) {
    XMC_REQUIRE(plan_host && n >= 1 && slots >= 1 && s >= 1 && pad >= 0 && h > pad && w > pad);
    for (int i = 0; i < n; ++i) {
        const int32_t* p = plan_host + (size_t)i * XMC_CACHE_PLAN_STRIDE;
        XMC_REQUIRE(p[0] >= 0 && (int64_t)p[0] < slots);
        XMC_REQUIRE(p[1] >= 0 && p[1] < s);
        XMC_REQUIRE(p[3] >= 0 && p[3] <= 2 * pad && p[4] >= 0 && p[4] <= 2 * pad);
    }
    return XMC_OK;
}

extern "C" int xmc_cache_gather(const float* img, const float* emb, const float* sent, const float* mlen, int64_t slots,
                                const int32_t* plan, const int32_t* plan_host, float* image, float* image_aug, float* embedding,
                                float* sentence, float* max_len, int32_t n, int32_t h, int32_t w, int32_t s, int32_t t, int32_t e,
                                int32_t pad, void* stream) {
    XMC_REQUIRE(img && emb && sent && mlen && plan && image && embedding && sentence && max_len);
    XMC_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && s >= 1 && t >= 1 && e >= 4 && (e % 4) == 0 && pad >= 0);
    XMC_REQUIRE(xmc_cache_plan_check(plan_host, n, slots, s, h, w, pad) == XMC_OK);
    XMC_REQUIRE(aligned16(img) && aligned16(emb) && aligned16(sent) && aligned16(image) && aligned16(image_aug) &&
                aligned16(embedding) && aligned16(sentence));
    XMC_REQUIRE(((uintptr_t)mlen % 4) == 0 && ((uintptr_t)max_len % 4) == 0 && ((uintptr_t)plan % 4) == 0);
    const long long chunks = (3LL * w + 3) / 4;
    const long long total = (image_aug ? 2 : 1) * h * chunks + ((long long)t * e + e) / 4 + 1;       // units of one example
    XMC_REQUIRE(total < (1LL << 30) && (long long)t * e < (1LL << 31));          // the kernel's per-example unit indices are ints
    cg_args a;
    a.img = img, a.emb = emb, a.sent = sent, a.mlen = mlen, a.plan = plan;
    a.image = image, a.image_aug = image_aug, a.embedding = embedding, a.sentence = sentence, a.max_len = max_len;
    a.slots = slots, a.h = h, a.w = w, a.s = s, a.t = t, a.e = e, a.pad = pad;
    long long gx = (total + CG_THREADS - 1) / CG_THREADS;
    const long long cap = CG_MAX_BLOCKS / n > 0 ? CG_MAX_BLOCKS / n : 1;
    gx = gx < cap ? gx : cap;
    hipLaunchKernelGGL(cache_gather_kernel, dim3((unsigned)gx, (unsigned)n), dim3(CG_THREADS), 0, static_cast<hipStream_t>(stream), a);
    XMC_LAUNCH_RET();
}
