// PNG scanline filtering for gfx950 (include/xmc_codec.h: xmc_png_filter_batch), bit-equal to libml/png.py: filter_rows_np.
//
//   launch 1  png_choose_kernel   one wave64 per image row: every lane walks the row's bytes at stride 64, forms the five
//             filtered values of each, sums their absolute values (read as signed); a shuffle reduction, and lane 0 stores
//             the id of the smallest sum (ties: the lowest id) as one int32 per row in the workspace
//   launch 2  png_write_kernel    one lane per aligned dword of the image's output stream (rows are 1 + 3 W bytes, so they
//             do not start on dwords): per byte its row, the row's id, the filtered value; one dword store
//
// Neighbours left of the row and above the image count as 0: they are loaded at a CLAMPED index and multiplied by 0, never
// loaded under a condition.
#include "codec_common.h"

namespace {

__device__ inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the five filtered bytes (0 .. 255) of byte i of row y
__device__ inline void filtered(const uint8_t* __restrict__ img, int nb, int y, int i, int f[5]) {
    const int has_left = i >= 3, has_up = y >= 1;
    const uint8_t* cur = img + (int64_t)y * nb;
    const uint8_t* prev = img + (int64_t)max(y - 1, 0) * nb;
    const int il = max(i - 3, 0);
    const int x = cur[i], a = cur[il] * has_left, b = prev[i] * has_up, c = prev[il] * (has_left & has_up);
    f[0] = x;
    f[1] = (x - a) & 0xff;
    f[2] = (x - b) & 0xff;
    f[3] = (x - ((a + b) >> 1)) & 0xff;
    f[4] = (x - paeth(a, b, c)) & 0xff;
}

__global__ __launch_bounds__(256) void png_choose_kernel(const uint8_t* __restrict__ px, const int64_t* __restrict__ desc,
                                                          int32_t* __restrict__ ids) {
    const int64_t* d = desc + (int64_t)blockIdx.y * XMC_CODEC_DESC_WORDS;
    const int w = (int)d[D_W], h = (int)d[D_H], nb = 3 * w;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int y = min(row, h - 1);                  // waves past the image redo its last row and store nothing
    const uint8_t* img = px + d[D_OUT];
    int cost[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < nb; i += 64) {
        int f[5];
        filtered(img, nb, y, i, f);
#pragma unroll
        for (int k = 0; k < 5; ++k) cost[k] += f[k] >= 128 ? 256 - f[k] : f[k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
        for (int off = 32; off > 0; off >>= 1) cost[k] += __shfl_down(cost[k], off, 64);
    if (lane == 0 && row < h) {
        int best = 0;
#pragma unroll
        for (int k = 1; k < 5; ++k) best = cost[k] < cost[best] ? k : best;
        ids[d[D_ROW] + row] = best;
    }
}

__global__ __launch_bounds__(256) void png_write_kernel(const uint8_t* __restrict__ px, const int64_t* __restrict__ desc,
                                                         const int32_t* __restrict__ ids, uint8_t* __restrict__ out) {
    const int64_t* d = desc + (int64_t)blockIdx.y * XMC_CODEC_DESC_WORDS;
    const int w = (int)d[D_W], h = (int)d[D_H], nb = 3 * w;
    const uint32_t stride = (uint32_t)nb + 1u, total = stride * (uint32_t)h;
    const uint32_t first = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= total) return;
    const uint8_t* img = px + d[D_OUT];
    const int32_t* rid = ids + d[D_ROW];
    uint8_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t pos = min(first + k, total - 1);
        const int y = (int)(pos / stride), j = (int)(pos - (uint32_t)y * stride);
        const int id = rid[y];
        int f[5];
        filtered(img, nb, y, max(j - 1, 0), f);
        const int val = id == 0 ? f[0] : id == 1 ? f[1] : id == 2 ? f[2] : id == 3 ? f[3] : f[4];
        v[k] = (uint8_t)(j == 0 ? id : val);
    }
    uint8_t* dst = out + d[D_FILT] + first;
    if (first + 4 <= total) {
        *reinterpret_cast<uint32_t*>(dst) = v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
        for (uint32_t i = 0; i < total - first; ++i) dst[i] = v[i];       // the last 1-3 bytes of the image's stream
    }
}

}  // namespace

extern "C" {

int64_t xmc_png_filter_workspace_bytes(const int64_t* desc, int32_t n) {
    XMC_REQUIRE(desc != nullptr && n >= 1 && n <= XMC_CODEC_MAX_BATCH);
    int64_t rows = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* d = desc + (int64_t)i * XMC_CODEC_DESC_WORDS;
        XMC_REQUIRE(xmc_desc_geometry_ok(d, false));
        XMC_REQUIRE(d[D_ROW] >= 0 && d[D_ROW] < ((int64_t)1 << 40));
        const int64_t e = d[D_ROW] + d[D_H];
        rows = e > rows ? e : rows;
    }
    return xmc_desc_region_bytes(n) + rows * 4;
}

int xmc_png_filter_batch(const uint8_t* px, int64_t px_bytes, const int64_t* desc, int32_t n, uint8_t* out, int64_t out_bytes,
                         void* ws, int64_t ws_bytes, void* stream) {
    XMC_REQUIRE(px != nullptr && desc != nullptr && out != nullptr && ws != nullptr && px_bytes >= 0 && out_bytes >= 0);
    XMC_REQUIRE(n >= 1 && n <= XMC_CODEC_MAX_BATCH);
    XMC_REQUIRE((uintptr_t)px % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0);
    const int64_t need = xmc_png_filter_workspace_bytes(desc, n);
    XMC_REQUIRE(need > 0 && ws_bytes >= need);
    int64_t max_rows = 0, max_words = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* d = desc + (int64_t)i * XMC_CODEC_DESC_WORDS;
        const int64_t w = d[D_W], h = d[D_H], bytes = h * (1 + 3 * w);
        XMC_REQUIRE(d[D_OUT] >= 0 && d[D_OUT] <= px_bytes && 3 * w * h <= px_bytes - d[D_OUT]);
        XMC_REQUIRE(d[D_FILT] >= 0 && d[D_FILT] % 4 == 0 && d[D_FILT] <= out_bytes && bytes <= out_bytes - d[D_FILT]);
        max_rows = h > max_rows ? h : max_rows;
        max_words = (bytes + 3) / 4 > max_words ? (bytes + 3) / 4 : max_words;
    }
    hipStream_t s = (hipStream_t)stream;
    int64_t* ddesc = (int64_t*)ws;
    int32_t* ids = (int32_t*)((uint8_t*)ws + xmc_desc_region_bytes(n));
    hipError_t e = hipMemcpyAsync(ddesc, desc, (size_t)n * XMC_CODEC_DESC_WORDS * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return xmc_hip_err(e);
    dim3 g1((unsigned)((max_rows + 3) / 4), (unsigned)n);
    hipLaunchKernelGGL(png_choose_kernel, g1, dim3(256), 0, s, px, ddesc, ids);
    e = hipGetLastError();
    if (e != hipSuccess) return xmc_hip_err(e);
    dim3 g2((unsigned)((max_words + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(png_write_kernel, g2, dim3(256), 0, s, px, ddesc, ids, out);
    return xmc_hip_err(hipGetLastError());
}

}  // extern "C"
