// The pixel half of a JPEG decode for gfx950 (include/xmc_codec.h: xmc_jpeg_decode_batch): quantised coefficients + tables ->
// RGB pixels, for a batch of images of different sizes and samplings.  The arithmetic is the specification's
// (libml/jpeg.py: decode_coefficients_np), integer only, and is held to it bit for bit.
//
//   launch 1  jpeg_idct_kernel     one lane per stored block ROW (8 int16 = one 16-byte load, plus the 16-byte table row):
//             dequantise, row pass in registers, transpose through LDS, column pass, clamp, one 8-byte store of the
//             sample row into the component plane (workspace)
//   launch 2  jpeg_colour_kernel   one lane per 4 output pixels: luma + the four chroma taps of each plane at CLAMPED
//             indices (edge replication without a load under a condition), fixed-point JFIF matrix, three dword stores
//
// Both are memory-bound: per 4:2:0 pixel launch 1 reads 3 B of coefficients and writes 1.5 B of samples, launch 2 reads those
// 1.5 B (the chroma taps repeat within a cache line) and writes 3 B -- 9 B of HBM traffic per pixel.
#include "codec_common.h"

namespace {

constexpr int kBlocksPerWg = 32;                // 256 lanes / 8 rows
constexpr int kLdsBlockStride = 68;             // int32 per block: 64 + one 16-byte slot, so the 8 blocks of a wave start on
                                                // different banks and the ds_read_b128 of the column pass do not conflict

__device__ const int32_t kIdct[8][8] = {        // round(2^13 * c(u) / 2 * cos((2x + 1) u pi / 16)), [x][u]
    {2896, 4017, 3784, 3406, 2896, 2276, 1567, 799},
    {2896, 3406, 1567, -799, -2896, -4017, -3784, -2276},
    {2896, 2276, -1567, -4017, -2896, 799, 3784, 3406},
    {2896, 799, -3784, -2276, 2896, 3406, -1567, -4017},
    {2896, -799, -3784, 2276, 2896, -3406, -1567, 4017},
    {2896, -2276, -1567, 4017, -2896, -799, 3784, -3406},
    {2896, -3406, 1567, 799, -2896, 4017, -3784, 2276},
    {2896, -4017, 3784, -3406, 2896, -2276, 1567, -799},
};

struct Geometry {
    int w, h, ncomp, hs, vs, mcus_x, mcus_y;
    int nb0, nbc;                               // blocks of the luma plane, of one chroma plane
};

__device__ __host__ inline Geometry geometry(const int64_t* d) {
    Geometry g;
    g.w = (int)d[D_W], g.h = (int)d[D_H], g.ncomp = (int)d[D_NCOMP], g.hs = (int)d[D_HS], g.vs = (int)d[D_VS];
    g.mcus_x = (g.w + 8 * g.hs - 1) / (8 * g.hs), g.mcus_y = (g.h + 8 * g.vs - 1) / (8 * g.vs);
    g.nbc = g.mcus_x * g.mcus_y;
    g.nb0 = g.nbc * g.hs * g.vs;
    return g;
}

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt,
                                                         const int64_t* __restrict__ desc, uint8_t* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) int32_t lds[kBlocksPerWg * kLdsBlockStride];
    const int64_t* d = desc + (int64_t)blockIdx.y * XMC_CODEC_DESC_WORDS;
    const Geometry g = geometry(d);
    const int total = g.nb0 + (g.ncomp - 1) * g.nbc;
    const int slot = threadIdx.x >> 3, row = threadIdx.x & 7;
    const int b = blockIdx.x * kBlocksPerWg + slot;
    const bool valid = b < total;
    const int bb = min(b, total - 1);           // lanes past the image redo its last block and store nothing
    const int comp = bb < g.nb0 ? 0 : (bb - g.nb0 < g.nbc ? 1 : 2);
    const int local = bb - (comp == 0 ? 0 : g.nb0 + (comp - 1) * g.nbc);
    const int bw = comp == 0 ? g.mcus_x * g.hs : g.mcus_x;

    // the planes follow each other in the arena, so the block index of the image addresses it directly
    const int4 craw = *reinterpret_cast<const int4*>(coef + d[D_COEF] + (int64_t)bb * 64 + row * 8);
    const int4 qraw = *reinterpret_cast<const int4*>(qt + d[D_QT] + comp * 64 + row * 8);
    const int cw[4] = {craw.x, craw.y, craw.z, craw.w}, qw[4] = {qraw.x, qraw.y, qraw.z, qraw.w};
    int dq[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c0 = (int)(int16_t)(cw[i] & 0xffff), c1 = cw[i] >> 16;
        const int q0 = qw[i] & 0xffff, q1 = (int)((uint32_t)qw[i] >> 16);
        // int16 times uint16 is at most 32768 * 65535 = 2^31 - 32768: the product fits int32 as it is
        dq[2 * i] = clampi(c0 * q0, -XMC_JPEG_DEQUANT_CLAMP, XMC_JPEG_DEQUANT_CLAMP);
        dq[2 * i + 1] = clampi(c1 * q1, -XMC_JPEG_DEQUANT_CLAMP, XMC_JPEG_DEQUANT_CLAMP);
    }
    // row pass: t[v][x] = clamp((sum_u M[x][u] d[v][u] + 2^8) >> 9), this lane's v
    int t[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int s = 1 << 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) s += kIdct[x][u] * dq[u];
        t[x] = clampi(s >> 9, -XMC_JPEG_PASS1_CLAMP, XMC_JPEG_PASS1_CLAMP);
    }
    int32_t* mine = lds + slot * kLdsBlockStride;
    *reinterpret_cast<int4*>(mine + row * 8) = make_int4(t[0], t[1], t[2], t[3]);
    *reinterpret_cast<int4*>(mine + row * 8 + 4) = make_int4(t[4], t[5], t[6], t[7]);
    __syncthreads();
    // column pass: this lane is now sample row y = row; s[x] = (sum_v M[y][v] t[v][x] + 2^16) >> 17
    int acc[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) acc[x] = 1 << 16;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int m = kIdct[row][v];
        const int4 lo = *reinterpret_cast<const int4*>(mine + v * 8), hi = *reinterpret_cast<const int4*>(mine + v * 8 + 4);
        acc[0] += m * lo.x, acc[1] += m * lo.y, acc[2] += m * lo.z, acc[3] += m * lo.w;
        acc[4] += m * hi.x, acc[5] += m * hi.y, acc[6] += m * hi.z, acc[7] += m * hi.w;
    }
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        w0 |= (uint32_t)clampi((acc[x] >> 17) + 128, 0, 255) << (8 * x);
        w1 |= (uint32_t)clampi((acc[x + 4] >> 17) + 128, 0, 255) << (8 * x);
    }
    if (valid) {
        const int by = local / bw, bx = local - by * bw;
        uint8_t* plane = planes + d[D_PLANE] + (comp == 0 ? 0 : (int64_t)(g.nb0 + (comp - 1) * g.nbc) * 64);
        *reinterpret_cast<uint2*>(plane + ((int64_t)(by * 8 + row) * bw + bx) * 8) = make_uint2(w0, w1);
    }
}

// the nearer and the farther sample of one axis and their weights in quarters (3/4 + 1/4 when subsampled, 4/4 + 0 when not)
__device__ inline void axis_taps(int i, int factor, int samples, int& near, int& far, int& wn, int& wf) {
    const bool sub = factor == 2;
    near = sub ? i >> 1 : i;
    far = sub ? clampi(near + ((i & 1) ? 1 : -1), 0, samples - 1) : near;
    wn = sub ? 3 : 4;
    wf = sub ? 1 : 0;
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, const int64_t* __restrict__ desc,
                                                           uint8_t* __restrict__ out) {
    const int64_t* d = desc + (int64_t)blockIdx.y * XMC_CODEC_DESC_WORDS;
    const Geometry g = geometry(d);
    const uint32_t npix = (uint32_t)g.w * (uint32_t)g.h;
    const uint32_t first = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= npix) return;
    const int s0 = g.mcus_x * g.hs * 8;                               // bytes per row of the luma plane
    const bool colour = g.ncomp == 3;
    // a grey image reads its "chroma" taps from the luma plane (hs = vs = 1: valid indices) and discards them
    const int sc = colour ? g.mcus_x * 8 : s0;
    const uint8_t* p0 = planes + d[D_PLANE];
    const uint8_t* p1 = colour ? p0 + (int64_t)g.nb0 * 64 : p0;
    const uint8_t* p2 = colour ? p1 + (int64_t)g.nbc * 64 : p0;
    const int cw = (g.w + g.hs - 1) / g.hs, ch = (g.h + g.vs - 1) / g.vs;
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t p = min(first + k, npix - 1);
        const int y = (int)(p / (uint32_t)g.w), x = (int)(p - (uint32_t)y * (uint32_t)g.w);
        int x0, x1, wx0, wx1, y0, y1, wy0, wy1;
        axis_taps(x, g.hs, cw, x0, x1, wx0, wx1);
        axis_taps(y, g.vs, ch, y0, y1, wy0, wy1);
        const int luma = p0[y * s0 + x];
        const int o00 = y0 * sc + x0, o01 = y0 * sc + x1, o10 = y1 * sc + x0, o11 = y1 * sc + x1;
        const int w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
        int cb = (w00 * p1[o00] + w01 * p1[o01] + w10 * p1[o10] + w11 * p1[o11] + 8) >> 4;
        int cr = (w00 * p2[o00] + w01 * p2[o01] + w10 * p2[o10] + w11 * p2[o11] + 8) >> 4;
        cb = colour ? cb - 128 : 0;
        cr = colour ? cr - 128 : 0;
        px[3 * k] = (uint8_t)clampi(luma + ((91881 * cr + 32768) >> 16), 0, 255);
        px[3 * k + 1] = (uint8_t)clampi(luma + ((-22553 * cb - 46802 * cr + 32768) >> 16), 0, 255);
        px[3 * k + 2] = (uint8_t)clampi(luma + ((116130 * cb + 32768) >> 16), 0, 255);
    }
    uint8_t* dst = out + d[D_OUT] + (int64_t)first * 3;
    if (first + 4 <= npix) {
        uint32_t* dw = reinterpret_cast<uint32_t*>(dst);                 // out_off is a multiple of 4, and so is 12 * lane
#pragma unroll
        for (int i = 0; i < 3; ++i)
            dw[i] = px[4 * i] | (uint32_t)px[4 * i + 1] << 8 | (uint32_t)px[4 * i + 2] << 16 | (uint32_t)px[4 * i + 3] << 24;
    } else {
        const int nbytes = (int)(npix - first) * 3;                       // the last 1-3 pixels of the image
        for (int i = 0; i < nbytes; ++i) dst[i] = px[i];
    }
}

int64_t plane_bytes(const Geometry& g) { return ((int64_t)g.nb0 + (int64_t)(g.ncomp - 1) * g.nbc) * 64; }

}  // namespace

extern "C" {

int xmc_codec_abi_version(void) { return XMC_CODEC_ABI_VERSION; }

int64_t xmc_jpeg_plane_bytes(int32_t width, int32_t height, int32_t ncomp, int32_t hs, int32_t vs) {
    int64_t d[XMC_CODEC_DESC_WORDS] = {0};
    d[D_W] = width, d[D_H] = height, d[D_NCOMP] = ncomp, d[D_HS] = hs, d[D_VS] = vs;
    XMC_REQUIRE(xmc_desc_geometry_ok(d, true));
    return plane_bytes(geometry(d));
}

int64_t xmc_jpeg_decode_workspace_bytes(const int64_t* desc, int32_t n) {
    XMC_REQUIRE(desc != nullptr && n >= 1 && n <= XMC_CODEC_MAX_BATCH);
    int64_t end = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* d = desc + (int64_t)i * XMC_CODEC_DESC_WORDS;
        XMC_REQUIRE(xmc_desc_geometry_ok(d, true));
        XMC_REQUIRE(d[D_PLANE] >= 0 && d[D_PLANE] % 8 == 0 && d[D_PLANE] < ((int64_t)1 << 40));
        const int64_t e = d[D_PLANE] + plane_bytes(geometry(d));
        end = e > end ? e : end;
    }
    return xmc_desc_region_bytes(n) + end;
}

int xmc_jpeg_decode_batch(const int16_t* coef, int64_t coef_elems, const uint16_t* qt, int64_t qt_elems, const int64_t* desc,
                          int32_t n, uint8_t* out, int64_t out_bytes, void* ws, int64_t ws_bytes, void* stream) {
    XMC_REQUIRE(coef != nullptr && qt != nullptr && desc != nullptr && out != nullptr && ws != nullptr);
    XMC_REQUIRE(n >= 1 && n <= XMC_CODEC_MAX_BATCH && coef_elems >= 0 && qt_elems >= 0 && out_bytes >= 0);
    XMC_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)qt % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0);
    const int64_t need = xmc_jpeg_decode_workspace_bytes(desc, n);
    XMC_REQUIRE(need > 0 && ws_bytes >= need);
    int64_t max_blocks = 0, max_groups = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* d = desc + (int64_t)i * XMC_CODEC_DESC_WORDS;
        const Geometry g = geometry(d);
        const int64_t blocks = (int64_t)g.nb0 + (int64_t)(g.ncomp - 1) * g.nbc;
        XMC_REQUIRE(d[D_COEF] >= 0 && d[D_COEF] % 8 == 0 && d[D_COEF] <= coef_elems && blocks * 64 <= coef_elems - d[D_COEF]);
        XMC_REQUIRE(d[D_QT] >= 0 && d[D_QT] % 8 == 0 && d[D_QT] <= qt_elems && (int64_t)g.ncomp * 64 <= qt_elems - d[D_QT]);
        const int64_t px = (int64_t)g.w * g.h;
        XMC_REQUIRE(d[D_OUT] >= 0 && d[D_OUT] % 4 == 0 && d[D_OUT] <= out_bytes && px * 3 <= out_bytes - d[D_OUT]);
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        max_groups = (px + 3) / 4 > max_groups ? (px + 3) / 4 : max_groups;
    }
    hipStream_t s = (hipStream_t)stream;
    int64_t* ddesc = (int64_t*)ws;
    uint8_t* planes = (uint8_t*)ws + xmc_desc_region_bytes(n);
    hipError_t e = hipMemcpyAsync(ddesc, desc, (size_t)n * XMC_CODEC_DESC_WORDS * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return xmc_hip_err(e);
    dim3 g1((unsigned)((max_blocks + kBlocksPerWg - 1) / kBlocksPerWg), (unsigned)n);
    hipLaunchKernelGGL(jpeg_idct_kernel, g1, dim3(256), 0, s, coef, qt, ddesc, planes);
    e = hipGetLastError();
    if (e != hipSuccess) return xmc_hip_err(e);
    dim3 g2((unsigned)((max_groups + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(jpeg_colour_kernel, g2, dim3(256), 0, s, planes, ddesc, out);
    return xmc_hip_err(hipGetLastError());
}

}  // extern "C"
