// MX-fp8 (OCP e4m3 elements, e8m0 scale per 32 channels) 3x3 convolution, forward and data gradient, for gfx950
// (BASELINE config #5: "fp8 MFMA convs"; reference call sites xmcgan/libml/layers.py:221-233 and flax nn.Conv in
// xmcgan/nets/common.py).  On gfx950 the plain fp8 MFMA runs at the bf16 rate; only the block-scaled
// v_mfma_scale_f32_32x32x64_f8f6f4 (K = 64 per instruction) doubles it, so both operands are MX blocks:
//
//   activations  x8 [pixel][Cp / 64][80] bytes (Cp = channels rounded up to 64, zero filled): per 64-channel chunk one 80-byte
//                PACKET = 64 e4m3 elements + the 2 e8m0 scale bytes of its two 32-channel blocks (bytes 64, 65) + pad --
//                exactly one row of the kernel's LDS patch, so staging a patch is nothing but 16-byte copies;
//                written by mx8_quantize_kernel from the bf16 tensor (the ReLU of `relu_in` folded in);
//   weights      fragment order [cout / 32][Cp / 64][tap][piece 0..1][lane 0..63][16 bytes] + scales
//                [cout / 32][Cp / 64][3][lane] uint32 (byte t % 4 of dword t / 4 = tap t), converted from the bf16
//                fragment-packed copy the prep kernels already write.  The 16-tap phase copies of the layers next to a 2x
//                resampling convert the same way ([tap 0..15], 4 scale dwords: one per phase) for conv_phase_mx8_kernel ("out" form,
//                conv3x3(upsample2(.))) and conv_phase_in_mx8_kernel ("in" form, avg_pool2(conv3x3(.))) below.
//
// Operand layout of the instruction (measured: tools/mx8_probe_layout.py, pinned by tests/test_gpu_mx8.py): lane l holds
// row / column l % 32; with h = l / 32 its registers 0..3 (16 bytes) are K = 16 h + 0..15 and its registers 4..7 are
// K = 32 + 16 h + 0..15; the scale byte of lanes 0..31 applies to K block 0 (K < 32, i.e. registers 0..3 of BOTH lane
// halves), the scale byte of lanes 32..63 to K block 1.  So piece 0 / 1 of a lane are 16 channels of the chunk's first /
// second 32-channel MX block, and lane half h carries the scale of block h.
//
// The kernel is the weight-streaming kernel of conv_stream.hip with 64-channel chunks: the input patch in LDS has the
// same 64-byte rows (+ the two scale bytes of the row in its pad), one chunk is 9 K=64 steps instead of 18 K=16 steps,
// the accumulators, tile shape (256 pixels x 128 couts, 4 waves x (2 x 4) 32x32 blocks), split-K and the whole
// epilogue (bias / mask / residual / pooling, bf16 or float32 out) are unchanged: float32 accumulation throughout.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "conv_plan.h"

#ifndef MX8_ABL
#define MX8_ABL 0        // timing ablations (tools only; results are wrong): 1 no B-fragment reads, 2 no weight refills, 4 no patch staging
#endif

namespace {

constexpr int SBM = 256, SPITCH_B = 80;              // tile pixels; patch row pitch: 64 data bytes + 2 scale bytes + pad
constexpr int NV_MAX = 8;                            // patch 16-byte vectors per thread: 5 per pixel packet, <= 409 patch pixels
constexpr int PBUF_BYTES = NV_MAX * 256 * 16;        // one patch buffer: EVERY vector of every thread has a slot (no guards)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
// two 16-byte pieces -> one 8-register operand tuple (a REG_SEQUENCE: the loads land in the tuple's halves, no copies)
__device__ __forceinline__ v8i join8(u32x4 lo, u32x4 hi) {
    return __builtin_shufflevector(__builtin_bit_cast(v4i, lo), __builtin_bit_cast(v4i, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- e4m3 / e8m0 helpers ---------------------------------------------------------------------------------------------
// MX block quantisation (OCP MX v1.0 format): elements = RNE(v / X) in e4m3, X = 2^k one e8m0 byte per 32 channels; amax == 0 ->
// scale byte 0, zero elements.  The scale: k = floor(log2(amax)) - 8 (the specification's conversion, e4m3: emax = 8) UNLESS the
// block maximum would then saturate -- amax / X in (448, 512), i.e. a significand above 1.75 -- in which case k is one higher
// (round 5).  With the plain floor rule a fifth of all blocks clip their largest element by up to 12.5 %: on post-ReLU activations
// that is a systematic shrink (-0.33 % of the mean, -1.4 % of the block maxima per layer; simulated and measured) which compounds
// through the network -- round 4's "+4 % g_loss bias" of config #5 -- and the RMS error is LOWER without it (2.65 % vs 3.18 %).
// Both rules are built: `rnd` = XMC_MX_RND_NEXT_BINADE (default) / XMC_MX_RND_OCP_FLOOR (xmc_set_tuning("mx8_scale_floor", 1), config.fp8_scale_rule).
__device__ __forceinline__ unsigned mx_scale_byte(float amax, unsigned rnd) {
    const int e = (int)(((__float_as_uint(amax) + rnd) >> 23) & 0xffu) - 8;         // biased exponent of X (denormal amax: 0);
    return (unsigned)(e < 0 ? 0 : e);                                               // + 0x1fffff: carries when the fraction > 0.75
}
__device__ __forceinline__ float mx_inv_scale(unsigned sb) {             // 1 / X = 2^(127 - sb)
    return __uint_as_float((254u - sb) << 23);
}
__device__ __forceinline__ unsigned pack_fp8x4(float a, float b, float c, float d) {
    a = fminf(fmaxf(a, -448.f), 448.f); b = fminf(fmaxf(b, -448.f), 448.f);
    c = fminf(fmaxf(c, -448.f), 448.f); d = fminf(fmaxf(d, -448.f), 448.f);
    int v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (unsigned)v;
}

// bf16 [M][C] -> x8 [M][Cp / 64][80].  Four lanes per 32-channel block (16 bytes of bf16 = 8 channels each).
__global__ __launch_bounds__(256) void mx8_quantize_kernel(const bf16_t* __restrict__ x, unsigned char* __restrict__ x8,
                                                           long long M, int C, int Cp, int relu, unsigned rnd) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int vpr = Cp >> 3;                          // 8-channel vectors per (padded) row
    const long long pix = t / vpr;
    const int c0 = (int)(t - pix * vpr) * 8;
    if (pix >= M) return;                             // (whole 4-lane groups: vpr % 8 == 0)
    float f[8];
    if (c0 < C) {
        Vec<bf16_t> v; v.load(x + pix * C + c0); v.get(f);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = 0.f;
    }
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (relu) f[e] = fmaxf(f[e], 0.f);
        amax = fmaxf(amax, fabsf(f[e]));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const unsigned sb = mx_scale_byte(amax, rnd);
    const float is = mx_inv_scale(sb);
    uint2 o;
    o.x = pack_fp8x4(f[0] * is, f[1] * is, f[2] * is, f[3] * is);
    o.y = pack_fp8x4(f[4] * is, f[5] * is, f[6] * is, f[7] * is);
    unsigned char* pk = x8 + (pix * (Cp >> 6) + (c0 >> 6)) * 80;       // the chunk's packet
    *reinterpret_cast<uint2*>(pk + (c0 & 63)) = o;
    if ((threadIdx.x & 3) == 0) pk[64 + ((c0 >> 5) & 1)] = (unsigned char)sb;
}

// bf16 fragment-packed weights (conv_stream.hip: [rows / 32][K / 32][tap][k16 half][lane][8]) -> MX-fp8 fragment order.
// One thread per (row block, 64-chunk, tap, lane).
__global__ __launch_bounds__(256) void mx8_pack_weight_kernel(const bf16_t* __restrict__ w, unsigned char* __restrict__ w8,
                                                              unsigned char* __restrict__ ws, int nrb, int kch32, int taps,
                                                              long long total, unsigned rnd) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int lane = (int)(t & 63);
    long long r = t >> 6;
    const int tap = (int)(r % taps); r /= taps;
    const int nc64 = (kch32 + 1) >> 1;
    const int c64 = (int)(r % nc64);
    const int rb = (int)(r / nc64);
    const int i = lane & 31, h = lane >> 5;
    float f[32];                                     // piece p (16 values) = channels 64 c64 + 32 p + 16 h + 0..15
    float am[2] = {0.f, 0.f};
#pragma unroll
    for (int pc = 0; pc < 2; ++pc)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c32 = 2 * c64 + pc;
            float g[8];
            if (c32 < kch32) {
                Vec<bf16_t> v;
                v.load(w + (((long long)rb * kch32 + c32) * taps + tap) * 1024 + h * 512 + (q * 32 + i) * 8);
                v.get(g);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) g[e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) { f[pc * 16 + q * 8 + e] = g[e]; am[pc] = fmaxf(am[pc], fabsf(g[e])); }
        }
    // an MX block = 32 channels = this lane's piece + the piece of lane ^ 32 (same row, other 16-channel half)
    am[0] = fmaxf(am[0], __shfl_xor(am[0], 32));
    am[1] = fmaxf(am[1], __shfl_xor(am[1], 32));
    const unsigned sb0 = mx_scale_byte(am[0], rnd), sb1 = mx_scale_byte(am[1], rnd);
    const float is0 = mx_inv_scale(sb0), is1 = mx_inv_scale(sb1);
    unsigned o[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_fp8x4(f[4 * e] * is0, f[4 * e + 1] * is0, f[4 * e + 2] * is0, f[4 * e + 3] * is0);
#pragma unroll
    for (int e = 4; e < 8; ++e) o[e] = pack_fp8x4(f[4 * e] * is1, f[4 * e + 1] * is1, f[4 * e + 2] * is1, f[4 * e + 3] * is1);
    const unsigned sb = h ? sb1 : sb0;               // lane half h carries the scale of block h
    const long long blk = ((long long)rb * nc64 + c64) * taps + tap;
    unsigned char* d = w8 + blk * 2048 + lane * 16;
    *reinterpret_cast<uint4*>(d) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4*>(d + 1024) = make_uint4(o[4], o[5], o[6], o[7]);
    const int sd = (taps + 3) >> 2;
    ws[((((long long)rb * nc64 + c64) * sd + (tap >> 2)) * 64 + lane) * 4 + (tap & 3)] = (unsigned char)sb;
}

// ONE scaled MFMA on operands given in matrix form -- pins the operand layout the kernels above assume.
//   a8 [32 rows][64 k] bytes, as [32][2] scale bytes, b8 [32 cols][64 k] bytes (B^T), bs [32][2] -> d [32][32] float32
__global__ void mx8_probe_kernel(const unsigned char* a8, const unsigned char* as, const unsigned char* b8,
                                 const unsigned char* bs, float* d) {
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    v8i a, b;
#pragma unroll
    for (int e = 0; e < 8; ++e) {                    // registers 0..3: K = 16 h + ..; registers 4..7: K = 32 + 16 h + ..
        const int k = (e >> 2) * 32 + h * 16 + (e & 3) * 4;
        a[e] = *reinterpret_cast<const int*>(a8 + i * 64 + k);
        b[e] = *reinterpret_cast<const int*>(b8 + i * 64 + k);
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 0, 0, 0, (int)as[i * 2 + h], 0, (int)bs[i * 2 + h]);
#pragma unroll
    for (int e = 0; e < 16; ++e) d[((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + i] = acc[e];
}

struct S8Args {
    const void* x; const void* w; const void* wsc; const float* bias; const void* mask; const void* res; void* y;
    unsigned mx_rnd;                // scale rule of the twin's packets
    void* y8; int y8_relu;          // optional MX-fp8 twin of y for the next convolution (bf16 output, Cout % 64 == 0, no split-K)
    // round 5: the features of the bf16 kernel's epilogue this one lacked (config #5 lost the stored ReLU and the bit masks of
    // every discriminator block to that): y = max(., 0), the ReLU mask read as bits, (y > 0) written as bits
    int relu_out; const unsigned short* mask_bits; unsigned short* y_bits;
    int N, Hi, Wi, Cp, Ho, Wo, Cout;
    int ups, res_ups, out_f32, pool_out;
    int nchunks, tiles_m, tiles_n;
    int log2_wt, log2_rt, log2_imgs, log2_tx, log2_ty;
    int PW, PR1, PP, pbuf_bytes;
    int magic_pw, magic_pr1;
    unsigned x_bytes, w_bytes, wsc_bytes;
    float alpha, res_scale;
    const float* alpha_dev;
    int ksplit, chunks_per_split;
    float* ws;
};

__global__ __launch_bounds__(256, 2) void conv_stream_mx8_kernel(const S8Args p) {
    constexpr int KS = 3, TAPS = 9, HALO = 1;
    constexpr int STEPS = TAPS;                      // one K = 64 step per tap per 64-channel chunk
    constexpr int D = 2;                             // weight register ring depth: slot = unit % 2; a chunk has 9 units, so the
                                                     // ring phase P alternates from chunk to chunk (two instantiations of the
                                                     // chunk body keep the slot indices compile-time)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int total_tiles = p.tiles_m * p.tiles_n;
    const int wid = xcd_remap(blockIdx.x, total_tiles * p.ksplit);
    const int split = wid / total_tiles, tile = wid - split * total_tiles;
    const int tn = tile / p.tiles_m, tm = tile - tn * p.tiles_m;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(p.nchunks, c_begin + p.chunks_per_split);
    const int Wt = 1 << p.log2_wt, Rt = 1 << p.log2_rt;
    const int tx = tm & ((1 << p.log2_tx) - 1), rest = tm >> p.log2_tx;
    const int ty = rest & ((1 << p.log2_ty) - 1);
    const int img0 = (rest >> p.log2_ty) << p.log2_imgs;
    const int y0 = ty << p.log2_rt, x0 = tx << p.log2_wt;

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wsc), 0, p.wsc_bytes, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;            // beyond any buffer: the load returns zeros

    // ---- patch staging.  A patch pixel's chunk is one 80-byte packet = five 16-byte vectors, in global memory and in LDS alike:
    //      vector v = thread + 256 i (i = 0 .. 7) is vector v % 5 of patch pixel v / 5 and lands at LDS byte 16 v of the buffer --
    //      a linear copy, no byte stores, no guards (a buffer holds all 2,048 vector slots; slots past the patch are never
    //      read).  The per-vector global offsets are computed once and parked in LDS (8 KiB behind the two buffers,
    //      [i][thread]), one ds_read_b32 per step: the kernel has no registers to hold them (first version: 44 spills whose
    //      scratch reloads sat in front of the patch loads), and recomputing them per step (~35 VALU with four quarter-rate
    //      multiplies beside eight 64-cycle MFMAs) cost 31 % (compile-time ablation, 768-channel 16^2 layer).
    const int nvec = p.PP * 5;
    const int row_bytes = (p.Cp >> 6) * 80;          // one pixel of x8
    auto patch_voff = [&](int i) -> unsigned {
        const int v = tid + 256 * i;
        const int pp = (v * 13108) >> 16, kv = v - pp * 5;               // v / 5 for v < 2^14
        const int pr = (pp * p.magic_pw) >> 16, pc = pp - pr * p.PW;
        const int im = (pr * p.magic_pr1) >> 16, rr = pr - im * p.PR1;
        const int y = y0 + rr - HALO, xx = x0 + pc - HALO;
        const bool in = (v < nvec) & ((unsigned)y < (unsigned)p.Ho) & ((unsigned)xx < (unsigned)p.Wo) & (img0 + im < p.N);
        const int sy = p.ups ? (y >> 1) : y, sx = p.ups ? (xx >> 1) : xx;
        return in ? (unsigned)((((img0 + im) * p.Hi + sy) * p.Wi + sx) * row_bytes + kv * 16) : OOB;
    };
    unsigned* const pvo_lds = reinterpret_cast<unsigned*>(lds + 2 * PBUF_BYTES) + tid;     // + i * 256
    auto store_vec = [&](int i, int bufoff, u32x4 q) {
        *reinterpret_cast<u32x4*>(lds + bufoff + (tid + 256 * i) * 16) = q;
    };

    // ---- MFMA geometry: wave -> 64 cout x 128 pixels (2 x 4 blocks)
    const int wp = wave >> 1, wc = (wave ^ (blockIdx.x >> 3)) & 1;
    const int l31 = lane & 31, lhi = lane >> 5;
    int pbase[4];                                    // LDS byte offset of (lane's pixel, tap (0,0), channels 16 lhi ..) in buffer 0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wp * 128 + j * 32 + l31;
        const int c = t & (Wt - 1), rowi = t >> p.log2_wt;
        const int im = rowi >> p.log2_rt, rj = rowi & (Rt - 1);
        pbase[j] = ((im * p.PR1 + rj) * p.PW + c) * SPITCH_B + lhi * 16;
    }
    auto out_pixel = [&](int j) {                    // output pixel index of block j's lane (or -1); epilogue only
        const int t = wp * 128 + j * 32 + l31;
        const int c = t & (Wt - 1), rowi = t >> p.log2_wt;
        const int im = rowi >> p.log2_rt, rj = rowi & (Rt - 1);
        return (img0 + im < p.N) ? ((img0 + im) * p.Ho + y0 + rj) * p.Wo + x0 + c : -1;
    };
    const int soff = 64 - 15 * lhi;                  // scale byte of K block lhi (row byte 64 + lhi), relative to pbase
    // ---- weight stream: block cb = tn * 4 + wc * 2 + i, linear over (chunk, tap, piece)
    const int ncb = (p.Cout + 31) >> 5;
    unsigned wvoff[2], wsvoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cb = tn * 4 + wc * 2 + i;
        wvoff[i] = cb < ncb ? (unsigned)(cb * p.nchunks + c_begin) * (unsigned)(STEPS * 2048) + lane * 16 : OOB;
        wsvoff[i] = cb < ncb ? (unsigned)(cb * p.nchunks + c_begin) * (unsigned)(3 * 256) + lane * 4 : OOB;
    }
    v8i wreg[D][2];
    auto load_w = [&](int slot, int unit) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            wreg[slot][i] = join8(__builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], unit * 2048, 0),
                                  __builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], unit * 2048 + 1024, 0));
    };
    unsigned wsc[2][3];                              // this chunk's weight scales: dword d = taps 4 d .. 4 d + 3
    auto load_wsc = [&](int cl) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int d = 0; d < 3; ++d)
                wsc[i][d] = __builtin_amdgcn_raw_buffer_load_b32(wsr, wsvoff[i], (cl * 3 + d) * 256, 0);
    };

    f32x16 acc[2][4];
    // B fragments: q = tap * 4 + j lives in xf[q & 1] and is read two fragments (= 2-4 MFMAs of 64 cycles) ahead of its
    // use -- the K = 64 instruction is long enough to cover the LDS latency, and four live 8-register fragments do not fit
    // beside 128 accumulators + the weight ring in the 256 registers of a 2-waves-per-SIMD kernel.
    v8i xf[2];
    unsigned xsc[2];
    auto read_x = [&](int q, int bufoff) {
        const int tap = q >> 2, j = q & 3;
        const int off = bufoff + ((tap / KS) * p.PW + (tap % KS)) * SPITCH_B;
        xf[q & 1] = join8(*reinterpret_cast<const u32x4*>(lds + pbase[j] + off), *reinterpret_cast<const u32x4*>(lds + pbase[j] + off + 32));
        xsc[q & 1] = lds[pbase[j] + off + soff];
    };

    // ---- prologue: whole patch of chunk 0 -> buffer 0; weight units 0 .. D-1; scales of chunk 0
    {
        u32x4 p0[NV_MAX];
#pragma unroll
        for (int i = 0; i < NV_MAX; ++i) {
            const unsigned vo = patch_voff(i);
            pvo_lds[i * 256] = vo;                   // read back only by this thread: no barrier needed for it
            p0[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo, c_begin * 80, 0);
        }
#pragma unroll
        for (int u = 0; u < D; ++u) load_w(u, u);
        load_wsc(0);
#pragma unroll
        for (int i = 0; i < NV_MAX; ++i) store_vec(i, 0, p0[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    read_x(0, 0); read_x(1, 0);

    auto k_loop = [&](auto nv_tag) {
        constexpr int NVB = decltype(nv_tag)::value;
        int unit = 0;
        auto chunk_body = [&](int chunk, auto phase_tag) {
            constexpr int P = decltype(phase_tag)::value;
            const bool next_chunk = chunk + 1 < c_end;
            const int cur = ((chunk - c_begin) & 1) * PBUF_BYTES, nxt = PBUF_BYTES - cur;
            const int nsoff = next_chunk ? (chunk + 1) * 80 : 0x7ffffff0;
            // Patch of the next chunk, one 16-byte vector per step: vector v is LOADED at the top of step v (v = 0 .. 7) and
            // STORED at the end of step v + 1 -- a whole step (8 MFMAs of 64 cycles) of slack for the L2 / HBM latency; two
            // register sets alternate.
            u32x4 pq[2];
#pragma unroll
            for (int s = 0; s < STEPS; ++s, ++unit) {
                const int slot = (s + P) & 1;        // compile-time after unrolling
#if !(MX8_ABL & 4)
                if (s < NV_MAX) pq[s & 1] = __builtin_amdgcn_raw_buffer_load_b128(xr, pvo_lds[s * 256], nsoff, 0);   // (last chunk: out of range, zeros, no traffic)
#endif
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (NVB >= 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = s * 4 + j;
                        const v8i xb = xf[q & 1];
                        const int xs_j = (int)xsc[q & 1];
#pragma unroll
                        for (int i = 0; i < NVB; ++i) {
                            const v8i wa = wreg[slot][i];
                            // opsel picks byte s % 4 of the lane's scale dword s / 4 (compile-time after unrolling)
                            if ((s & 3) == 0) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 0, (int)wsc[i][s >> 2], 0, xs_j);
                            else if ((s & 3) == 1) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 1, (int)wsc[i][s >> 2], 0, xs_j);
                            else if ((s & 3) == 2) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 2, (int)wsc[i][s >> 2], 0, xs_j);
                            else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 3, (int)wsc[i][s >> 2], 0, xs_j);
                        }
#if !(MX8_ABL & 1)
                        if (q + 2 < STEPS * 4) read_x(q + 2, cur);       // behind the last reader of its register set
#endif
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    // pin this step's MFMAs here: they have no side effects, and wherever the step body is more than one basic
                    // block LLVM sinks them to the end of the chunk (all 36 B fragments then live through scratch)
#pragma unroll
                    for (int i = 0; i < NVB; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(acc[i][j]));
#if !(MX8_ABL & 2)
#pragma unroll
                    for (int i = 0; i < NVB; ++i)
                        wreg[slot][i] = join8(__builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], (unit + D) * 2048, 0),
                                              __builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], (unit + D) * 2048 + 1024, 0));
#endif
                }
                __builtin_amdgcn_sched_barrier(0);
#if !(MX8_ABL & 4)
                if (s >= 1) store_vec(s - 1, nxt, pq[(s - 1) & 1]);
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
            if (NVB > 0) load_wsc(chunk + 1 - c_begin);      // (past the last chunk: the next block's scales or zeros, unused)
            __syncthreads();                         // next patch published; everyone is done reading the current one
            if (NVB > 0) { read_x(0, nxt); read_x(1, nxt); }
        };
        for (int chunk = c_begin; chunk < c_end; chunk += 2) {
            chunk_body(chunk, std::integral_constant<int, 0>{});
            if (chunk + 1 < c_end) chunk_body(chunk + 1, std::integral_constant<int, 1>{});
        }
    };
    const int left = ncb - (tn * 4 + wc * 2);
    if (left >= 2) k_loop(std::integral_constant<int, 2>{});
    else if (left == 1) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

    // ---- epilogue: as conv_stream_kernel (common.h)
    if (p.ksplit > 1) {
        ConvEpi e;
        e.bias = nullptr; e.mask = nullptr; e.res = nullptr; e.y = p.ws + (size_t)split * ((size_t)p.N * p.Ho * p.Wo * p.Cout);
        e.Cout = p.Cout; e.out_f32 = 1; e.alpha = 1.f; e.res_scale = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int opx = out_pixel(j);
            const bool live = opx >= 0;
            ConvEpi ej = e;
            if (!live) ej.Cout = 0;
            const size_t obase = (size_t)(live ? opx : 0) * p.Cout;
#pragma unroll
            for (int i = 0; i < 2; ++i) conv_epilogue_block(acc[i][j], tn * 128 + wc * 64 + i * 32, lhi, obase, obase, ej);
        }
        return;
    }
    ConvEpi e;
    e.bias = p.bias; e.mask = static_cast<const bf16_t*>(p.mask); e.res = static_cast<const bf16_t*>(p.res); e.y = p.y;
    e.Cout = p.Cout; e.out_f32 = p.out_f32; e.alpha = conv_alpha(p.alpha, p.alpha_dev); e.res_scale = p.res_scale;
    e.y8 = static_cast<unsigned char*>(p.y8); e.y8_relu = p.y8_relu; e.mx_rnd = p.mx_rnd;
    e.relu_out = p.relu_out; e.mask_bits = p.mask_bits; e.y_bits = p.y_bits;
    const int n0 = tn * 128;
    if (p.pool_out) {
        e.alpha = 0.25f * e.alpha;
        const int jstep = p.log2_wt == 6 ? 2 : 1;    // blocks (j, j + jstep) hold rows (r, r + 1)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ja = jstep == 2 ? q : 2 * q;
            const int t = wp * 128 + ja * 32 + l31;
            const int col = t & (Wt - 1), rowi = t >> p.log2_wt;
            const int im = rowi >> p.log2_rt, rj = rowi & (Rt - 1);
            const bool live = (l31 & 1) == 0 && img0 + im < p.N;
            const size_t obase = live ? ((size_t)((img0 + im) * (p.Ho >> 1) + ((y0 + rj) >> 1)) * (p.Wo >> 1) + ((x0 + col) >> 1)) * p.Cout : 0;
            ConvEpi ej = e;
            if (!live) ej.Cout = 0;
            ej.y8_pix = (long long)(obase / (size_t)p.Cout);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x16 sacc;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = (jstep == 2 ? acc[i][q][r] + acc[i][q + 2][r] : acc[i][2 * q][r] + acc[i][2 * q + 1][r]);
                    sacc[r] = v + __shfl_xor(v, 1);
                }
                conv_epilogue_block<true>(sacc, n0 + wc * 64 + i * 32, lhi, obase, obase, ej);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = out_pixel(j);
        const bool live = pix >= 0;
        const size_t obase = (size_t)(live ? pix : 0) * p.Cout;
        size_t rbase = obase;
        if (e.res && p.res_ups && live) {
            const int hw = p.Ho * p.Wo;
            const int n = pix / hw, rem = pix - n * hw;
            const int y2 = (rem / p.Wo) >> 1, x2 = (rem & (p.Wo - 1)) >> 1;
            rbase = ((size_t)(n * (p.Ho >> 1) + y2) * (p.Wo >> 1) + x2) * p.Cout;
        }
        ConvEpi ej = e;
        if (!live) ej.Cout = 0;
        ej.y8_pix = live ? pix : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) conv_epilogue_block<true>(acc[i][j], n0 + wc * 64 + i * 32, lhi, obase, rbase, ej);
    }
}

// ---- round 7: the "out" phase form on MX-fp8 operands ----------------------------------------------------------------
// conv3x3(nearest_upsample2(x)) as four 2x2 convolutions on the LOW-resolution grid (conv_phase_kernel of conv_stream.hip),
// multiplied by the block-scaled MFMA: y[2i+a][2j+b] = sum_{tu,tv} E_ab[tu][tv] x[i+a-1+tu][j+b-1+tv].  Weights: the MX copy
// of the 16-tap phase weights (tap = phase * 4 + tu * 2 + tv, phase = 2a + b; the tap sums were formed in float32 and are
// quantised once, when the weight is prepared).  The kernel is conv_stream_mx8_kernel with the phase as a grid dimension:
//   * a workgroup = one phase of one tile of 256 LOW-resolution pixels x 128 couts; the four phases of a tile are
//     neighbours in the launch order, so three of the four patch reads hit the L2;
//   * the patch is the (Wt + 1) x (Rt + 1) low-resolution packets with origin (y0 + a - 1, x0 + b - 1): whole packets,
//     linear 16-byte copies as before; at most 400 patch pixels (16 images of 4 x 4), so the 4^2 grids fit too;
//   * one chunk is 4 K = 64 steps (16 MFMA groups) instead of 9: the ring phase no longer alternates between chunks, and
//     the 8 patch vectors of the next chunk are staged as two groups of four (loaded at the top of steps 0 / 2, stored at
//     the end of steps 1 / 3: two steps = 16 MFMAs of slack each), four register sets instead of two;
//   * a chunk has ONE scale dword per weight block (byte s = tap s of this phase) instead of three;
//   * the store is stride 2: output pixel (2 (y0 + r) + a, 2 (x0 + c) + b) -- mask, mask bits, y bits and packets are
//     addressed by that pixel through the shared epilogue.
// Registers: 128 accumulators + 32 weight ring + 16 B fragments + 16 patch staging; LDS as the 3x3 kernel (2 x 32 KiB patch
// buffers + 8 KiB parked offsets = 72 KiB, two workgroups per CU).
__global__ __launch_bounds__(256, 2) void conv_phase_mx8_kernel(const S8Args p) {
    constexpr int STEPS = 4;                         // taps of one phase: one K = 64 step each per 64-channel chunk
    constexpr int D = 2;                             // weight register ring depth: slot = step % 2 (STEPS is even)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int total_tiles = p.tiles_m * p.tiles_n;
    const int wid = xcd_remap(blockIdx.x, total_tiles * p.ksplit * 4);
    const int ph = wid & 3, pa = ph >> 1, pb = ph & 1;
    const int wrest = wid >> 2;
    const int split = wrest / total_tiles, tile = wrest - split * total_tiles;
    const int tn = tile / p.tiles_m, tm = tile - tn * p.tiles_m;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(p.nchunks, c_begin + p.chunks_per_split);
    const int Wt = 1 << p.log2_wt, Rt = 1 << p.log2_rt;
    const int tx = tm & ((1 << p.log2_tx) - 1), rest = tm >> p.log2_tx;
    const int ty = rest & ((1 << p.log2_ty) - 1);
    const int img0 = (rest >> p.log2_ty) << p.log2_imgs;
    const int y0 = ty << p.log2_rt, x0 = tx << p.log2_wt;        // low-resolution origin of the tile

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wsc), 0, p.wsc_bytes, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;            // beyond any buffer: the load returns zeros

    // ---- patch staging: as conv_stream_mx8_kernel (vector v = thread + 256 i is vector v % 5 of patch pixel v / 5)
    const int nvec = p.PP * 5;
    const int row_bytes = (p.Cp >> 6) * 80;          // one pixel of x8
    auto patch_voff = [&](int i) -> unsigned {
        const int v = tid + 256 * i;
        const int pp = (v * 13108) >> 16, kv = v - pp * 5;               // v / 5 for v < 2^14
        const int pr = (pp * p.magic_pw) >> 16, pc = pp - pr * p.PW;
        const int im = (pr * p.magic_pr1) >> 16, rr = pr - im * p.PR1;
        const int y = y0 + rr + pa - 1, xx = x0 + pc + pb - 1;           // source pixel on the low-resolution map
        const bool in = (v < nvec) & ((unsigned)y < (unsigned)p.Hi) & ((unsigned)xx < (unsigned)p.Wi) & (img0 + im < p.N);
        return in ? (unsigned)((((img0 + im) * p.Hi + y) * p.Wi + xx) * row_bytes + kv * 16) : OOB;
    };
    unsigned* const pvo_lds = reinterpret_cast<unsigned*>(lds + 2 * PBUF_BYTES) + tid;     // + i * 256
    auto store_vec = [&](int i, int bufoff, u32x4 q) {
        *reinterpret_cast<u32x4*>(lds + bufoff + (tid + 256 * i) * 16) = q;
    };

    // ---- MFMA geometry: wave -> 64 cout x 128 low-resolution pixels (2 x 4 blocks)
    const int wp = wave >> 1, wc = (wave ^ (blockIdx.x >> 3)) & 1;
    const int l31 = lane & 31, lhi = lane >> 5;
    int pbase[4];                                    // LDS byte offset of (lane's pixel, tap (0,0), channels 16 lhi ..) in buffer 0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wp * 128 + j * 32 + l31;
        const int c = t & (Wt - 1), rowi = t >> p.log2_wt;
        const int im = rowi >> p.log2_rt, rj = rowi & (Rt - 1);
        pbase[j] = ((im * p.PR1 + rj) * p.PW + c) * SPITCH_B + lhi * 16;
    }
    auto out_pixel = [&](int j) {                    // output pixel index of block j's lane (or -1); epilogue only
        const int t = wp * 128 + j * 32 + l31;
        const int c = t & (Wt - 1), rowi = t >> p.log2_wt;
        const int im = rowi >> p.log2_rt, rj = rowi & (Rt - 1);
        return (img0 + im < p.N) ? ((img0 + im) * p.Ho + 2 * (y0 + rj) + pa) * p.Wo + 2 * (x0 + c) + pb : -1;
    };
    const int soff = 64 - 15 * lhi;                  // scale byte of K block lhi (row byte 64 + lhi), relative to pbase
    // ---- weight stream: block cb = tn * 4 + wc * 2 + i; a chunk holds 16 units (4 phases x 4 taps), this phase's are 4 ph ..
    const int ncb = (p.Cout + 31) >> 5;
    unsigned wvoff[2], wsvoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cb = tn * 4 + wc * 2 + i;
        wvoff[i] = cb < ncb ? ((unsigned)(cb * p.nchunks + c_begin) * 16u + 4u * ph) * 2048u + lane * 16 : OOB;
        wsvoff[i] = cb < ncb ? ((unsigned)(cb * p.nchunks + c_begin) * 4u + ph) * 256u + lane * 4 : OOB;
    }
    v8i wreg[D][2];
    auto load_w = [&](int slot, int i, int wch, int u) {             // unit u = tap u of this phase in the chunk at byte wch
        const int off = wch + u * 2048;
        wreg[slot][i] = join8(__builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], off, 0),
                              __builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], off + 1024, 0));
    };
    unsigned wsc[2];                                 // this chunk's weight scales: byte s = tap s of this phase
    auto load_wsc = [&](int cl) {
#pragma unroll
        for (int i = 0; i < 2; ++i) wsc[i] = __builtin_amdgcn_raw_buffer_load_b32(wsr, wsvoff[i], cl * 1024, 0);
    };

    f32x16 acc[2][4];
    v8i xf[2];                                       // B fragments: q = tap * 4 + j in xf[q & 1], read two fragments ahead
    unsigned xsc[2];
    auto read_x = [&](int q, int bufoff) {
        const int tap = q >> 2, j = q & 3;
        const int off = bufoff + ((tap >> 1) * p.PW + (tap & 1)) * SPITCH_B;
        xf[q & 1] = join8(*reinterpret_cast<const u32x4*>(lds + pbase[j] + off), *reinterpret_cast<const u32x4*>(lds + pbase[j] + off + 32));
        xsc[q & 1] = lds[pbase[j] + off + soff];
    };

    // ---- prologue: whole patch of chunk 0 -> buffer 0; weight units 0 .. D-1; scales of chunk 0
    {
        u32x4 p0[NV_MAX];
#pragma unroll
        for (int i = 0; i < NV_MAX; ++i) {
            const unsigned vo = patch_voff(i);
            pvo_lds[i * 256] = vo;                   // read back only by this thread: no barrier needed for it
            p0[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo, c_begin * 80, 0);
        }
#pragma unroll
        for (int u = 0; u < D; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i) load_w(u, i, 0, u);
        load_wsc(0);
#pragma unroll
        for (int i = 0; i < NV_MAX; ++i) store_vec(i, 0, p0[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    read_x(0, 0); read_x(1, 0);

    auto k_loop = [&](auto nv_tag) {
        constexpr int NVB = decltype(nv_tag)::value;
        for (int chunk = c_begin; chunk < c_end; ++chunk) {
            const bool next_chunk = chunk + 1 < c_end;
            const int cl = chunk - c_begin;
            const int cur = (cl & 1) * PBUF_BYTES, nxt = PBUF_BYTES - cur;
            const int nsoff = next_chunk ? (chunk + 1) * 80 : 0x7ffffff0;      // (last chunk: out of range, zeros, no traffic)
            const int wch = cl * 32768;              // this chunk's 16 units
            // the ring refills of steps 2 / 3 fetch the NEXT chunk's first units; behind the weight's last chunk they re-read this
            // chunk's instead (unused either way) so that no load leaves the buffer
            const int wnx = chunk + 1 < p.nchunks ? wch + 32768 : wch;
            u32x4 pq[4];
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int slot = s & 1;
#if !(MX8_ABL & 4)
                if ((s & 1) == 0) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) pq[v] = __builtin_amdgcn_raw_buffer_load_b128(xr, pvo_lds[(2 * s + v) * 256], nsoff, 0);
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (NVB >= 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = s * 4 + j;
                        const v8i xb = xf[q & 1];
                        const int xs_j = (int)xsc[q & 1];
#pragma unroll
                        for (int i = 0; i < NVB; ++i) {
                            const v8i wa = wreg[slot][i];
                            // opsel picks byte s of the lane's scale dword (compile-time after unrolling)
                            if (s == 0) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 0, (int)wsc[i], 0, xs_j);
                            else if (s == 1) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 1, (int)wsc[i], 0, xs_j);
                            else if (s == 2) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 2, (int)wsc[i], 0, xs_j);
                            else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 3, (int)wsc[i], 0, xs_j);
                        }
#if !(MX8_ABL & 1)
                        if (q + 2 < STEPS * 4) read_x(q + 2, cur);       // behind the last reader of its register set
#endif
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    // pin this step's MFMAs here (conv_stream_mx8_kernel: LLVM sinks them out of a multi-block step body)
#pragma unroll
                    for (int i = 0; i < NVB; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(acc[i][j]));
#if !(MX8_ABL & 2)
#pragma unroll
                    for (int i = 0; i < NVB; ++i) load_w(slot, i, s + D < STEPS ? wch : wnx, (s + D) & 3);
#endif
                }
                __builtin_amdgcn_sched_barrier(0);
#if !(MX8_ABL & 4)
                if (s & 1) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) store_vec(2 * (s - 1) + v, nxt, pq[v]);
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
            if (NVB > 0) load_wsc(chunk + 1 < p.nchunks ? cl + 1 : cl);      // (behind the last chunk: unused)
            __syncthreads();                         // next patch published; everyone is done reading the current one
            if (NVB > 0) { read_x(0, nxt); read_x(1, nxt); }
        }
    };
    const int left = ncb - (tn * 4 + wc * 2);
    if (left >= 2) k_loop(std::integral_constant<int, 2>{});
    else if (left == 1) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

    // ---- epilogue: as conv_stream_mx8_kernel, stride-2 store
    if (p.ksplit > 1) {
        ConvEpi e;
        e.bias = nullptr; e.mask = nullptr; e.res = nullptr; e.y = p.ws + (size_t)split * ((size_t)p.N * p.Ho * p.Wo * p.Cout);
        e.Cout = p.Cout; e.out_f32 = 1; e.alpha = 1.f; e.res_scale = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int opx = out_pixel(j);
            const bool live = opx >= 0;
            ConvEpi ej = e;
            if (!live) ej.Cout = 0;
            const size_t obase = (size_t)(live ? opx : 0) * p.Cout;
#pragma unroll
            for (int i = 0; i < 2; ++i) conv_epilogue_block(acc[i][j], tn * 128 + wc * 64 + i * 32, lhi, obase, obase, ej);
        }
        return;
    }
    ConvEpi e;
    e.bias = p.bias; e.mask = static_cast<const bf16_t*>(p.mask); e.res = nullptr; e.y = p.y;
    e.Cout = p.Cout; e.out_f32 = p.out_f32; e.alpha = conv_alpha(p.alpha, p.alpha_dev); e.res_scale = 0.f;
    e.y8 = static_cast<unsigned char*>(p.y8); e.y8_relu = p.y8_relu; e.mx_rnd = p.mx_rnd;
    e.relu_out = p.relu_out; e.mask_bits = p.mask_bits; e.y_bits = p.y_bits;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = out_pixel(j);
        const bool live = pix >= 0;
        const size_t obase = (size_t)(live ? pix : 0) * p.Cout;
        ConvEpi ej = e;
        if (!live) ej.Cout = 0;
        ej.y8_pix = live ? pix : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) conv_epilogue_block<true>(acc[i][j], tn * 128 + wc * 64 + i * 32, lhi, obase, obase, ej);
    }
}

// ---- round 8: the "in" phase form on MX-fp8 operands -----------------------------------------------------------------
// avg_pool2(conv3x3(x)) as four 2x2 convolutions on the LOW-resolution OUTPUT grid (conv_phase_kernel MODE 1 of
// conv_stream.hip), multiplied by the block-scaled MFMA:
//   P[i][j] = 1/4 sum_{a,b} sum_{tu,tv} F_ab[tu][tv] x[2 (i + tu) - a][2 (j + tv) - b]          (x at the HIGH resolution)
// decomposed by the PARITY (a, b) of the input pixel: parity ph = 2a + b is a 2x2 convolution over whole 80-byte packets of the
// sub-grid x[(2 - a) % 2 :: 2, (2 - b) % 2 :: 2] with window origin (i - a, j - b), and the four parities accumulate into the same
// output pixel -- the phase index sits in the K loop, not in the grid.  Weights: the MX copy of the "in"-order 16-tap phase
// weights (tap = ph * 4 + tu * 2 + tv; tap sums formed in float32, quantised once when the weight is prepared).  The kernel is
// conv_phase_mx8_kernel with
//   * a STAGE = one (parity, 64-channel chunk) pair = 4 K = 64 steps, walked PARITY-major like the bf16 kernel (all chunks of
//     parity 0, then parity 1, ...): inside a parity the weight stream advances by 16 units per stage exactly as one phase's
//     does in the "out" kernel, and consecutive stages read neighbouring packets of the same pixels;
//   * the patch of a stage = the (Wt + 1) x (Rt + 1) packets of its parity with origin (y0 - a, x0 - b), read at pixel stride 2.
//     The parked per-vector word (8 KiB of LDS, as before) is the byte offset of the parity-(0, 0) source pixel
//     (2 (y0 + rr), 2 (x0 + pc)) in bits 4..31 (offsets are multiples of 16) and one validity bit per parity in bits 0..3; a
//     stage subtracts its parity's (a Wi + b) pixels -- a scalar -- and selects "beyond the buffer" (zeros) where the bit is
//     clear: two VALU and a select per 16-byte vector, no second offset table, LDS stays 72 KiB (two workgroups per CU);
//   * split-K over the 64-channel chunks: every split walks its chunk range once per parity;
//   * a plain store at the output resolution; the 1/4 of the pooling is folded into alpha by the launcher, the residual is read
//     at the output resolution.
// Registers / LDS as the "out" kernel: 239 VGPRs, no scratch, 72 KiB, two workgroups per CU.  Measured on one MI355X at the C1 shapes
// (profiles/r08_conv_phase_in_mx_fp8.txt): the eight in-form launches take 1.178 ms on the bf16 "in" phase kernel, 0.818 ms here with the
// quantisation pass in front (1.44 x) and 0.647 ms on packets (1.82 x; per row 1.60-2.03 x); with the pass in front D 64>32 (192>192) is
// level (0.96 x).  C4 step with both phase switches 0.977 x the out-form-only C4, 0.945-0.948 x C3 (profiles/r08_c4_phase_in_mx_vs_c3.txt).
__global__ __launch_bounds__(256, 2) void conv_phase_in_mx8_kernel(const S8Args p) {
    constexpr int STEPS = 4;                         // taps of one parity: one K = 64 step each per 64-channel chunk
    constexpr int D = 2;                             // weight register ring depth: slot = step % 2 (STEPS is even)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int total_tiles = p.tiles_m * p.tiles_n;
    const int wid = xcd_remap(blockIdx.x, total_tiles * p.ksplit);
    const int split = wid / total_tiles, tile = wid - split * total_tiles;
    const int tn = tile / p.tiles_m, tm = tile - tn * p.tiles_m;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(p.nchunks, c_begin + p.chunks_per_split);
    const int Wt = 1 << p.log2_wt, Rt = 1 << p.log2_rt;
    const int tx = tm & ((1 << p.log2_tx) - 1), rest = tm >> p.log2_tx;
    const int ty = rest & ((1 << p.log2_ty) - 1);
    const int img0 = (rest >> p.log2_ty) << p.log2_imgs;
    const int y0 = ty << p.log2_rt, x0 = tx << p.log2_wt;        // origin of the tile on the OUTPUT (low-resolution) grid

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wsc), 0, p.wsc_bytes, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;            // beyond any buffer: the load returns zeros

    // ---- patch staging: vector v = thread + 256 i is vector v % 5 of patch pixel v / 5 (conv_stream_mx8_kernel).  Patch pixel
    //      (rr, pc) of parity (a, b) is input pixel (2 (y0 + rr) - a, 2 (x0 + pc) - b): inside the map iff y0 + rr < Ho (a = 0) /
    //      y0 + rr >= 1 (a = 1), the same for the columns (y0 + rr runs over 0 .. Ho inclusive).
    const int nvec = p.PP * 5;
    const int row_bytes = (p.Cp >> 6) * 80;          // one pixel of x8
    auto patch_word = [&](int i) -> unsigned {
        const int v = tid + 256 * i;
        const int pp = (v * 13108) >> 16, kv = v - pp * 5;               // v / 5 for v < 2^14
        const int pr = (pp * p.magic_pw) >> 16, pc = pp - pr * p.PW;
        const int im = (pr * p.magic_pr1) >> 16, rr = pr - im * p.PR1;
        const int yv = y0 + rr, xv = x0 + pc;
        const unsigned live = (v < nvec) & (img0 + im < p.N);
        const unsigned ry0 = live & (yv < p.Ho), ry1 = live & (yv >= 1), cx0 = xv < p.Wo, cx1 = xv >= 1;
        const unsigned m = (ry0 & cx0) | ((ry0 & cx1) << 1) | ((ry1 & cx0) << 2) | ((ry1 & cx1) << 3);
        return ((unsigned)(((img0 + im) * p.Hi + 2 * yv) * p.Wi + 2 * xv) * (unsigned)row_bytes + (unsigned)(kv * 16)) | m;
    };
    // this stage's parity: the pixels to step back from the parity-(0, 0) source (a scalar)
    auto parity_delta = [&](int ph) -> unsigned { return (unsigned)(((ph >> 1) * p.Wi + (ph & 1)) * row_bytes); };
    auto patch_voff = [&](unsigned word, unsigned bit, unsigned delta) -> unsigned {
        return (word & bit) ? (word & ~15u) - delta : OOB;
    };
    unsigned* const pvo_lds = reinterpret_cast<unsigned*>(lds + 2 * PBUF_BYTES) + tid;     // + i * 256
    auto store_vec = [&](int i, int bufoff, u32x4 q) {
        *reinterpret_cast<u32x4*>(lds + bufoff + (tid + 256 * i) * 16) = q;
    };

    // ---- MFMA geometry: wave -> 64 cout x 128 output pixels (2 x 4 blocks)
    const int wp = wave >> 1, wc = (wave ^ (blockIdx.x >> 3)) & 1;
    const int l31 = lane & 31, lhi = lane >> 5;
    int pbase[4];                                    // LDS byte offset of (lane's pixel, tap (0,0), channels 16 lhi ..) in buffer 0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wp * 128 + j * 32 + l31;
        const int c = t & (Wt - 1), rowi = t >> p.log2_wt;
        const int im = rowi >> p.log2_rt, rj = rowi & (Rt - 1);
        pbase[j] = ((im * p.PR1 + rj) * p.PW + c) * SPITCH_B + lhi * 16;
    }
    auto out_pixel = [&](int j) {                    // output pixel index of block j's lane (or -1); epilogue only
        const int t = wp * 128 + j * 32 + l31;
        const int c = t & (Wt - 1), rowi = t >> p.log2_wt;
        const int im = rowi >> p.log2_rt, rj = rowi & (Rt - 1);
        return (img0 + im < p.N) ? ((img0 + im) * p.Ho + y0 + rj) * p.Wo + x0 + c : -1;
    };
    const int soff = 64 - 15 * lhi;                  // scale byte of K block lhi (row byte 64 + lhi), relative to pbase
    // ---- weight stream: block cb = tn * 4 + wc * 2 + i; a chunk holds 16 units (4 parities x 4 taps): stage (ph, c) starts at
    //      unit c * 16 + ph * 4 of the block, its scale dword is number c * 4 + ph
    const int ncb = (p.Cout + 31) >> 5;
    unsigned wvoff[2], wsvoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cb = tn * 4 + wc * 2 + i;
        wvoff[i] = cb < ncb ? (unsigned)(cb * p.nchunks) * 32768u + lane * 16 : OOB;
        wsvoff[i] = cb < ncb ? (unsigned)(cb * p.nchunks) * 1024u + lane * 4 : OOB;
    }
    v8i wreg[D][2];
    auto load_w = [&](int slot, int i, int wst, int u) {             // unit u = tap u of the stage at byte wst
        const int off = wst + u * 2048;
        wreg[slot][i] = join8(__builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], off, 0),
                              __builtin_amdgcn_raw_buffer_load_b128(wr, wvoff[i], off + 1024, 0));
    };
    unsigned wsc[2];                                 // this stage's weight scales: byte s = tap s of its parity
    auto load_wsc = [&](int ph, int chunk) {
#pragma unroll
        for (int i = 0; i < 2; ++i) wsc[i] = __builtin_amdgcn_raw_buffer_load_b32(wsr, wsvoff[i], (chunk * 4 + ph) * 256, 0);
    };

    f32x16 acc[2][4];
    v8i xf[2];                                       // B fragments: q = tap * 4 + j in xf[q & 1], read two fragments ahead
    unsigned xsc[2];
    auto read_x = [&](int q, int bufoff) {
        const int tap = q >> 2, j = q & 3;
        const int off = bufoff + ((tap >> 1) * p.PW + (tap & 1)) * SPITCH_B;
        xf[q & 1] = join8(*reinterpret_cast<const u32x4*>(lds + pbase[j] + off), *reinterpret_cast<const u32x4*>(lds + pbase[j] + off + 32));
        xsc[q & 1] = lds[pbase[j] + off + soff];
    };

    // ---- prologue: whole patch of stage (parity 0, chunk c_begin) -> buffer 0; weight units 0 .. D-1; its scales
    {
        u32x4 p0[NV_MAX];
#pragma unroll
        for (int i = 0; i < NV_MAX; ++i) {
            const unsigned word = patch_word(i);
            pvo_lds[i * 256] = word;                 // read back only by this thread: no barrier needed for it
            p0[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, patch_voff(word, 1u, 0u), c_begin * 80, 0);
        }
#pragma unroll
        for (int u = 0; u < D; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i) load_w(u, i, c_begin * 32768, u);
        load_wsc(0, c_begin);
#pragma unroll
        for (int i = 0; i < NV_MAX; ++i) store_vec(i, 0, p0[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    read_x(0, 0); read_x(1, 0);

    auto k_loop = [&](auto nv_tag) {
        constexpr int NVB = decltype(nv_tag)::value;
        const int nst = (c_end - c_begin) * 4;
        int ph = 0, chunk = c_begin;
        for (int st = 0; st < nst; ++st) {
            const bool next = st + 1 < nst;
            int nph = ph, nchunk = chunk + 1;        // the stage after this one (behind the last: this one again, unused)
            if (nchunk == c_end) { nchunk = c_begin; nph = ph + 1; }
            if (!next) { nchunk = chunk; nph = ph; }
            const int cur = (st & 1) * PBUF_BYTES, nxt = PBUF_BYTES - cur;
            const unsigned nbit = next ? 1u << nph : 0u;                 // (last stage: every vector beyond the buffer, no traffic)
            const unsigned ndelta = parity_delta(nph);
            const int nsoff = nchunk * 80;
            const int wst = (chunk * 16 + ph * 4) * 2048, wnx = (nchunk * 16 + nph * 4) * 2048;
            u32x4 pq[4];
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int slot = s & 1;
#if !(MX8_ABL & 4)
                if ((s & 1) == 0) {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        pq[v] = __builtin_amdgcn_raw_buffer_load_b128(xr, patch_voff(pvo_lds[(2 * s + v) * 256], nbit, ndelta), nsoff, 0);
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (NVB >= 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = s * 4 + j;
                        const v8i xb = xf[q & 1];
                        const int xs_j = (int)xsc[q & 1];
#pragma unroll
                        for (int i = 0; i < NVB; ++i) {
                            const v8i wa = wreg[slot][i];
                            // opsel picks byte s of the lane's scale dword (compile-time after unrolling)
                            if (s == 0) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 0, (int)wsc[i], 0, xs_j);
                            else if (s == 1) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 1, (int)wsc[i], 0, xs_j);
                            else if (s == 2) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 2, (int)wsc[i], 0, xs_j);
                            else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xb, acc[i][j], 0, 0, 3, (int)wsc[i], 0, xs_j);
                        }
#if !(MX8_ABL & 1)
                        if (q + 2 < STEPS * 4) read_x(q + 2, cur);       // behind the last reader of its register set
#endif
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    // pin this step's MFMAs here (conv_stream_mx8_kernel: LLVM sinks them out of a multi-block step body)
#pragma unroll
                    for (int i = 0; i < NVB; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(acc[i][j]));
#if !(MX8_ABL & 2)
#pragma unroll
                    for (int i = 0; i < NVB; ++i) load_w(slot, i, s + D < STEPS ? wst : wnx, (s + D) & 3);
#endif
                }
                __builtin_amdgcn_sched_barrier(0);
#if !(MX8_ABL & 4)
                if (s & 1) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) store_vec(2 * (s - 1) + v, nxt, pq[v]);
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
            if (NVB > 0) load_wsc(nph, nchunk);
            __syncthreads();                         // next patch published; everyone is done reading the current one
            if (NVB > 0) { read_x(0, nxt); read_x(1, nxt); }
            ph = nph; chunk = nchunk;
        }
    };
    const int left = ncb - (tn * 4 + wc * 2);
    if (left >= 2) k_loop(std::integral_constant<int, 2>{});
    else if (left == 1) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

    // ---- epilogue: as conv_stream_mx8_kernel without pooling (the accumulators ARE the pooled sums; p.alpha carries the 1/4)
    if (p.ksplit > 1) {
        ConvEpi e;
        e.bias = nullptr; e.mask = nullptr; e.res = nullptr; e.y = p.ws + (size_t)split * ((size_t)p.N * p.Ho * p.Wo * p.Cout);
        e.Cout = p.Cout; e.out_f32 = 1; e.alpha = 1.f; e.res_scale = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int opx = out_pixel(j);
            const bool live = opx >= 0;
            ConvEpi ej = e;
            if (!live) ej.Cout = 0;
            const size_t obase = (size_t)(live ? opx : 0) * p.Cout;
#pragma unroll
            for (int i = 0; i < 2; ++i) conv_epilogue_block(acc[i][j], tn * 128 + wc * 64 + i * 32, lhi, obase, obase, ej);
        }
        return;
    }
    ConvEpi e;
    e.bias = p.bias; e.mask = nullptr; e.res = static_cast<const bf16_t*>(p.res); e.y = p.y;
    e.Cout = p.Cout; e.out_f32 = p.out_f32; e.alpha = conv_alpha(p.alpha, p.alpha_dev); e.res_scale = p.res_scale;
    e.y8 = static_cast<unsigned char*>(p.y8); e.y8_relu = p.y8_relu; e.mx_rnd = p.mx_rnd;
    e.relu_out = 0; e.mask_bits = nullptr; e.y_bits = p.y_bits;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = out_pixel(j);
        const bool live = pix >= 0;
        const size_t obase = (size_t)(live ? pix : 0) * p.Cout;
        ConvEpi ej = e;
        if (!live) ej.Cout = 0;
        ej.y8_pix = live ? pix : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) conv_epilogue_block<true>(acc[i][j], tn * 128 + wc * 64 + i * 32, lhi, obase, obase, ej);
    }
}

// y = epilogue(sum_s ws[s]) of a split-K launch (same contract as conv_splitk_finish_kernel of conv_stream.hip)
__global__ __launch_bounds__(256) void mx8_splitk_finish_kernel(const S8Args p, long long nvec) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvec) return;
    const int cv = p.Cout >> 2;
    const long long pix = v / cv;
    const int c = (int)(v - pix * cv) * 4;
    const size_t off = (size_t)pix * p.Cout + c, slice = (size_t)p.N * p.Ho * p.Wo * p.Cout;
    float4 a = *reinterpret_cast<const float4*>(p.ws + off);
    for (int s = 1; s < p.ksplit; ++s) {
        const float4 b = *reinterpret_cast<const float4*>(p.ws + s * slice + off);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    const float alpha = conv_alpha(p.alpha, p.alpha_dev);
    float r[4] = {a.x * alpha, a.y * alpha, a.z * alpha, a.w * alpha};
    if (p.bias) {
        const float4 b = *reinterpret_cast<const float4*>(p.bias + c);
        r[0] += b.x; r[1] += b.y; r[2] += b.z; r[3] += b.w;
    }
    if (p.mask) {
        const bf16_t* m = static_cast<const bf16_t*>(p.mask) + off;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (!(bf2f(m[e]) > 0.f)) r[e] = 0.f;
    }
    if (p.res) {
        size_t rb = off;
        if (p.res_ups) {
            const int hw = p.Ho * p.Wo;
            const int n = (int)(pix / hw), rem = (int)(pix - (long long)n * hw);
            const int y2 = (rem / p.Wo) >> 1, x2 = (rem % p.Wo) >> 1;
            rb = ((size_t)(n * (p.Ho >> 1) + y2) * (p.Wo >> 1) + x2) * p.Cout + c;
        }
        const bf16_t* q = static_cast<const bf16_t*>(p.res) + rb;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] += p.res_scale * bf2f(q[e]);
    }
    if (p.relu_out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], 0.f);
    }
    if (p.out_f32) *reinterpret_cast<float4*>(static_cast<float*>(p.y) + off) = make_float4(r[0], r[1], r[2], r[3]);
    else *reinterpret_cast<uint2*>(static_cast<bf16_t*>(p.y) + off) = make_uint2(pack_bf2(r[0], r[1]), pack_bf2(r[2], r[3]));
}

// Tile plan of the MX-fp8 launches: 256-pixel tiles at most 64 wide on an (n, h, w) grid; the patch (the tile plus `margin` rows and
// columns) is staged as 5 vectors per pixel packet
XmcTilePlan mx8_plan(int n, int h, int w, int margin) { return xmc_tile_plan(n, h, w, SBM, 64, margin, 5, NV_MAX * 256); }
XmcTilePlan mx8_stream_plan(const xmc_conv_desc* d) {         // the 3x3 form: the output grid, one-pixel halo
    const int up = d->ups ? 2 : 1;
    return mx8_plan(d->n, up * d->hi, up * d->wi, 2);
}

int mx8_ksplit(const xmc_conv_desc* d, long long tiles_m) {
    if (d->pool_out) return 1;
    // as the bf16 kernel: few-tile, long-K layers (4^2 / 8^2) only
    return xmc_ksplit_for(tiles_m * ((d->cout + 127) / 128), (d->cin + 63) / 64, 384, 8, 640, 2);
}

// Geometry of the MX-fp8 phase launches (XMC_CONV_PHASE on the MX entry points): tiles of 256 LOW-resolution pixels.  form 0, "out"
// (xmc_conv2d_mx8 with ups): the grid is the input map, the phase a grid dimension; form 1, "in" (xmc_conv2d_mx8_phase_in*): the grid
// is the pooled output map, the input parity in the K loop.  The single source of truth of the domains of conv_phase_mx8_kernel and
// conv_phase_in_mx8_kernel (xmc_conv2d_mx8_phase_supported / xmc_conv2d_mx8_phase_in_supported).
struct Mx8PhaseGeom { XmcTilePlan plan; int tiles_n, ksplit; };
bool mx8_phase_geom(const xmc_conv_desc* d, int form, Mx8PhaseGeom* g) {
    if (!(d->w_packed & XMC_CONV_PACKED) || !(d->w_packed & XMC_CONV_PHASE) || d->dtype != XMC_BF16 || d->ks != 3) return false;
    if ((form == 0) != (d->ups != 0) || (form == 1) != (d->pool_out != 0)) return false;      // "out": ups only; "in": pool_out only
    if (d->relu_in || (form == 1 && d->relu_out) || d->res_ups || d->mask_after_res || d->valid_h || d->valid_w) return false;
    if (d->n <= 0 || d->cin <= 0 || (d->cin % 64) != 0 || d->cout <= 0 || (d->cout % 32) != 0) return false;   // whole packets; the phase copies have rows % 32 == 0
    const int hv = form ? d->hi / 2 : d->hi, wv = form ? d->wi / 2 : d->wi, least = form ? 4 : 2;     // "in": output grids from 4 x 4
    if (ilog2_exact(d->hi) < 0 || ilog2_exact(d->wi) < 0 || hv < least || wv < least) return false;
    g->plan = mx8_plan(d->n, hv, wv, 1);
    if (!g->plan.fits) return false;                 // ("out" on 2 x 2 maps: 64 images x 9 patch pixels)
    g->tiles_n = (d->cout + 127) / 128;
    const long long wgs = g->plan.tiles_m * g->tiles_n * (form ? 1 : 4);
    if (wgs >= (1ll << 24)) return false;
    // as the bf16 phase kernels: few-tile, long-K layers (4^2 / 8^2) only
    g->ksplit = xmc_ksplit_for(wgs, d->cin / 64, 384, 8, xmc_internal_tuning(XMC_TUNE_KSPLIT_TARGET_PHASE), 2);
    return true;
}

}  // namespace

// > 64 KiB of dynamic LDS is an opt-in per kernel per device (also called by xmc_create for its device, so that a hipGraph
// capture never meets a first-use hipFuncSetAttribute)
extern "C" int xmc_internal_optin_mx8(void) {
    static XmcLdsOptIn opt_in;
    return opt_in.ensure({reinterpret_cast<const void*>(&conv_stream_mx8_kernel), reinterpret_cast<const void*>(&conv_phase_mx8_kernel),
                          reinterpret_cast<const void*>(&conv_phase_in_mx8_kernel)},
                         160 * 1024) ? XMC_OK : XMC_EINVAL;
}
static int optin_mx8() { return xmc_internal_optin_mx8(); }

extern "C" int xmc_mx8_quantize(const void* x, void* x8, int64_t pixels, int32_t c, int32_t relu, void* stream) {
    XMC_REQUIRE(x && x8 && pixels > 0 && c > 0 && (c % 8) == 0);
    XMC_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)x8 % 16) == 0);
    const int cp = (c + 63) & ~63;
    const long long nthr = (long long)pixels * (cp >> 3);
    hipLaunchKernelGGL(mx8_quantize_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(x), static_cast<unsigned char*>(x8), (long long)pixels, c, cp, relu, xmc_mx_rnd());
    XMC_LAUNCH_RET();
}

extern "C" int xmc_mx8_pack_conv_weight(const void* w_packed, void* w8, void* wscale, int32_t rows, int32_t taps, int32_t k,
                                        void* stream) {
    XMC_REQUIRE(w_packed && w8 && wscale && rows > 0 && (taps == 9 || taps == 16) && k > 0 && (k % 32) == 0);
    const int nrb = (rows + 31) / 32, kch32 = k / 32, nc64 = (kch32 + 1) / 2;
    const long long total = (long long)nrb * nc64 * taps * 64;
    hipLaunchKernelGGL(mx8_pack_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(w_packed), static_cast<unsigned char*>(w8), static_cast<unsigned char*>(wscale),
                       nrb, kch32, taps, total, xmc_mx_rnd());
    XMC_LAUNCH_RET();
}

extern "C" int xmc_mx8_probe(const void* a8, const void* as, const void* b8, const void* bs, float* d, void* stream) {
    XMC_REQUIRE(a8 && as && b8 && bs && d);
    hipLaunchKernelGGL(mx8_probe_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned char*>(a8), static_cast<const unsigned char*>(as),
                       static_cast<const unsigned char*>(b8), static_cast<const unsigned char*>(bs), d);
    XMC_LAUNCH_RET();
}

extern "C" int64_t xmc_conv2d_mx8_workspace_bytes(const xmc_conv_desc* d) {
    if (!d || d->ks != 3) return 0;
    Mx8PhaseGeom g;
    const bool phase = (d->w_packed & XMC_CONV_PHASE) != 0;
    if (phase && !mx8_phase_geom(d, 0, &g)) return 0;
    // Known wart, kept because the ABI's answers are: the 3x3 form is answered without asking whether the plan FITS, so a 4 x 4 map
    // (56 x 4 x 4, 1536 -> 1536: 66,060,288 bytes) gets a workspace although xmc_conv2d_mx8_bits rejects it (16 images per tile, 576
    // patch pixels); callers keep such maps on the bf16 kernel (ops._mx8_patch_fits).
    const int ks = phase ? g.ksplit : mx8_ksplit(d, mx8_stream_plan(d).tiles_m);
    if (ks <= 1) return 0;
    const long long m = (long long)d->n * (d->ups ? 4 : 1) * d->hi * d->wi;
    return (int64_t)ks * m * d->cout * 4;
}

extern "C" int xmc_conv2d_mx8_phase_supported(const xmc_conv_desc* d) {
    Mx8PhaseGeom g;
    return d && mx8_phase_geom(d, 0, &g) ? 1 : 0;
}

extern "C" int xmc_conv2d_mx8_phase_in_supported(const xmc_conv_desc* d) {
    Mx8PhaseGeom g;
    return d && mx8_phase_geom(d, 1, &g) ? 1 : 0;
}

extern "C" int64_t xmc_conv2d_mx8_phase_in_workspace_bytes(const xmc_conv_desc* d) {
    Mx8PhaseGeom g;
    if (!d || !mx8_phase_geom(d, 1, &g) || g.ksplit <= 1) return 0;
    return (int64_t)g.ksplit * ((long long)d->n * (d->hi / 2) * (d->wi / 2)) * d->cout * 4;
}

// What every launcher of this file puts into S8Args first: operands, shapes (y is (n, ho, wo, cout)), scales and the byte extents of
// the packets and of the MX weight copy (`taps` filter taps).  false: an operand is too large or misaligned.
static bool mx8_args(S8Args* a, const xmc_conv_desc* d, int ho, int wo, int taps, const void* x8, const void* w8, const void* wscale,
                     const float* bias, const void* mask, const void* res, void* y, void* y8, int32_t y8_relu) {
    a->x = x8; a->w = w8; a->wsc = wscale; a->bias = bias; a->mask = mask; a->res = res; a->y = y;
    a->y8 = y8; a->y8_relu = y8_relu; a->mx_rnd = xmc_mx_rnd();
    a->relu_out = d->relu_out;
    a->N = d->n; a->Hi = d->hi; a->Wi = d->wi; a->Cp = (d->cin + 63) & ~63; a->Cout = d->cout; a->Ho = ho; a->Wo = wo;
    a->ups = d->ups; a->res_ups = d->res_ups; a->out_f32 = d->out_f32; a->pool_out = d->pool_out;
    a->alpha = d->alpha; a->res_scale = d->res_scale; a->alpha_dev = d->alpha_dev;
    a->nchunks = a->Cp / 64;
    const long long pin = (long long)a->N * a->Hi * a->Wi, pout = (long long)a->N * ho * wo, ncb = (a->Cout + 31) / 32;
    const long long xb = pin * a->nchunks * 80, wb = ncb * a->nchunks * taps * 2048, wsb = ncb * a->nchunks * ((taps + 3) / 4) * 256;
    if (!xmc_extents_ok(pin > pout ? pin : pout, {xb, wb}, {x8, w8, y}) || ((uintptr_t)wscale % 4)) return false;
    a->x_bytes = (unsigned)xb; a->w_bytes = (unsigned)wb; a->wsc_bytes = (unsigned)wsb;
    return true;
}

// The phase forms (XMC_CONV_PACKED | XMC_CONV_PHASE; w8 / wscale are the MX copy, taps = 16, of the 16-tap phase weights).
// form 0, "out": conv3x3(upsample2(x)) on conv_phase_mx8_kernel (d->ups; no res).  form 1, "in": avg_pool2(conv3x3(x)) on
// conv_phase_in_mx8_kernel (d: hi / wi = the INPUT (high-resolution) map, pool_out = 1, ups = 0; the "in"-order copy; res and y at the
// output resolution; no mask) -- entry points of its own: on xmc_conv2d_mx8 the same descriptor stays XMC_EINVAL.
static int conv2d_mx8_phase(const xmc_conv_desc* d, int form, const void* x8, const void* w8, const void* wscale, const float* bias,
                            const void* mask, const void* res, void* y, void* y8, int32_t y8_relu, void* ws,
                            const void* mask_bits, void* y_bits, void* stream) {
    Mx8PhaseGeom g;
    if (!mx8_phase_geom(d, form, &g) || (form == 0 ? res != nullptr : (mask || mask_bits))) return XMC_EINVAL;
    S8Args a{};
    if (!mx8_args(&a, d, form ? d->hi / 2 : 2 * d->hi, form ? d->wi / 2 : 2 * d->wi, 16, x8, w8, wscale, bias, mask, res, y, y8, y8_relu))
        return XMC_EINVAL;
    a.ups = form ? 0 : 1; a.pool_out = 0;            // ("in": the finishing pass sees a plain launch on Ho x Wo)
    if (form) a.alpha = 0.25f * d->alpha;            // the 1/4 of the average pooling
    else a.res_scale = 0.f;
    xmc_plan_to_args(g.plan, &a);
    a.tiles_n = g.tiles_n;
    if (!xmc_settle_splitk(&a, g.ksplit, ws, mask, mask_bits, y_bits, false, y8)) return XMC_EINVAL;
    if (optin_mx8() != XMC_OK) return XMC_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(a.tiles_m * a.tiles_n * a.ksplit * (form ? 1 : 4)));
    const size_t lds_bytes = 2 * (size_t)PBUF_BYTES + NV_MAX * 1024;           // two patch buffers + the parked patch offsets
    if (form) hipLaunchKernelGGL(conv_phase_in_mx8_kernel, grid, dim3(256), lds_bytes, s, a);
    else hipLaunchKernelGGL(conv_phase_mx8_kernel, grid, dim3(256), lds_bytes, s, a);
    return xmc_finish_splitk<mx8_splitk_finish_kernel>(a, (long long)a.N * a.Ho * a.Wo, s);
}

extern "C" int xmc_conv2d_mx8_phase_in_bits(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                                            const float* bias, const void* res, void* y, void* y8, int32_t y8_relu,
                                            void* ws, void* y_bits, void* stream) {
    XMC_REQUIRE(d && x8 && w8 && wscale && y);
    return conv2d_mx8_phase(d, 1, x8, w8, wscale, bias, nullptr, res, y, y8, y8_relu, ws, nullptr, y_bits, stream);
}

extern "C" int xmc_conv2d_mx8_phase_in(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                                       const float* bias, const void* res, void* y, void* y8, int32_t y8_relu,
                                       void* ws, void* stream) {
    return xmc_conv2d_mx8_phase_in_bits(d, x8, w8, wscale, bias, res, y, y8, y8_relu, ws, nullptr, stream);
}

// 3x3 convolution on MX-fp8 operands.  d->cin = true channel count (x8 rows are padded to 64), d->relu_in must be 0 (fold it
// into xmc_mx8_quantize), mask_after_res / valid_* are not supported; relu_out, mask_bits (instead of mask) and y_bits as in
// xmc_conv2d_nhwc_bits (bits: launches without split-K, cout % 16 == 0).  Everything else as xmc_conv2d_nhwc_ws.
extern "C" int xmc_conv2d_mx8_bits(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                                   const float* bias, const void* mask, const void* res, void* y, void* y8, int32_t y8_relu,
                                   void* ws, const void* mask_bits, void* y_bits, void* stream) {
    XMC_REQUIRE(d && x8 && w8 && wscale && y);
    if (d->w_packed & XMC_CONV_PHASE)                // 16-tap phase weights: the "out" form or nothing
        return conv2d_mx8_phase(d, 0, x8, w8, wscale, bias, mask, res, y, y8, y8_relu, ws, mask_bits, y_bits, stream);
    if (d->ks != 3 || d->relu_in || d->mask_after_res || d->valid_h || (d->cout % 4) != 0) return XMC_EINVAL;
    if (d->pool_out && d->relu_out) return XMC_EINVAL;
    const int up = d->ups ? 2 : 1;
    if (d->pool_out && (up * d->wi < 32 || mask || mask_bits || d->res_ups)) return XMC_EINVAL;
    if (ilog2_exact(up * d->wi) < 0 || ilog2_exact(up * d->hi) < 0) return XMC_EINVAL;
    S8Args a{};
    if (!mx8_args(&a, d, up * d->hi, up * d->wi, 9, x8, w8, wscale, bias, mask, res, y, y8, y8_relu)) return XMC_EINVAL;
    const XmcTilePlan plan = mx8_stream_plan(d);
    if (!plan.fits) return XMC_EINVAL;
    xmc_plan_to_args(plan, &a);
    a.tiles_n = (a.Cout + 127) / 128;
    if (!xmc_settle_splitk(&a, mx8_ksplit(d, plan.tiles_m), ws, mask, mask_bits, y_bits, false, y8)) return XMC_EINVAL;
    if (optin_mx8() != XMC_OK) return XMC_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(conv_stream_mx8_kernel, dim3(a.tiles_m * a.tiles_n * a.ksplit), dim3(256), 2 * (size_t)PBUF_BYTES + NV_MAX * 1024, s, a);   // two patch buffers + the parked patch offsets
    return xmc_finish_splitk<mx8_splitk_finish_kernel>(a, (long long)a.N * a.Ho * a.Wo, s);
}

extern "C" int xmc_conv2d_mx8(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                              const float* bias, const void* mask, const void* res, void* y, void* y8, int32_t y8_relu,
                              void* ws, void* stream) {
    return xmc_conv2d_mx8_bits(d, x8, w8, wscale, bias, mask, res, y, y8, y8_relu, ws, nullptr, nullptr, stream);
}
