// Host-side launch planning shared by the launchers of conv_stream.hip and conv_stream_mx8.hip: the spatial tile plan, the
// extent / alignment guard and the split-K bookkeeping.  Host code only (no kernel, no device function); the launchers' argument
// structs (SArgs, S8Args) name the plan's fields alike, so the helpers that fill them are templates over the struct.
#pragma once

#include <initializer_list>

#include "common.h"

// A launch walks an (n, h, w) grid of pixels (h, w powers of two) in tiles of `tile_px` pixels: wt columns x rt rows x imgs
// images (a tile holds several whole images once a map is smaller than it).  The tile's input patch -- the tile plus `margin`
// rows and columns, per image -- is staged through LDS as `vec_per_px` 16-byte vectors per patch pixel out of `vec_budget` slots.
struct XmcTilePlan {
    int wt, rt, imgs;
    int log2_wt, log2_rt, log2_imgs, log2_tx, log2_ty;       // -1 where the value is no power of two (the launchers reject those)
    int PW, PR1, PP, pbuf_bytes;                             // patch columns, rows, pixels; bytes of one patch buffer
    int magic_pw, magic_pr1;                                 // q = (x * magic) >> 16 == x / d for x < 1024
    long long tiles_m;
    bool fits;                                               // the patch fits the staging budget
};

constexpr int XMC_PATCH_PITCH_B = 80;                        // patch row pitch of every kernel planned here (64 data bytes + pad)

static inline XmcTilePlan xmc_tile_plan(int n, int h, int w, int tile_px, int wt_max, int margin, int vec_per_px, int vec_budget) {
    XmcTilePlan p{};
    if (n <= 0 || h <= 0 || w <= 0) return p;                // (fits = false, no tiles)
    p.wt = w < wt_max ? w : wt_max;
    p.rt = tile_px / p.wt; if (p.rt > h) p.rt = h;
    p.imgs = tile_px / (p.wt * p.rt);
    p.log2_wt = ilog2_exact(p.wt); p.log2_rt = ilog2_exact(p.rt); p.log2_imgs = ilog2_exact(p.imgs);
    p.log2_tx = ilog2_exact(w) - p.log2_wt; p.log2_ty = ilog2_exact(h) - p.log2_rt;
    p.PW = p.wt + margin; p.PR1 = p.rt + margin; p.PP = p.imgs * p.PR1 * p.PW;
    p.pbuf_bytes = ((p.PP + 7) & ~7) * XMC_PATCH_PITCH_B;
    p.magic_pw = 65536 / p.PW + 1; p.magic_pr1 = 65536 / p.PR1 + 1;
    p.tiles_m = (long long)((n + p.imgs - 1) / p.imgs) * (w / p.wt) * (h / p.rt);
    p.fits = p.PP * vec_per_px <= vec_budget;
    return p;
}

template <class Args>
static inline void xmc_plan_to_args(const XmcTilePlan& p, Args* a) {
    a->log2_wt = p.log2_wt; a->log2_rt = p.log2_rt; a->log2_imgs = p.log2_imgs; a->log2_tx = p.log2_tx; a->log2_ty = p.log2_ty;
    a->PW = p.PW; a->PR1 = p.PR1; a->PP = p.PP; a->pbuf_bytes = p.pbuf_bytes;
    a->magic_pw = p.magic_pw; a->magic_pr1 = p.magic_pr1;
    a->tiles_m = (int)p.tiles_m;
}

// The kernels index pixels with int and address their operands through 32-bit buffer offsets, 16 bytes at a time.
static inline bool xmc_extents_ok(long long pixels, std::initializer_list<long long> bytes, std::initializer_list<const void*> ptrs) {
    if (pixels >= (1ll << 31)) return false;
    for (long long b : bytes) if (b >= 0xfffffff0ll) return false;
    for (const void* q : ptrs) if ((uintptr_t)q % 16) return false;
    return true;
}

// Split-K factor of a launch of `wgs` workgroups over `nchunks` reduction chunks: only few-workgroup, long-K launches split, aiming
// at `target` workgroups with at least `min_chunks_per_split` chunks each.
static inline int xmc_ksplit_for(long long wgs, int nchunks, int max_wgs, int min_chunks, int target, int min_chunks_per_split) {
    if (wgs <= 0 || wgs >= max_wgs || nchunks < min_chunks) return 1;
    int ks = (int)((target + wgs / 2) / wgs);
    if (ks > nchunks / min_chunks_per_split) ks = nchunks / min_chunks_per_split;
    return ks < 2 ? 1 : ks;
}

// Settles a->ksplit / chunks_per_split / ws (a->nchunks and a->Cout are set; `ksplit` = the plan's factor, used only when the
// caller lends a workspace) and the features a split launch cannot serve: its finishing kernel writes neither bit masks nor MX
// packets, and reads bf16 masks only -- `mask_fallback`: a launch given both `mask` and `mask_bits` then reads `mask`.
// false: XMC_EINVAL.
template <class Args>
static inline bool xmc_settle_splitk(Args* a, int ksplit, void* ws, const void* mask, const void* mask_bits, void* y_bits,
                                     bool mask_fallback, const void* y8 = nullptr) {
    a->ksplit = ws ? ksplit : 1;
    a->chunks_per_split = (a->nchunks + a->ksplit - 1) / a->ksplit;
    a->ksplit = (a->nchunks + a->chunks_per_split - 1) / a->chunks_per_split;
    a->ws = static_cast<float*>(ws);
    if (a->ksplit > 1 && (y_bits || (mask_bits && !(mask_fallback && mask)))) return false;
    if ((mask_bits || y_bits) && (a->Cout % 16) != 0) return false;
    if (y8 && (a->ksplit > 1 || a->out_f32 || (a->Cout % 64) != 0 || ((uintptr_t)y8 % 16))) return false;   // the twin is written by the kernel's own epilogue
    a->mask_bits = a->ksplit > 1 ? nullptr : static_cast<const unsigned short*>(mask_bits);
    a->y_bits = static_cast<unsigned short*>(y_bits);
    return true;
}

// After the convolution kernel: the fixed-order finishing pass (FinishKernel(const Args, long long nvec)) of a split launch over the
// m output pixels, and the launch status.
template <auto FinishKernel, class Args>
static inline int xmc_finish_splitk(const Args& a, long long m, hipStream_t s) {
    if (a.ksplit > 1) {
        const long long nvec = m * (a.Cout / 4);
        hipLaunchKernelGGL(FinishKernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, a, nvec);
    }
    return xmc_hip_err(hipGetLastError());
}
