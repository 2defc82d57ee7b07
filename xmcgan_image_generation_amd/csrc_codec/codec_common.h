// Shared by the codec kernels (libxmc_codec.so; include/xmc_codec.h): return codes and the per-image table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xmc_codec.h"

#define XMC_OK 0
#define XMC_EINVAL (-22)
static inline int xmc_hip_err(hipError_t e) { return e == hipSuccess ? XMC_OK : -(1000 + (int)e); }
#define XMC_REQUIRE(cond) \
    do {                  \
        if (!(cond)) return XMC_EINVAL; \
    } while (0)

enum { D_COEF = 0, D_QT, D_PLANE, D_OUT, D_W, D_H, D_NCOMP, D_HS, D_VS, D_FILT, D_ROW };

// the table at the front of a workspace, rounded to 256 bytes: what follows keeps the workspace's own alignment
static inline int64_t xmc_desc_region_bytes(int32_t n) {
    return (((int64_t)n * XMC_CODEC_DESC_WORDS * 8) + 255) & ~(int64_t)255;
}

// size and sampling of one row: what every call checks first
static inline bool xmc_desc_geometry_ok(const int64_t* d, bool need_sampling) {
    const int64_t w = d[D_W], h = d[D_H];
    if (w < 1 || h < 1 || w > XMC_CODEC_MAX_SIDE || h > XMC_CODEC_MAX_SIDE || w * h > XMC_CODEC_MAX_PIXELS) return false;
    if (!need_sampling) return true;
    const int64_t nc = d[D_NCOMP], hs = d[D_HS], vs = d[D_VS];
    if (nc == 1) return hs == 1 && vs == 1;
    return nc == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}
