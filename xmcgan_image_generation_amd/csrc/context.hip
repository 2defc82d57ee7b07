// Per-device context handle of the C ABI (include/xmcgan_hip.h: xmc_create / xmc_destroy).
//
// The launch entry points keep no mutable global state except idempotent, lock-free per-device flags (the opt-in
// to > 64 KiB of dynamic LDS, common.h::XmcLdsOptIn), so a handle is not REQUIRED to launch; creating one
// validates the device (gfx950 only) and performs that per-device setup eagerly -- e.g. before a hipGraph capture
// or before several host threads start issuing work for the same GPU.
#include <atomic>
#include <cstring>
#include <new>

#include "common.h"

// ---- launch-heuristic knobs (xmc_set_tuning / xmc_get_tuning): the ONLY process-wide mutable state besides the LDS opt-in
// flags.  Defaults are the values A/B'd inside the training step; a setter exists so that those A/Bs
// can be repeated without rebuilding -- round 4 read them from the environment, which the header promises not to do.
namespace {
struct Knob { const char* key; int dflt; std::atomic<int> v; };
Knob g_knobs[XMC_TUNE_COUNT] = {
    {"ksplit_target", 256, {0}}, {"ksplit_target_phase", 384, {0}}, {"ksplit_target_pw", 256, {0}}, {"tile64_pct", 100, {0}},
    {"wgrad_target_hi", 384, {0}}, {"wgrad_target_lo", 512, {0}}, {"wgrad_target_phase", 384, {0}}, {"cbn_run", 1, {-1}},
    {"mx8_scale_floor", 0, {-1}},
};
}  // namespace

extern "C" int xmc_internal_tuning(int id) {
    if (id < 0 || id >= XMC_TUNE_COUNT) return 0;
    const int v = g_knobs[id].v.load(std::memory_order_relaxed);
    if (id == XMC_TUNE_CBN_RUN || id == XMC_TUNE_MX8_SCALE_FLOOR) return v < 0 ? g_knobs[id].dflt : v;         // switches: 0 is a value
    return v > 0 ? v : g_knobs[id].dflt;
}

extern "C" int xmc_set_tuning(const char* key, int32_t value) {
    XMC_REQUIRE(key);
    for (int i = 0; i < XMC_TUNE_COUNT; ++i)
        if (std::strcmp(key, g_knobs[i].key) == 0) {
            XMC_REQUIRE(value >= (i == XMC_TUNE_CBN_RUN || i == XMC_TUNE_MX8_SCALE_FLOOR ? -1 : 0));
            g_knobs[i].v.store(value, std::memory_order_relaxed);
            return XMC_OK;
        }
    return XMC_EINVAL;
}

extern "C" int xmc_get_tuning(const char* key, int32_t* value) {
    XMC_REQUIRE(key && value);
    for (int i = 0; i < XMC_TUNE_COUNT; ++i)
        if (std::strcmp(key, g_knobs[i].key) == 0) { *value = xmc_internal_tuning(i); return XMC_OK; }
    return XMC_EINVAL;
}

struct xmc_context {
    int device;
    char arch[64];
};

extern "C" int xmc_create(int32_t device, void** handle) {
    XMC_REQUIRE(handle);
    *handle = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) return xmc_hip_err(e);
    XMC_REQUIRE(device >= 0 && device < count);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return xmc_hip_err(e);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return XMC_EINVAL;          // CDNA4 only
    int prev = 0;
    e = hipGetDevice(&prev);
    if (e != hipSuccess) return xmc_hip_err(e);
    e = hipSetDevice(device);
    if (e != hipSuccess) return xmc_hip_err(e);
    int rc = xmc_internal_optin_conv_stream();
    if (rc == XMC_OK) rc = xmc_internal_optin_wgrad_dma();
    if (rc == XMC_OK) rc = xmc_internal_optin_wgrad_patch();
    if (rc == XMC_OK) rc = xmc_internal_optin_losses();
    if (rc == XMC_OK) rc = xmc_internal_optin_mx8();
    (void)hipSetDevice(prev);
    if (rc != XMC_OK) return rc;
    xmc_context* c = new (std::nothrow) xmc_context;
    if (!c) return -12;                                                                 // -ENOMEM
    c->device = device;
    std::strncpy(c->arch, prop.gcnArchName, sizeof(c->arch) - 1);
    c->arch[sizeof(c->arch) - 1] = 0;
    *handle = c;
    return XMC_OK;
}

extern "C" int xmc_destroy(void* handle) {
    XMC_REQUIRE(handle);
    delete static_cast<xmc_context*>(handle);
    return XMC_OK;
}

extern "C" int xmc_handle_device(void* handle) {
    XMC_REQUIRE(handle);
    return static_cast<xmc_context*>(handle)->device;
}
