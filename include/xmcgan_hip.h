/* libxmcgan_hip.so -- C ABI of the MI355X-native (gfx950) XMC-GAN G+D training-step kernels.
 *
 * The reference (google-research/xmcgan_image_generation) has no FFI: every device op is
 * emitted by XLA from jax.numpy / flax.linen calls.  This header therefore declares the
 * operator boundary a maintainer would bind from xmcgan/libml/layers.py,
 * xmcgan/libml/attention_lib.py, xmcgan/libml/losses.py, xmcgan/nets/common.py and
 * xmcgan/xmc_gan.py (file:line cited per entry point; paths relative to the reference
 * root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *    (kernels never allocate, so a whole step is hipGraph-capturable);
 *  - activations are NHWC, `dtype` = XMC_F32 or XMC_BF16; parameters, gradients,
 *    statistics and losses are always float32;
 *  - conv weights are "prepared" copies in the activation dtype:
 *      forward  layout [Cout][kh*kw][Cin]            (K contiguous per output channel)
 *      dgrad    layout [Cin][kh*kw flipped][Cout]
 *    produced by xmc_prep_conv_weight from the float32 master [Cout][kh*kw][Cin];
 *  - all launches are asynchronous on `stream` (a hipStream_t passed as void*), no hidden
 *    synchronisation; no environment variables are read and the only process-wide state is a set of
 *    idempotent per-device "LDS opt-in done" flags and the explicit tuning table of xmc_set_tuning
 *    (re-entrant, thread-safe, several GPUs per process);
 *  - return 0 on success, XMC_EINVAL for bad shape/dtype/alignment, -(1000+hipError_t) for
 *    HIP launch errors.  No exceptions, no abort.
 */
#ifndef XMCGAN_HIP_H_
#define XMCGAN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMC_OK 0
#define XMC_EINVAL (-22)

#define XMC_F32 0
#define XMC_BF16 1

#define XMC_ABI_VERSION 36
int xmc_abi_version(void);

/* Launch-heuristic knobs -- split-K workgroup targets and tile-selection thresholds whose defaults were A/B'd inside the
 * training step.  Process-wide, relaxed atomics; meant for repeating those A/Bs without a rebuild, not
 * for production use (the defaults are the product).  value 0 restores a target's default ("cbn_run": -1).  Keys:
 * "ksplit_target", "ksplit_target_phase", "ksplit_target_pw", "tile64_pct", "wgrad_target_hi", "wgrad_target_lo",
 * "wgrad_target_phase", "cbn_run", and one numerics switch: "mx8_scale_floor" (MX-fp8 quantisers, BASELINE config #5): 0 / -1 = the
 * build's default rule -- X = 2^(floor(log2 amax) - 8), one binade higher when the block maximum would saturate e4m3 (amax / X > 448)
 * -- 1 = the OCP MX v1.0 conversion exactly (plain floor rule; the largest element of ~1/5 of the blocks clips by up to 12.5 %).
 * Read at launch time by xmc_mx8_quantize, xmc_mx8_pack_conv_weight, xmc_cbn_act_fwd_mx8 and the packet-emitting epilogue of
 * xmc_conv2d_mx8(_bits).  Unknown key: XMC_EINVAL.  The library itself reads NO environment variable. */
int xmc_set_tuning(const char* key, int32_t value);
int xmc_get_tuning(const char* key, int32_t* value);

/* ------------------------------------------------------------------------------ per-device handle
 * xmc_create validates `device` (gfx950 only), performs the per-device kernel setup (opt-in to the
 * 160 KiB LDS of the convolution / word-loss kernels) and returns an opaque handle; xmc_destroy frees
 * it.  Launch entry points do not take the handle: the only process-wide state behind them are
 * idempotent per-device flags set lock-free, so calls are re-entrant and thread-safe with or without a
 * handle.  Create one per GPU before capturing a hipGraph or sharing a GPU between host threads. */
int xmc_create(int32_t device, void** handle);
int xmc_destroy(void* handle);
int xmc_handle_device(void* handle);     /* -> the device index the handle was created for */

/* ------------------------------------------------------------------ convolution (K1, K2, K4, K5)
 * Implicit-GEMM NHWC convolution, stride 1, SAME, ks in {1,3}; replaces
 * lax.conv_general_dilated at xmcgan/libml/layers.py:224-233 and flax nn.Conv in
 * xmcgan/nets/common.py:71-75,127-132,153-159,179-185, xmcgan/nets/xmc_net.py:114,220,245.
 *   a   = relu_in ? relu(x) : x ; a = ups ? nearest_upsample2(a) : a      (common.py:48-51)
 *   v   = alpha * conv(a, w) + bias
 *   v   = mask && !mask_after_res ? (mask > 0 ? v : 0) : v                (ReLU backward)
 *   v   = v + res_scale * (res_ups ? nearest_upsample2(res) : res)        (residual / unpool)
 *   v   = mask && mask_after_res ? (mask > 0 ? v : 0) : v                 (ReLU backward of a post-activation sum)
 *   v   = relu_out ? max(v, 0) : v                                        (post-activation residual, resnet_v1.py:86)
 *   y   = valid_h && (oy >= valid_h || ox >= valid_w) ? 0 : v             (canvas margin of the ResNet-50 path)
 * The same entry point computes dgrad when given the dgrad-layout weights.
 * Output spatial dims must be powers of two (4..256 in every XMC-GAN layer). */
typedef struct {
    int32_t n, hi, wi, cin;   /* x is (n, hi, wi, cin) */
    int32_t cout;             /* y is (n, ho, wo, cout), ho = ups ? 2*hi : hi */
    int32_t ks;               /* 1 or 3 */
    int32_t ups;              /* nearest 2x upsample of x fused into the gather */
    int32_t relu_in;          /* relu applied to x on load */
    int32_t res_ups;          /* res is (n, ho/2, wo/2, cout) and is nearest-upsampled */
    int32_t out_f32;          /* store y as float32 even when dtype == XMC_BF16 */
    int32_t dtype;            /* dtype of x, w, mask, res (and y unless out_f32) */
    float alpha;              /* scale on the convolution result */
    float res_scale;
    int32_t w_packed;         /* 0: w is the plain prepared copy; else a sum of the XMC_CONV_* values below:
                                 XMC_CONV_PACKED: w is in MFMA-fragment order (xmc_pack_conv_weight): bf16, cin % 32 == 0;
                                 XMC_CONV_PHASE: w holds the 16-tap PHASE weights of xmc_phase_conv_weight -- only with ks == 3 and
                                 exactly one of ups / pool_out: the launch runs as four 2x2 convolutions on the low-resolution
                                 grid (16 instead of 36 multiply-adds per low-resolution pixel; `ups`: no res, `pool_out`: no mask);
                                 XMC_CONV_PHASE_PER_WG: with PHASE and `ups`: the one-phase-per-workgroup form (A/B hook of tools/);
                                 XMC_CONV_COMPACT: compact pointwise launch (ks == 1, bf16, valid_h == valid_w = v > 0, no split-K): the
                                 workgroups cover only the v x v valid pixels of each ho x wo canvas (ResNet's 112/56/28/14/7
                                 maps on 128/64/32/16/8 canvases: 1.31x fewer pixels); margin pixels of y are NOT written --
                                 the caller keeps y in a buffer whose margins are zero once and stay zero;
                                 XMC_CONV_NO_PX128: with PHASE and `ups`: keep the 64-pixel x 128-cout tiles where the 128-pixel x
                                 64-cout ones would be chosen (A/B hook); XMC_CONV_NO_TILE96 .. XMC_CONV_PW_TILE_*: kernel A/B hooks
                                 of tools/ (0 = the shipped choice) */
    int32_t pool_out;         /* y = avg_pool2x2(v) + res_scale * res, y and res at (ho/2, wo/2): fused pooling of
                                 DiscBlock / DiscOptimizedBlock (common.py:76-78,131); w_packed, wo >= 32, no mask */
    int32_t relu_out;         /* ReLU on the result (after the residual) */
    int32_t mask_after_res;   /* the mask applies to v + res instead of to v */
    int32_t valid_h, valid_w; /* 0: every output pixel is live; else pixels outside the top-left valid_h x valid_w
                                 region of each image are stored as zero (no pool_out) */
    const float* alpha_dev;   /* NULL, or a float32 scalar in DEVICE memory multiplied into alpha when the kernel runs:
                                 1 / (sigma + eps) of a spectrally-normalised layer (W / sigma feeds a linear op, so the
                                 scale commutes with the convolution: xmcgan/libml/layers.py:209-233) -- the prepared
                                 weights are then a pure cast of W and need not wait for the power iteration */
} xmc_conv_desc;
/* xmc_conv_desc.w_packed */
#define XMC_CONV_PACKED 0x1
#define XMC_CONV_PHASE 0x10
#define XMC_CONV_PHASE_PER_WG 0x20
#define XMC_CONV_COMPACT 0x40
#define XMC_CONV_NO_PX128 0x80
#define XMC_CONV_NO_TILE96 0x100          /* A/B: 128-cout tiles where the 96-cout ones would be chosen */
#define XMC_CONV_FORCE_TILE96 0x200       /* A/B: 96-cout tiles for every cout % 96 == 0 */
#define XMC_CONV_NO_TILE64 0x400          /* A/B: no 64-cout tiles on unsplit few-tile 3x3 launches */
#define XMC_CONV_NO_TILE32 0x800          /* A/B: no 32-cout tiles for the <= 32-channel outputs */
#define XMC_CONV_PW_VARIANT_SHIFT 12      /* A/B, two bits: pointwise kernel 1 <32,3>, 2 <64,3>, 3 <32,4>; 0 = the shipped choice */
#define XMC_CONV_PW_VARIANT_MASK 0x3
#define XMC_CONV_PW_TILE_SHIFT 14         /* A/B, two bits: pointwise pixel tile 1 = 256, 2 = 128; 0 = the shipped choice */
#define XMC_CONV_PW_TILE_MASK 0x3

int xmc_conv2d_nhwc(const xmc_conv_desc* d, const void* x, const void* w, const float* bias,
                    const void* mask, const void* res, void* y, void* stream);

/* Layers with too few output tiles to fill the chip (the 4x4 / 8x8 layers) run split-K when the caller lends a
 * scratch buffer: xmc_conv2d_workspace_bytes(d) is the size xmc_conv2d_nhwc_ws wants for this descriptor (0: no
 * split; ws may then be NULL).  The buffer needs no initialisation; each split writes its own float32 slice and a
 * finishing kernel applies the epilogue.  xmc_conv2d_nhwc == xmc_conv2d_nhwc_ws(..., ws = NULL, ...). */
int64_t xmc_conv2d_workspace_bytes(const xmc_conv_desc* d);
/* 1 when a descriptor with XMC_CONV_PHASE (16-tap phase weights) is inside the phase-decomposed kernels' domain, else 0 (the
 * launch would return XMC_EINVAL): lets the caller decide between the phase copies and the plain 3x3 copies of a layer */
int xmc_conv2d_phase_supported(const xmc_conv_desc* d);
int xmc_conv2d_nhwc_ws(const xmc_conv_desc* d, const void* x, const void* w, const float* bias,
                       const void* mask, const void* res, void* y, void* ws, void* stream);
/* ReLU masks as BITS (kernels on fragment-packed weights, cout % 16 == 0): a mask tensor m (pixels, c) is also kept as
 * (pixels, c / 16) uint16 words, bit k of word j = (m[16 j + k] > 0).
 *   y_bits    (may be NULL): the launch also writes the bits of its OUTPUT (the stored value > 0) -- for the tensors that
 *             later serve as the `mask` of a data-gradient launch (jax.vjp of nn.relu: xmcgan/nets/common.py:63,66,129);
 *   mask_bits (may be NULL): used INSTEAD of `mask` (same shape convention): one 2-byte word per 16 couts and pixel
 *             in place of 32 bytes of bf16 that the epilogue would wait for (D 128^2 data gradient: 302 -> ~205 us).
 * A launch that takes the split-K route (xmc_conv2d_workspace_bytes(d) != 0 and ws given) cannot write y_bits (EINVAL) and
 * falls back to `mask` (which must then be given as well).  mask_bits == y_bits == NULL: xmc_conv2d_nhwc_ws. */
int xmc_conv2d_nhwc_bits(const xmc_conv_desc* d, const void* x, const void* w, const float* bias, const void* mask,
                         const void* res, void* y, void* ws, const void* mask_bits, void* y_bits, void* stream);

/* Pointwise (1x1) convolution whose reduction runs over TWO concatenated sources (round 6): y = epilogue([x | x2'] W^T), x2' pixel
 * (n, y, x) = x2[n, stride2 * y, stride2 * x, :] of an (n, h2, w2, cin2) tensor.  Replaces, in the frozen ResNet-50's down-sampling
 * bottleneck blocks, relu(bn3(conv3(h)) + proj_bn(proj_conv(x_in))) (xmcgan/utils/resnet_v1.py:74-86: the 1x1 stride-`strides`
 * projection shortcut and the block's last 1x1, eval-mode BatchNorm folded into W = [W3 | Wp], bias = b3 + bp) by ONE launch: the
 * projection's output is never written and re-read as the residual, and the sub-sampling copy in front of it is gone.
 * d as for xmc_conv2d_nhwc with ks = 1, dtype = XMC_BF16, cin = channels of x, fragment-packed w (K = cin + cin2; cin, cin2 multiples of
 * 32), COMPACT (w_packed = XMC_CONV_PACKED | XMC_CONV_COMPACT, valid_h == valid_w = v with 0 < v < hi: only the v x v corner of every canvas is walked, the
 * margins of y are not written); relu_out, mask_after_res honoured; no ups / res_ups / pool_out / relu_in / split-K.  mask / mask_bits /
 * res (each may be NULL) and y_bits (may be NULL; cout % 16 == 0) as in xmc_conv2d_nhwc_bits.
 * stride2 = 1 or 2: x2' as above.  stride2 = -2: the ADJOINT sampling -- x2' pixel (n, y, x) = x2[n, y / 2, x / 2, :] where y and x are both
 * even, zero elsewhere: the block's data gradient mask(conv1^T(dh1) + scatter2(proj^T(g))) of the same blocks as one launch over
 * [dh1 | g'] with W = [W1^T | Wp^T] (jax.vjp of resnet_v1.py:74-86): the projection's gradient is never written, zero-scattered or re-read. */
int xmc_conv2d_pw_dual(const xmc_conv_desc* d, const void* x, const void* x2, int32_t cin2, int32_t h2, int32_t w2,
                       int32_t stride2, const void* w, const float* bias, const void* mask, const void* res, void* y,
                       const void* mask_bits, void* y_bits, void* stream);

/* ---- MX-fp8 3x3 convolution (BASELINE config #5: fp8 MFMA convolutions; replaces the conv_general_dilated of
 * xmcgan/libml/layers.py:221-233 and the flax nn.Conv of xmcgan/nets/common.py:152-159 when config.conv_fp8 is set).
 * Operands are OCP MX blocks: e4m3 elements with one e8m0 scale byte per 32 channels, multiplied by the gfx950
 * block-scaled MFMA (K = 64 per instruction, twice the bf16 rate), float32 accumulation, the bf16 kernel's epilogue.
 *
 * xmc_mx8_quantize: bf16 x [pixels][c] (c % 8 == 0) -> x8 [pixels][cp / 64][80] bytes (cp = c rounded up to 64, zero filled):
 *   per 64-channel chunk one 80-byte packet = 64 elements + the two scale bytes of its 32-channel blocks (bytes 64, 65) +
 *   pad; relu != 0 applies max(., 0) first (the `relu_in` of the convolution).
 * xmc_mx8_pack_conv_weight: bf16 fragment-packed weights (xmc_pack_conv_weight / the packed prep outputs: rows x 9 taps x
 *   k) -> w8 (ceil(rows / 32) * ceil(k / 64) * 9 * 2048 bytes) and wscale (ceil(rows / 32) * ceil(k / 64) * 3 * 256 bytes).
 *   taps = 16 (ABI 24): the input is an "out"-order 16-tap phase copy of xmc_phase_conv_weight / xmc_wprep_batched (tap = phase * 4 +
 *   tu * 2 + tv; the tap sums were formed in float32 and rounded to bf16 once) -> w8 (ceil(rows / 32) * ceil(k / 64) * 16 * 2048
 *   bytes) and wscale (ceil(rows / 32) * ceil(k / 64) * 4 * 256 bytes: one scale dword per phase, byte = tu * 2 + tv).
 * xmc_conv2d_mx8: y = epilogue(conv3x3(x8, w8)); d as for xmc_conv2d_nhwc with ks = 3, cin = the TRUE channel count,
 *   relu_in = mask_after_res = valid_* = 0 (relu_out: see xmc_conv2d_mx8_bits); ws (may be NULL) of xmc_conv2d_mx8_workspace_bytes(d) bytes
 *   enables split-K on few-tile layers.  y8 (may be NULL; needs bf16 output, cout % 64 == 0 and a launch without
 *   split-K): the epilogue also writes y as packets for the NEXT convolution, y8_relu = that convolution's relu_in --
 *   byte for byte what xmc_mx8_quantize(y, relu) would write, without the extra pass.
 * The "out" PHASE form on MX-fp8 operands (ABI 24): d->w_packed = XMC_CONV_PACKED | XMC_CONV_PHASE with d->ups = 1 runs conv3x3(nearest_upsample2(x)) as four
 *   2x2 convolutions on the low-resolution grid, y[2i+a][2j+b] = sum_{tu,tv} E_ab[tu][tv] x[i+a-1+tu][j+b-1+tv] (16 instead of 36
 *   block-scaled products per low-resolution pixel); x8 = the packets of the LOW-resolution tensor, w8 / wscale = the taps = 16
 *   output of xmc_mx8_pack_conv_weight.  Replaces, when config.conv_fp8_phase is set, the generator blocks' first convolution
 *   (xmcgan/nets/common.py:152-159) and the data gradient of the down-sampling discriminator blocks' second convolution (the
 *   adjoint of xmcgan/nets/common.py:76-78).  Domain = xmc_conv2d_mx8_phase_supported(d): bf16, ks = 3, ups, no pool_out (the "in"
 *   form is not built: XMC_EINVAL), cin % 64 == 0, cout % 32 == 0, power-of-two low-resolution grids of 4 x 4 and larger,
 *   relu_in = res_ups = mask_after_res = valid_* = 0; res must be NULL.  bias, alpha, alpha_dev, mask, mask_bits, y_bits,
 *   relu_out, out_f32, y8 and the split-K workspace as for the 3x3 form (xmc_conv2d_mx8_workspace_bytes answers for these
 *   descriptors too).  Outside the domain the launch returns XMC_EINVAL; it never runs another kernel.
 * The "in" PHASE form on MX-fp8 operands (ABI 25; entry points of their own -- on xmc_conv2d_mx8 a pool_out descriptor with XMC_CONV_PHASE
 *   stays XMC_EINVAL): xmc_conv2d_mx8_phase_in[_bits] runs avg_pool2(conv3x3(x)) as four 2x2 convolutions on the low-resolution
 *   OUTPUT grid, decomposed by the parity (a, b) of the input pixel: y[i][j] = 1/4 sum_{a,b} sum_{tu,tv} F_ab[tu][tv]
 *   x[2(i+tu)-a][2(j+tv)-b] (16 instead of 36 block-scaled products per output pixel; every parity gathers whole 80-byte packets at
 *   pixel stride 2).  d: hi / wi = the INPUT map, ups = 0, pool_out = 1, w_packed = XMC_CONV_PACKED | XMC_CONV_PHASE; x8 = the packets of the input tensor; w8 /
 *   wscale = the taps = 16 output of xmc_mx8_pack_conv_weight on an "in"-order phase copy (xmc_phase_conv_weight / xmc_wprep_batched:
 *   tap = (2a + b) * 4 + tu * 2 + tv).  Replaces, when config.conv_fp8_phase_in is set, the second convolution of the down-sampling
 *   discriminator blocks (xmcgan/nets/common.py:76-78) and the data gradient of the generator blocks' first convolution (the
 *   adjoint of xmcgan/nets/common.py:152-159).  Domain = xmc_conv2d_mx8_phase_in_supported(d): bf16, ks = 3, pool_out, no ups,
 *   cin % 64 == 0, cout % 32 == 0, power-of-two input maps of 8 x 8 and larger (output grids from 4 x 4), relu_in = relu_out =
 *   res_ups = mask_after_res = valid_* = 0, no mask; the stride-2 ("s2in") copies are not its operands.  y = alpha * alpha_dev * 1/4 *
 *   acc + bias + res_scale * res (res, y, y_bits, y8 at the output resolution); out_f32, y8 / y8_relu as xmc_conv2d_mx8; ws (may be
 *   NULL) of xmc_conv2d_mx8_phase_in_workspace_bytes(d) bytes enables split-K (fixed-order finishing pass; then no y8 / y_bits).
 *   Outside the domain the launch returns XMC_EINVAL; it never runs another kernel.  Measured (profiles/r08_conv_phase_in_mx_fp8.txt):
 *   1.44 x (quantisation pass in front) / 1.82 x (on packets) the bf16 "in" phase kernel over the eight C1 launches.
 * xmc_mx8_probe: one scaled MFMA on a8 [32][64] / b8 [32][64] (B transposed) bytes with scales as / bs [32][2] ->
 *   d [32][32] float32; pins the operand layout (tests). */
int xmc_mx8_quantize(const void* x, void* x8, int64_t pixels, int32_t c, int32_t relu, void* stream);
int xmc_mx8_pack_conv_weight(const void* w_packed, void* w8, void* wscale, int32_t rows, int32_t taps, int32_t k,
                             void* stream);
int64_t xmc_conv2d_mx8_workspace_bytes(const xmc_conv_desc* d);
/* 1 when a descriptor with XMC_CONV_PACKED | XMC_CONV_PHASE is inside the MX-fp8 "out" phase kernel's domain, else 0 */
int xmc_conv2d_mx8_phase_supported(const xmc_conv_desc* d);
/* 1 when the descriptor is inside the MX-fp8 "in" phase kernel's domain, else 0; its split-K workspace (0: none) */
int xmc_conv2d_mx8_phase_in_supported(const xmc_conv_desc* d);
int64_t xmc_conv2d_mx8_phase_in_workspace_bytes(const xmc_conv_desc* d);
int xmc_conv2d_mx8_phase_in(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                            const float* bias, const void* res, void* y, void* y8, int32_t y8_relu,
                            void* ws, void* stream);
int xmc_conv2d_mx8_phase_in_bits(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                                 const float* bias, const void* res, void* y, void* y8, int32_t y8_relu,
                                 void* ws, void* y_bits, void* stream);
int xmc_conv2d_mx8(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                   const float* bias, const void* mask, const void* res, void* y, void* y8, int32_t y8_relu,
                   void* ws, void* stream);
/* ... with the bf16 kernel's epilogue features (ABI 21): d->relu_out = 1 allowed (y = max(., 0); not with pool_out), mask_bits
 * (may be NULL) used INSTEAD of mask, y_bits (may be NULL) receives (y > 0) -- both as in xmc_conv2d_nhwc_bits: cout % 16 == 0 and
 * a launch without split-K (XMC_EINVAL otherwise; pass ws = NULL or check xmc_conv2d_mx8_workspace_bytes(d) == 0). */
int xmc_conv2d_mx8_bits(const xmc_conv_desc* d, const void* x8, const void* w8, const void* wscale,
                        const float* bias, const void* mask, const void* res, void* y, void* y8, int32_t y8_relu,
                        void* ws, const void* mask_bits, void* y_bits, void* stream);
int xmc_mx8_probe(const void* a8, const void* as, const void* b8, const void* bs, float* d, void* stream);

/* Weight gradient of the convolution above (jax.vjp of the same call sites):
 *   dw[cout][tap][cin] += alpha * sum_p dy'(p, cout) * a(p + tap, cin)
 * with a() as in xmc_conv2d_nhwc and dy' = dy_ups ? nearest_upsample2(dy) : dy.
 * dw is float32 in the master layout and is ACCUMULATED (atomic adds): zero it first. */
typedef struct {
    int32_t n, hi, wi, cin;   /* x is (n, hi, wi, cin) */
    int32_t cout;
    int32_t ks;
    int32_t x_ups, x_relu;
    int32_t dy_ups;           /* dy is (n, ho/2, wo/2, cout), nearest-upsampled on load */
    int32_t dtype;            /* dtype of x and dy */
    int32_t variant;          /* a sum of the XMC_WGRAD_* fields below.  XMC_WGRAD_KERNEL_MASK, kernel choice: 0 = generic split-K
                                 kernel only (bring-up / float32), 1 = auto (phase-decomposed kernel, else LDS-DMA kernel, else
                                 register-staged patch kernel, else generic), 2 = as 1 without the phase and LDS-DMA kernels (A/B);
                                 XMC_WGRAD_OVERWRITE: dw / db = alpha * (...) instead of += -- the FIRST write of a gradient
                                 nobody zeroed (the optimiser then need not clear what it consumed, and the reducing pass
                                 reads no old value); needs the workspace of xmc_conv2d_wgrad_ws for split launches;
                                 every other field: A/B hooks of tools/ (0 = the shipped choice) */
    float alpha;
} xmc_wgrad_desc;
/* xmc_wgrad_desc.variant */
#define XMC_WGRAD_KERNEL_MASK 0xf
#define XMC_WGRAD_TUNE_SHIFT 4            /* LDS-DMA kernel, four bits: bit 0 launch order, bits 1-3 workgroup target */
#define XMC_WGRAD_TUNE_MASK 0xf
#define XMC_WGRAD_PHASE_TARGET_SHIFT 5    /* phase kernel, three bits: index of its workgroup target -- OVERLAPS the tune field's */
#define XMC_WGRAD_PHASE_TARGET_MASK 0x7   /* upper three bits (one sweep variable of tools/ drives either kernel) */
#define XMC_WGRAD_NO_PHASE 0x100          /* no phase-decomposed kernel */
#define XMC_WGRAD_FORCE_SHIFT 9           /* 1x1 LDS-DMA kernel, two bits: force 1 / 2 / 4 cin blocks per workgroup */
#define XMC_WGRAD_FORCE_MASK 0x3
#define XMC_WGRAD_NO_C96 0x800            /* no 96-cout tiles in the LDS-DMA kernel */
#define XMC_WGRAD_OVERWRITE 0x1000
#define XMC_WGRAD_NST3 0x2000             /* three-stage ring on the 4 x 4 maps too */

/* db (may be NULL): the bias gradient of the same convolution, db[cout] += alpha * sum_p dy'(p, cout),
 * fused into the weight-gradient kernel. */
int xmc_conv2d_wgrad(const xmc_wgrad_desc* d, const void* x, const void* dy, float* dw, float* db,
                     void* stream);
/* Deterministic split-K: with a workspace of xmc_conv2d_wgrad_workspace_bytes(d) bytes (no initialisation
 * needed) every pixel split writes its partial dW / db slab with plain stores and a second kernel adds the
 * slabs to dw / db in a FIXED order -- bit-reproducible gradients, no float atomics.  ws == NULL behaves
 * like xmc_conv2d_wgrad. */
int64_t xmc_conv2d_wgrad_workspace_bytes(const xmc_wgrad_desc* d);
int xmc_conv2d_wgrad_ws(const xmc_wgrad_desc* d, const void* x, const void* dy, float* dw, float* db,
                        void* ws, int64_t ws_bytes, void* stream);

/* float32 master [cout][taps][cin] -> forward copy [cout][taps][cin] and dgrad copy
 * [cin][taps flipped][cout] in `dtype`, both multiplied by *inv_sigma when inv_sigma != NULL
 * (kernel / (sigma + eps), xmcgan/libml/layers.py:219-221).  Either output may be NULL.
 * packed bit 0 / bit 1: write the forward / dgrad copy in MFMA-fragment order (see xmc_pack_conv_weight;
 * bf16 only, cin % 32 == 0 resp. cout % 32 == 0; the buffer holds ceil(rows / 32) * 32 rows). */
int xmc_prep_conv_weight(const float* w, const float* inv_sigma, void* w_fwd, void* w_dgrad,
                         int32_t cout, int32_t taps, int32_t cin, int32_t dtype, int32_t packed, void* stream);

/* Prepared bf16 weights [cout][taps][cin] (forward or dgrad copy) -> MFMA-fragment order
 *   [ceil(cout/32)][cin/32][tap][k16 half][lane 0..63][8]   lane = (k8 half) * 32 + cout % 32
 * (ceil(cout/32) * 32 * taps * cin elements; rows >= cout are zero) consumed by xmc_conv2d_nhwc with
 * desc.w_packed = XMC_CONV_PACKED: every MFMA A operand is then one coalesced 1 KiB load, no LDS staging of weights. */
int xmc_pack_conv_weight(const void* w, void* out, int32_t cout, int32_t taps, int32_t cin, void* stream);

/* Phase weights of a 3x3 layer that sits next to a 2x resampling (the generator blocks' conv3x3(upsample(.)),
 * xmcgan/nets/common.py:152-159, and the discriminator blocks' avg_pool(conv3x3(.)), common.py:76-78,131).  Two of the
 * three rows / columns of such a window read the same low-resolution pixel, so the layer equals four 2x2 convolutions
 * whose taps are SUMS of the 3x3 taps (formed here in float32, x *inv_sigma, rounded to bf16 once):
 *   fwd_mode 0 (layer = conv(upsample2(x))):  w_fwd in "out" order for desc.ups launches, w_dgrad (rows = cin) in "in"
 *                                             order for the pool_out launch that computes its data gradient;
 *   fwd_mode 1 (layer = avg_pool2(conv(x))):  w_fwd in "in" order for desc.pool_out launches, w_dgrad in "out" order for
 *                                             the ups launch that computes its data gradient.
 *   fwd_mode 2 (layer = a STRIDE-2 SAME 3x3 convolution of an even-sized map, flax padding (0, 1): y[o] = sum_r w[r] x[2o + r]
 *               -- xmcgan/utils/resnet_v1.py:70): single taps instead of sums (7 of the 16 entries are zero); w_fwd for a
 *               pool_out launch with alpha = 4 (y at half the resolution), w_dgrad for the ups launch that computes the adjoint.
 * Both outputs: fragment order with 16 taps, rows * 16 * k bf16 elements (cout % 32 == 0, cin % 32 == 0); pass them
 * with desc.w_packed = XMC_CONV_PACKED | XMC_CONV_PHASE.  Either may be NULL. */
int xmc_phase_conv_weight(const float* w, const float* inv_sigma, void* w_fwd, void* w_dgrad, int32_t cout, int32_t cin,
                          int32_t fwd_mode, void* stream);

/* ------------------------------------------------------------------------ dense / small GEMMs (K2)
 * C[b] = alpha * (*alpha_dev) * A[b] x B[b] + beta * C[b], float32, arbitrary element strides
 * (so NN / NT / TN need no copies); MFMA 32x32x2 f32 (exact fp32).  Replaces flax nn.Dense and
 * lax.dot_general (xmcgan/libml/layers.py:104-112), jnp.matmul in
 * xmcgan/libml/attention_lib.py:64-67,120,126,210,218.  alpha_dev may be NULL.
 * ws (may be NULL): xmc_gemm_ws_floats(m, n, k, batch, bf16_mfma) floats of scratch.  Products with few
 * output tiles and K >= 1024 split K over several workgroups ONLY when ws is given: each K range writes its
 * partial product to ws and a second kernel adds the partials in a fixed order (no float atomics). */
int64_t xmc_gemm_ws_floats(int32_t m, int32_t n, int32_t k, int32_t batch, int32_t bf16_mfma);
int xmc_gemm_f32(const float* a, const float* b, float* c, int32_t m, int32_t n, int32_t k,
                 int64_t sab, int64_t sam, int64_t sak, int64_t sbb, int64_t sbk, int64_t sbn,
                 int64_t scb, int64_t ldc, float alpha, const float* alpha_dev, float beta,
                 int32_t batch, float* ws, void* stream);

/* Same contract, but the float32 operands are rounded to bf16 on their way into LDS and multiplied on
 * v_mfma_f32_32x32x16_bf16 (float32 accumulate): the bf16 training mode's region-word similarity GEMMs
 * (xmcgan/libml/attention_lib.py:143-166, B^2*R*T*E products).  The float32 parity mode never calls it. */
int xmc_gemm_f32_bf16mfma(const float* a, const float* b, float* c, int32_t m, int32_t n, int32_t k,
                 int64_t sab, int64_t sam, int64_t sak, int64_t sbb, int64_t sbk, int64_t sbn,
                 int64_t scb, int64_t ldc, float alpha, const float* alpha_dev, float beta,
                 int32_t batch, float* ws, void* stream);

/* y[a][c] (+)= scale * sum_r f(x[a][r][c]),  f = relu or identity; x in `dtype`, y float32.
 * Bias gradients, the projection head's spatial SUM (xmcgan/nets/xmc_net.py:97-98) and
 * the tile/broadcast adjoints. */
int xmc_reduce_mid(const void* x, float* y, int64_t a, int64_t r, int64_t c, int32_t dtype,
                   int32_t relu, float scale, int32_t accumulate, void* stream);
/* Atomic-free two-stage variant (partial rows in `ws`, xmc_reduce_mid_ws_floats(a, r, c) floats, no
 * initialisation; fixed summation order -> bit-reproducible).  ws == NULL behaves like xmc_reduce_mid. */
int64_t xmc_reduce_mid_ws_floats(int64_t a, int64_t r, int64_t c);
int xmc_reduce_mid_ws(const void* x, float* y, float* ws, int64_t a, int64_t r, int64_t c, int32_t dtype,
                      int32_t relu, float scale, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------- batch norm + conditional affine (K3)
 * flax.linen.BatchNorm(use_scale=False, use_bias=False, momentum .9, eps 1e-5) as configured at
 * xmcgan/nets/xmc_net.py:192-201, fused with (Local)ConditionalBatchNorm's affine
 * x_hat * (gamma + 1) + beta (xmcgan/libml/layers.py:256-257,271-272) and the following ReLU.
 * sums: 2*C floats {sum, sum of squares}, ACCUMULATED (zero first). */
int xmc_bn_stats(const void* x, float* sums, int64_t pixels, int32_t c, int32_t dtype, void* stream);
int xmc_bn_finalize(const float* sums, float* mean, float* rstd, float* run_mean, float* run_var,
                    int64_t pixels, int32_t c, float eps, float momentum, int32_t update_running,
                    void* stream);
/* eval mode: mean/rstd from running statistics */
/* Batch statistics + finalize without same-address atomics (the path the step uses): <= 512 workgroups
 * write one row of partial [sum, sum of squares] each into `ws` (xmc_bn_stats_ws_floats(pixels, c) floats,
 * no initialisation needed), a second small kernel reduces the rows in a FIXED order -- bit-reproducible
 * statistics -- and produces mean / rstd / the running statistics exactly as xmc_bn_finalize. */
int64_t xmc_bn_stats_ws_floats(int64_t pixels, int32_t c);
int xmc_bn_batch_stats(const void* x, float* ws, float* mean, float* rstd, float* run_mean, float* run_var,
                       int64_t pixels, int32_t c, int32_t dtype, float eps, float momentum,
                       int32_t update_running, void* stream);
int xmc_bn_from_running(const float* run_mean, const float* run_var, float* mean, float* rstd,
                        int32_t c, float eps, void* stream);
/* Cross-replica BatchNorm groups (ABI 28; flax nn.BatchNorm(axis_name="batch", axis_index_groups=groups),
 * xmcgan/nets/xmc_net.py:192-201): the statistics pass split at the point where the replicas of a group exchange.
 * xmc_bn_batch_sums: the two stages of xmc_bn_batch_stats stopped at sums[2c] = {sum x, sum x^2} of this replica
 *   (ws: xmc_bn_stats_ws_floats(pixels, c) floats; same partial geometry, same fixed order, no atomics, nothing to zero).
 * xmc_bn_finalize_rows: rows[g][2c], one such row per replica in rank order, added in a fixed order (row r in lane group
 *   r % 16, the groups in index order: plain index order for g <= 16) and finalized with 1 / (g * pixels_per_row) by the
 *   kernel that finalizes xmc_bn_batch_stats: the same bits on every replica; g == 1 is bit-equal to xmc_bn_batch_stats.
 * xmc_rows_mean: out[i] = (sum_r rows[r][i]) / g in the same order -- the group mean of the backward sums s[2c] of
 *   xmc_cbn_bwd_sums (xmc_cbn_act_bwd_dx divides by the local pixel count); g == 1: out is the row, bit for bit. */
int xmc_bn_batch_sums(const void* x, float* ws, float* sums, int64_t pixels, int32_t c, int32_t dtype,
                      void* stream);
int xmc_bn_finalize_rows(const float* rows, int32_t g, float* mean, float* rstd, float* run_mean,
                         float* run_var, int64_t pixels_per_row, int32_t c, float eps, float momentum,
                         int32_t update_running, void* stream);
int xmc_rows_mean(const float* rows, int32_t g, int32_t n, float* out, void* stream);
/* gamma/beta: one row of c values per conditioning cell (n * hc * hc cells, hc | h; hc == 1:
 * per-sample conditional BN), rows `cstride` ELEMENTS apart (cstride >= c): gamma and beta are normally
 * the two halves of ONE (cells, 2c) conv / dense output (gamma = p, beta = p + c, cstride = 2c).
 * gb_dtype = XMC_F32, or XMC_BF16 (round 5: what LocalConditionalBatchNorm's nn.Conv(dtype=bfloat16) produces in the
 * reference's bf16 mode, xmcgan/libml/layers.py:261-273; needs dtype == XMC_BF16, c % 8 == 0, cstride % 8 == 0 and
 * 16-byte aligned gamma / beta -- and, in the backward passes, dgamma / dbeta of the same type). */
int xmc_cbn_act_fwd(const void* x, const float* mean, const float* rstd, const void* gamma,
                    const void* beta, void* y, int32_t n, int32_t h, int32_t w, int32_t c,
                    int32_t hc, int32_t cstride, int32_t relu, int32_t dtype, int32_t gb_dtype, void* stream);
/* The same with an MX-fp8 twin of y (bf16, c % 64 == 0): y8 [pixels][c / 64][80] as xmc_mx8_quantize(y, 0) would write
 * it, for the 3x3 convolution that consumes y when config.conv_fp8 is set. */
int xmc_cbn_act_fwd_mx8(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        void* y, void* y8, int32_t n, int32_t h, int32_t w, int32_t c, int32_t hc, int32_t cstride,
                        int32_t relu, void* stream);
/* pass 1: dgamma/dbeta per conditioning cell (exclusive writes, same row stride as gamma/beta) */
int xmc_cbn_act_bwd_cells(const void* dy, const void* x, const float* mean, const float* rstd,
                          const void* gamma, const void* beta, void* dgamma, void* dbeta,
                          int32_t n, int32_t h, int32_t w, int32_t c, int32_t hc, int32_t cstride,
                          int32_t relu, int32_t dtype, int32_t gb_dtype, void* stream);
/* s[0:C] = sum_cells (gamma+1)*dbeta ; s[C:2C] = sum_cells (gamma+1)*dgamma.  Two-stage through `ws`
 * (xmc_cbn_bwd_sums_ws_floats(cells, c) floats; neither ws nor s needs initialising): workgroups write partial
 * rows, a fixed-order row reduction writes s -- atomic-free, bit-reproducible. */
int64_t xmc_cbn_bwd_sums_ws_floats(int64_t cells, int32_t c);
int xmc_cbn_bwd_sums(const void* gamma, const void* dgamma, const void* dbeta, float* s, float* ws,
                     int64_t cells, int32_t c, int32_t cstride, int32_t gb_dtype, void* stream);
/* pass 2: dx = rstd * (g*(gamma+1) - s1/P - x_hat * s2/P) */
int xmc_cbn_act_bwd_dx(const void* dy, const void* x, const float* mean, const float* rstd,
                       const void* gamma, const void* beta, const float* s, void* dx,
                       int32_t n, int32_t h, int32_t w, int32_t c, int32_t hc, int32_t cstride,
                       int32_t relu, int32_t dtype, int32_t gb_dtype, void* stream);

/* ------------------------------------------------------------------------------ resampling / pointwise
 * y = scale * sum_{2x2} x (+ res): dsample (xmcgan/nets/common.py:23-55) with scale .25 and the
 * adjoint of nearest upsample with scale 1. */
int xmc_pool2(const void* x, const void* res, void* y, int32_t n, int32_t h, int32_t w, int32_t c,
              float scale, int32_t dtype, void* stream);
/* xmc_pool2 that also writes xr = max(x, 0) at full resolution (xr NULL: xmc_pool2).  A down-sampling DiscBlock
 * (xmcgan/nets/common.py:67-78) pools its input x for the shortcut and feeds relu(x) to its first convolution; the
 * pooling pass holds every element of x, so it emits relu(x) once and neither the convolution nor its weight gradient
 * applies the ReLU again. */
int xmc_pool2_relu(const void* x, const void* res, void* y, void* xr, int32_t n, int32_t h, int32_t w, int32_t c,
                   float scale, int32_t dtype, void* stream);
/* y (n,h,w,32)[tap*c + j] = x (n,h,w,c)[pixel + sign * offset(tap)][j], zero outside the image and for the
 * padding channels (ks*ks*c <= 32): the im2col of an RGB-like tensor (sign = +1), or the shifted copies of a
 * 3-channel output gradient (sign = -1).  Lets the 3-channel first / last convolutions
 * (xmcgan/nets/common.py:127, xmcgan/nets/xmc_net.py:245) and their weight gradients run as 1x1 convolutions
 * on the MFMA kernels. */
int xmc_expand_taps(const void* x, void* y, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ks,
                    int32_t sign, int32_t dtype, void* stream);
/* adjoint of xmc_reduce_mid(relu=1): dx[a][r][c] = x[a][r][c] > 0 ? dpool[a][c] : 0
 * (backward of activation_fn + jnp.sum(x, axis=(1,2)), xmcgan/nets/xmc_net.py:97-98). */
int xmc_bcast_relu_bwd(const float* dpool, const void* x, void* dx, int64_t a, int64_t r, int64_t c,
                       int32_t dtype, void* stream);
/* (tanh(x)+1)/2 (xmcgan/nets/xmc_net.py:246-247) */
int xmc_tanh_out_fwd(const void* x, void* y, int64_t n, int32_t dtype, void* stream);
/* dx = dy * 0.5 * (1 - (2y-1)^2) */
int xmc_tanh_out_bwd(const void* dy, const void* y, void* dx, int64_t n, int32_t dtype, void* stream);
int xmc_cast(const void* x, int32_t dtype_in, void* y, int32_t dtype_out, int64_t n, void* stream);
/* out = a + b (same dtype) */
int xmc_add(const void* a, const void* b, void* out, int64_t n, int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------- attention (K7)
 * attention_for_g, xmcgan/libml/attention_lib.py:194-219 with the mask of
 * xmcgan/nets/xmc_net.py:225-228: region (b, r, e) in `dtype`; words_n (b, t, e) float32 already
 * l2-normalised; ctx (b, r, e) in `dtype`; attn (b, r, t) float32; rinv (b, r) float32. */
int xmc_attn_g_fwd(const void* region, const float* words_n, const float* max_len, void* ctx,
                   float* attn, float* rinv, int32_t b, int32_t r, int32_t t, int32_t e,
                   float gamma, int32_t dtype, void* stream);
int xmc_attn_g_bwd(const void* dctx, const void* region, const float* words_n, const float* attn,
                   const float* rinv, void* dregion, int32_t b, int32_t r, int32_t t, int32_t e,
                   float gamma, int32_t dtype, void* stream);
/* attention_for_g on the matrix cores (bf16 tensors; r % 128 == 0, e % 64 == 0, t <= 64 -- xmc_attn_g_mfma_supported): both
 * products as MFMA 32x32x16 tiles with the words as the A operand, softmax in registers, float32 accumulation.  t <= 32 runs
 * the one-word-block kernels; 32 < t <= 64 (Localized Narratives) the two-block kernels, which stage the words and then the
 * transposed words in ONE LDS region in turn (144 e bytes, e <= 1088).  Same
 * arguments and results as xmc_attn_g_fwd / xmc_attn_g_bwd with dtype = XMC_BF16 (the float32 parity mode keeps those: the
 * attention indices are held bit-exact against the float32 oracle there). */
int xmc_attn_g_mfma_supported(int32_t b, int32_t r, int32_t t, int32_t e);
int xmc_attn_g_fwd_mfma(const void* region, const float* words_n, const float* max_len, void* ctx, float* attn,
                        float* rinv, int32_t b, int32_t r, int32_t t, int32_t e, float gamma, void* stream);
int xmc_attn_g_bwd_mfma(const void* dctx, const void* region, const float* words_n, const float* attn, const float* rinv,
                        void* dregion, int32_t b, int32_t r, int32_t t, int32_t e, float gamma, void* stream);
/* The same two launches with ctx / dctx as a COLUMN SLICE of a wider tensor (row pitch ld_* elements, % 8 == 0, >= e): the
 * generator concatenates the context with the global condition along the channel axis (xmcgan/nets/xmc_net.py:231-235) --
 * the forward writes its context straight into that tensor, the backward reads its cotangent out of that tensor's gradient,
 * and neither a concatenation nor a contiguous copy of the slice is made. */
int xmc_attn_g_fwd_mfma_ld(const void* region, const float* words_n, const float* max_len, void* ctx, int32_t ld_ctx, float* attn,
                           float* rinv, int32_t b, int32_t r, int32_t t, int32_t e, float gamma, void* stream);
int xmc_attn_g_bwd_mfma_ld(const void* dctx, int32_t ld_dctx, const void* region, const float* words_n, const float* attn,
                           const float* rinv, void* dregion, int32_t b, int32_t r, int32_t t, int32_t e, float gamma, void* stream);


/* l2_normalize along the last axis, xmcgan/libml/attention_lib.py:30-33:
 * y = x * rsqrt(max(sum x^2, 1e-12)); x in dtype_in, y float32, inv (rows) float32. */
int xmc_l2norm_rows_fwd(const void* x, float* y, float* inv, int64_t rows, int32_t cols,
                        int32_t dtype_in, void* stream);
/* dx (dtype_out) = inv * (dy - y * <y, dy>)  (or inv * dy when the clamp was active) */
int xmc_l2norm_rows_bwd(const float* dy, const float* y, const float* inv, void* dx, int64_t rows,
                        int32_t cols, int32_t dtype_out, void* stream);

/* ------------------------------------------------------------------------- word-level loss (K8)
 * word_loss / attention, xmcgan/libml/attention_lib.py:105-191, restructured:
 *   S[(j,r)][(i,t)] = R^_j[r] . W^_i[t]  (GEMM),  G_j = R^_j R^_j^T  (GEMM),
 *   alpha = softmax_r(gamma1 * S + mask),  nn = sum_r alpha S,  H = G_j alpha (GEMM),
 *   q = sum_r alpha H,  cos = nn / sqrt(q)   (== cosine_similarity(word, context)).
 * Matrices are float32 (b*r) x (b*t), row-major.  max_len (b) float32. */
int xmc_wl_softmax(const float* s, const float* max_len, float* alpha, float* nn, int32_t b,
                   int32_t r, int32_t t, float gamma1, void* stream);
int xmc_wl_qdot(const float* alpha, const float* h, float* q, int32_t b, int32_t r, int32_t t,
                void* stream);
/* sim_t[i][j] = gamma3/gamma2 * logsumexp_t(gamma2 * nn/sqrt(q) + mask); pi = softmax_t(...) */
int xmc_wl_rows(const float* nn, const float* q, const float* max_len, float* sim_t, float* pi,
                int32_t b, int32_t t, float gamma2, float gamma3, void* stream);
/* backward of the column stage: given dsim_t (b x b), writes dS (in place over h) and
 * alpha_scaled = alpha * dq (for dG_j = alpha_scaled alpha^T). */
int xmc_wl_bwd_cols(const float* s, const float* alpha, float* h_ds, const float* nn, const float* q,
                    const float* pi, const float* dsim_t, float* alpha_scaled, int32_t b, int32_t r,
                    int32_t t, float gamma1, float gamma3, void* stream);

/* word_loss fused on the matrix cores (round 4; bf16 mode, r == 256, e % 128 == 0 -- xmc_wl_fused_supported): the same
 * quantities as the entries above (xmcgan/libml/attention_lib.py:105-127 `attention`, :130-191 `word_loss`) without the
 * float32 (b*r) x (b*t) score / probability / H tensors.  ldp = xmc_wl_fused_ldp(b, t) = b*t rounded up to 64: the padded
 * column count of every [.., ldp] tensor below (padding columns hold zeros).
 *   xmc_wl_prep_regions  x (b, r, e) bf16 -> rn = l2_normalize(x) (:30-33) bf16 (b, r, e), rnT (b, e, r), rinv (b*r) float32
 *   xmc_wl_prep_words    words_n (ld = b*t, e) float32, already normalised -> w (ldp, e) bf16 (rows >= ld zero), wT (e, ldp)
 *   xmc_wl_tn_gemm       out[z][x][y] = alpha * (sum_k x0[z][x][k] y0[z][y][k] + sum_k x1[z][x][k] y1[z][y][k]); bf16 operands
 *                        with k contiguous (row pitches ld*, batch strides s* in elements, 0 = shared); k0, k1 % 64 == 0
 *                        (k1 = 0: one segment); rows_x, rows_y % 128 == 0; out bf16 or float32 (out_f32), row pitch ldo
 *   xmc_wl_cols_fwd      per (image j, column (i,t)): S = R^_j W^^T, alpha = softmax over the r regions of gamma1 * S (+ mask),
 *                        nn = sum alpha S, q = alpha^T G_j alpha with g = R^_j R^_j^T (b, r, r) bf16 -> nn, q (b, b*t) float32,
 *                        the inputs of xmc_wl_rows
 *   xmc_wl_cols_bwd      recomputes S / alpha / H and writes dS, alpha * dq and alpha as bf16 (b, r, ldp) given dsim_t (b, b)
 *                        and pi (b, b*t) (same formulas as xmc_wl_bwd_cols)
 *   xmc_l2norm_rows_bwd_bf16y   xmc_l2norm_rows_bwd with the normalised rows y in bf16 */
int xmc_wl_fused_supported(int32_t b, int32_t r, int32_t t, int32_t e);
int xmc_wl_fused_ldp(int32_t b, int32_t t);
int xmc_wl_prep_regions(const void* x, void* rn, void* rnT, float* rinv, int32_t b, int32_t r, int32_t e, void* stream);
int xmc_wl_prep_words(const float* words_n, void* w, void* wT, int32_t ld, int32_t ldp, int32_t e, void* stream);
int xmc_wl_tn_gemm(const void* x0, int64_t sx0, int32_t ldx0, const void* y0, int64_t sy0, int32_t ldy0, int32_t k0,
                   const void* x1, int64_t sx1, int32_t ldx1, const void* y1, int64_t sy1, int32_t ldy1, int32_t k1,
                   void* out, int64_t so, int32_t ldo, int32_t out_f32, float alpha, int32_t rows_x, int32_t rows_y,
                   int32_t batch, void* stream);
int xmc_wl_cols_fwd(const void* rn, const void* w, const void* g, const float* max_len, float* nn, float* q, int32_t b,
                    int32_t t, int32_t e, int32_t ldp, float gamma1, void* stream);
int xmc_wl_cols_bwd(const void* rn, const void* w, const void* g, const float* max_len, const float* dsim_t,
                    const float* pi, void* ds, void* as, void* al, int32_t b, int32_t t, int32_t e, int32_t ldp,
                    float gamma1, float gamma3, void* stream);
int xmc_l2norm_rows_bwd_bf16y(const float* dy, const void* y, const float* inv, void* dx, int64_t rows, int32_t cols,
                              int32_t dtype_out, void* stream);

/* --------------------------------------------------------------- contrastive / GAN scalar losses (K9, K11)
 * Symmetric cross-entropy with identity labels over a b x b logit matrix L (row direction)
 * and its transpose: contrastive_loss / word_loss tails, xmcgan/libml/attention_lib.py:61-74,
 * :175-182, xmcgan/libml/losses.py:47-51.  *loss += weight * (mean_i CE(L[i,:], i) + mean_i
 * CE(L[:,i], i)); dlogits (may be NULL) = weight * d loss / dL; stats (may be NULL) receives
 * get_statistics (attention_lib.py:36-43) averaged over both directions: {accuracy, entropy}. */
int xmc_xent_sym(const float* logits, int32_t b, float weight, float* loss, float* dlogits,
                 float* stats, void* stream);
/* out[4] = {d_loss, g_loss, c_loss_d, c_loss_g} (xmcgan/xmc_gan.py:58-71,146-154): loss_vec[5] = {fake word, real word, fake sentence,
 * real sentence, image contrastive}, hinge[2] = {hinge_d, hinge_g}. */
int xmc_loss_assemble(const float* loss_vec, const float* hinge, float* out, void* stream);
/* contrastive_loss (xmcgan/libml/attention_lib.py:46-79) without the normalised copies and the GEMM launches (round 5):
 * xmc_cl_logits: logits[i][j] = <a_i, b_j> / (|a_i| |b_j|) * inv_temperature for a, b (n, d) float32, with l2_normalize's clamp
 * (attention_lib.py:30-33); ainv / binv (n) receive 1 / |row| for the backward pass.  Follow with xmc_xent_sym.
 * xmc_cl_bwd: the pullback onto ONE operand x (trans = 0: x = a, coefficients dlogits[i][j]; trans = 1: x = b, dlogits[j][i]),
 * through the normalisation: out[i] (+)= xinv_i (g_i - xn_i <xn_i, g_i>), g_i = inv_temperature * sum_j dl(i, j) yinv_j y_j.
 * d <= 2048. */
int xmc_cl_logits(const float* a, const float* b, float* logits, float* ainv, float* binv, int32_t n, int32_t d,
                  float inv_temperature, void* stream);
int xmc_cl_bwd(const float* dlogits, const float* x, const float* y, const float* xinv, const float* yinv, float* out,
               int32_t n, int32_t d, float inv_temperature, int32_t trans, int32_t accumulate, void* stream);
/* hinge_loss, xmcgan/libml/losses.py:30-35: logit (2b) = [real; fake].
 * *d_loss += mean(relu(1-real)+relu(1+fake)); *g_loss += -mean(fake); gradients (2b) each. */
int xmc_hinge(const float* logit, int32_t b, float* d_loss, float* g_loss, float* dlogit_d,
              float* dlogit_g, void* stream);
/* projection head, xmcgan/nets/xmc_net.py:99-104: out[n] = bias + sum_c pool[n][c] *
 * (w[c] * (*inv_sigma) + emb[n % b][c]) */
int xmc_proj_head_fwd(const float* pool, const float* w, const float* inv_sigma, const float* bias,
                      const float* emb, float* out, int32_t n2, int32_t b, int32_t c, void* stream);
/* dpool[n][c] (+)= dout[n] * (w[c]*inv_sigma + emb[n%b][c]); demb[i][c] (+)= sum_{n%b==i} dout[n]*pool[n][c] */
int xmc_proj_head_bwd(const float* dout, const float* pool, const float* w, const float* inv_sigma,
                      const float* emb, float* dpool, float* demb, int32_t n2, int32_t b, int32_t c,
                      int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------ spectral norm (K6)
 * One power-iteration step, xmcgan/libml/layers.py:92-101, :209-220, on W viewed as
 * rows x cols float32 with u0 along `u_axis` (0: u over rows -- conv master [cout][K];
 * 1: u over cols -- dense kernels (in, out)).  Writes v (other axis), u_new, and
 * scal = {sigma, 1/(sigma+eps)}.  tmp: rows + cols + 4 floats of scratch. */
int xmc_spectral_power_iter(const float* w, const float* u0, float* u_new, float* v, float* scal,
                            float* tmp, int32_t rows, int32_t cols, int32_t u_axis, float eps,
                            void* stream);
/* Gradient through sigma: g <- (g - (<g,w> * inv_s) * outer(u, v)) * inv_s  in place
 * (u indexed along u_axis).  tmp: 1 float of scratch. */
int xmc_spectral_grad_fix(float* g, const float* w, const float* u, const float* v,
                          const float* scal, float* tmp, int32_t rows, int32_t cols, int32_t u_axis,
                          void* stream);

/* Batched form over ALL spectrally-normalised weights of a network (one descriptor table in device
 * memory; 4 + 1 launches per forward, 2 per backward instead of ~9 per weight).  Offsets are in floats
 * into the parameter / gradient arena (w_off), the flat u / v buffers (u_off, v_off) and the prepared
 * weight buffers (wf_off, wd_off, in elements).  blk_a / blk_b / blk_p are exclusive prefix sums of the
 * workgroups each entry owns in the three grids (host-computed, see ops.py::SpectralBank):
 *   A: ceil(rows / 4)                        B: ceil(cols / 128)   (one workgroup per 128 columns, all rows)
 *   P (prep table): taps * ceil(cin/32) * ceil(cout/32) for conv entries, 0 otherwise
 *   P (grad-fix table, a second copy of the table): ceil(rows * cols / 65536)
 * No float atomics anywhere: every matvec output element has one writer, <g,w> is kept as one partial per
 * 64K-element chunk (`dots`: `blocks` floats) and summed in a fixed order -- bit-reproducible.  u / v slices
 * (u_off, v_off) must start 16-byte aligned. */
typedef struct {
    int64_t w_off;
    int32_t rows, cols, u_axis;
    int32_t u_off, v_off;
    int32_t blk_a, blk_b;
    int32_t taps, is_conv;
    int64_t wf_off, wd_off;
    int32_t blk_p;
    int32_t packed;           /* as xmc_prep_conv_weight: bit 0 forward, bit 1 dgrad copy in fragment order; bit 2: a layer
                                 next to a 2x resampling whose launches read only the 16-tap copies of xmc_phase_conv_weight --
                                 xmc_sn_batched_prep leaves its 3x3 copies UNWRITTEN when bit 8 of its `dtype` argument is set */
} xmc_sn_entry;

int xmc_sn_batched_power_iter(const void* table, int32_t n, const float* params, const float* u0,
                              float* u_new, float* v, float* u_raw, float* scal, int32_t blocks_a,
                              int32_t blocks_b, int32_t nu_total, int32_t nv_total, float eps,
                              void* stream);
int xmc_sn_batched_prep(const void* table, int32_t n, const float* params, const float* scal,
                        void* wf_buf, void* wd_buf, int32_t blocks_p, int32_t dtype, void* stream);
int xmc_sn_batched_grad_fix(const void* table, int32_t n, const float* params, float* grads,
                            const float* u, const float* v, const float* scal, float* dots,
                            int32_t blocks, void* stream);

/* Round 4 -- prepared weights as a pure cast of W (1 / sigma rides in xmc_conv_desc.alpha_dev): one pass over each weight's
 * float32 master writes the fragment-ordered forward / data-gradient copies, the 16-tap phase copies of the layers next to a
 * 2x resampling (xmc_phase_conv_weight's outputs, modes 0 / 1) and -- for spectrally-normalised weights -- the row tiles'
 * partial sums of the power iteration's first product v_raw = W^T u0 (xmcgan/libml/layers.py:209-214).  Table entries: bf16
 * mode only, cout % 32 == cin % 32 == 0, taps 1 or 9.  part: sum over entries of (cout / 32) * taps * cin floats. */
typedef struct {
    int64_t w_off;            /* floats into the parameter arena ([cout][taps][cin] master) */
    int64_t wf_off, wd_off;   /* bf16 elements into the plain forward / data-gradient buffers */
    int64_t pf_off, pd_off;   /* bf16 elements into the phase forward / data-gradient buffers */
    int64_t part_off;         /* floats into `part` */
    int32_t cout, cin, taps;
    int32_t blk0;             /* first workgroup of the entry in the tile grid ((cout / 32) * (cin / 32) workgroups each) */
    int32_t flags;            /* bit 0 / 1: write the plain forward / data-gradient copy; bits 2-3: 0 no phase copies, 1 the
                                 layer is conv3x3(upsample2(.)), 2 avg_pool2(conv3x3(.)); bit 4: write the W^T u0 partials */
    int32_t u_off, v_off;     /* slices of the flat u0 / v buffers (floats) */
    int32_t blk_c;            /* first workgroup of the entry in the column-sum grid (ceil(taps * cin / 256) workgroups each) */
} xmc_wprep_entry;
int xmc_wprep_batched(const void* table, int32_t n, const float* params, const float* u0, void* wf_buf, void* wd_buf,
                      void* pf_buf, void* pd_buf, float* part, int32_t blocks, void* stream);
/* The power iteration of xmc_sn_batched_power_iter with the first product of the `wtab` weights taken from `part`
 * (xmc_wprep_batched) and that of the remaining weights (`irr`: an xmc_sn_entry table with its own blk_a / blk_b prefixes;
 * n_irr may be 0) computed here; `table` lists all n weights. */
int xmc_sn_power_iter_fused(const void* table, int32_t n, int32_t blocks_a, int32_t blocks_b, const void* irr, int32_t n_irr,
                            int32_t irr_blocks_a, int32_t irr_blocks_b, const void* wtab, int32_t n_w, int32_t blocks_c,
                            const float* params, const float* u0, const float* part, float* u_new, float* v, float* u_raw,
                            float* scal, float eps, void* stream);
/* kvec[i] = <G_i, W_i> / (sigma_i + eps) (table = the dot-chunk table of xmc_sn_batched_grad_fix): first half of the gradient
 * through sigma; the second half is applied by xmc_adam_ema_dev_sn while it reads the gradient. */
int xmc_sn_batched_dot(const void* table, int32_t n, const float* params, const float* grads, const float* scal,
                       float* dots, float* kvec, int32_t blocks, void* stream);

/* ---------------------------------------------------------------------------------- optimiser (K12)
 * flax.optim.Adam.apply_gradient (xmcgan/xmc_gan.py:172-173,252) over a flat float32 arena, with
 * the 1/world gradient scale of lax.pmean (xmc_gan.py:170-171,251) and the EMA of
 * xmc_gan.py:174-177 fused.  ema may be NULL.  c1 = 1-beta1^t, c2 = 1-beta2^t. */
int xmc_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr,
                 float beta1, float beta2, float eps, float c1, float c2, float grad_scale,
                 float ema_decay, void* stream);
/* Same update with the optimiser's step counter in DEVICE memory so that a captured hipGraph replays
 * consecutive steps: step_state is 4 float32 slots, [0] = t as int32 bits (0 before the first step),
 * [1], [2] = 1/(1-beta1^t), 1/(1-beta2^t), refreshed (in double) by a one-thread kernel launched in
 * front of the update (beta1 / beta2 are doubles so that 1-beta^t matches the host formula).  Each call
 * advances t by one. */
int xmc_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr,
                     double beta1, double beta2, float eps, float* step_state, float grad_scale,
                     float ema_decay, void* stream);

/* xmc_adam_ema_dev that also (a) overwrites the gradient it consumed with zeros (zero_grads == 1; 2: writes the gradient with
 * the sigma term applied back instead, 0: leaves it) and (b) applies the
 * gradient through sigma of the spectrally-normalised tensors while reading it (map != NULL: one int16 per 64 arena elements
 * = index of the owning entry of `table`, or -1, or -2 = "leave this tensor alone" (xmc_adam_wprep_tiles updates it); kvec
 * from xmc_sn_batched_dot; u, v, scal of the forward's power iteration):
 * G <- (G - kvec_i u (x) v) / (sigma_i + eps), xmcgan/libml/layers.py:217-219.  `map` without `table`: skip marks only. */
int xmc_adam_ema_dev_sn(float* p, float* g, float* m, float* v, float* ema, int64_t n, float lr, double beta1,
                        double beta2, float eps, float* step_state, float grad_scale, float ema_decay,
                        int32_t zero_grads, const void* map, const void* table, int32_t n_entries,
                        const float* kvec, const float* scal, const float* u, const float* vv, void* stream);
/* Round 5 -- the optimiser emits the prepared weights (W-bar's copies are a pure function of W, xmcgan/libml/layers.py:209-221,
 * and the optimiser holds the new W in registers): the Adam (+ EMA) update of the weights of an xmc_wprep_batched `table`,
 * element for element the arithmetic of xmc_adam_ema_dev_sn (gradient through sigma, zero_grads modes), followed by that
 * table's preparation from the UPDATED tiles -- fragment-ordered / phase copies and, for spectral entries (flags bit 4, bank
 * index in flags >> 8), W_new^T u as partial rows (`u` = this half step's new u = the next power iteration's u0).  Call
 * xmc_adam_ema_dev_sn on the same arena FIRST, with a `map` that carries -2 on these tensors (it advances `step_state` and
 * leaves them alone; a map without `table` is allowed there: skip marks only).  kvec / scal / u / vv NULL: plain arena. */
int xmc_adam_wprep_tiles(const void* table, int32_t n, int32_t blocks, float* p, float* g, float* m, float* v, float* ema,
                         float lr, double beta1, double beta2, float eps, const float* step_state, float grad_scale,
                         float ema_decay, int32_t zero_grads, const float* kvec, const float* scal, const float* u,
                         const float* vv, void* wf_buf, void* wd_buf, void* pf_buf, void* pd_buf, float* part, void* stream);


/* -------------------------------------------------------- frozen ResNet-50 feature path
 * xmcgan/xmc_gan.py:74-90, xmcgan/utils/pretrained_model_utils.py:102-127, xmcgan/utils/resnet_v1.py:60-186.
 * ResNet's feature maps (112^2 .. 7^2) live on power-of-two CANVASES (valid region top-left, margin zero) so its
 * convolutions run on xmc_conv2d_nhwc; these entry points are the rest.  dtype = XMC_F32 | XMC_BF16.
 *  - xmc_resize_bilinear: jax.image.resize(..., "bilinear") of x (n, hs, ws, c) into the hd x wd region of the
 *    canvas y (n, hc, wc, c): triangle filter on half-pixel centres, widened by max(hs / hd, 1) (jax anti-aliases by
 *    default when shrinking, e.g. 256 px -> 224), weights normalised over the in-bounds taps; backward = 1: x is dy
 *    on the canvas, y receives dx.
 *  - xmc_stem_im2col: the 7x7 stride-2 SAME stem conv (resnet_v1.py:148-154) as im2col of the (n, hc, wc, 3) image
 *    canvas (valid hv x wv) into col (n, ho, wo, kp >= 147), k = tap * 3 + ch; backward = 1: col2im (x = dcol).
 *  - xmc_maxpool3x3s2: nn.max_pool((3,3), strides (2,2), "SAME") (resnet_v1.py:156) canvas -> half-size canvas; idx
 *    (uint8, shape of y, may be NULL) receives the in-window position 0..8 of each window's first maximum;
 *    xmc_maxpool3x3s2_bwd: the adjoint (the gradient of a window goes to that element, as XLA's select-and-scatter).
 *  - xmc_zero_margin: zero a canvas outside its valid region, in place.
 *  - xmc_subsample2: small[o] = large[2 o + off] (the stride-2 view of a stride-1 convolution: off = 1 for flax's
 *    3x3, 0 for its 1x1 SAME stride-2 convs); scatter = 1: the adjoint (zero insertion into `large`).
 *  - xmc_add_relu: o = relu(a + b) (post-activation residual, resnet_v1.py:86); xmc_relu_bwd: g = (dy + dy2) * (out > 0). */
int xmc_resize_bilinear(const void* x, void* y, int32_t n, int32_t hs, int32_t ws, int32_t c, int32_t hd,
                        int32_t wd, int32_t hc, int32_t wc, int32_t backward, int32_t dtype, void* stream);
int xmc_stem_im2col(const void* x, void* col, int32_t n, int32_t hc, int32_t wc, int32_t hv, int32_t wv,
                    int32_t ho, int32_t wo, int32_t kp, int32_t backward, int32_t dtype, void* stream);
/* The stem as ONE implicit-GEMM launch (round 6, bf16): y canvas (n, ho, wo, 64), valid (hov, wov), <- conv 7x7 stride 2 SAME (2 before,
 * 3 after) of the image canvas x (n, hc, wc, 3) whose valid rows are hv and whose margin is ZERO (xmc_resize_bilinear's output), plus
 * bias (the folded init_bn; no ReLU: xmcgan/utils/resnet_v1.py:148-156).  Replaces xmc_stem_im2col + the pointwise GEMM: the 160-wide
 * columns (587 MB per 112 images) are never written.  wfrag: 64 x 176 bf16 in MFMA A-fragment order [cout / 32][k-step 0..10][lane][8] --
 * element e of lane l of fragment (cb, ks) = W[cb * 32 + (l & 31)][ky][kx][ch] with ky * 24 + kx * 3 + ch = ks * 16 + (l >> 5) * 8 + e
 * (zero where kx * 3 + ch >= 21 or ky >= 7).  wc <= 256, wov <= 128.  Only the valid corner of y is written (the caller keeps the
 * margins zero, as for the COMPACT pointwise launches). */
int xmc_stem_conv7x7s2(const void* x, const void* wfrag, const float* bias, void* y, int32_t n, int32_t hc, int32_t wc,
                       int32_t hv, int32_t ho, int32_t wo, int32_t hov, int32_t wov, void* stream);
/* ... and its data gradient onto the image as ONE launch (jax.vjp of the same convolution; replaces the pointwise GEMM 64 -> 160 into
 * im2col columns + xmc_stem_im2col(backward = 1)): dx canvas (n, hc, wc, 3), valid corner 2 hov x 2 wov written (margin untouched), <-
 * ds canvas (n, ho, wo, 64) with valid (hov, wov) (margin not read); bf16.  Per low-resolution pixel (Y, X) the 2 x 2 image pixels it
 * covers are 12 outputs r = (2 py + px) * 3 + c of a 4 x 4-tap correlation over ds: dx[2Y + py][2X + px][c] = sum_{t, u = 0..3} sum_co
 * ds[Y + 1 - t][X + 1 - u][co] W[co][2t + py][2u + px][c].  wfrag: 64 x 1 KiB fragments [channel half][tap t * 4 + u][k-step 0..1][lane][8],
 * element e of lane l = W[co][2t + py][2u + px][c] with l & 31 = (2 py + px) * 3 + c (rows >= 12 and taps beyond 6: zero),
 * co = half * 32 + k-step * 16 + (l >> 5) * 8 + e.  wov <= 128. */
int xmc_stem_conv7x7s2_dgrad(const void* ds, const void* wfrag, void* dx, int32_t n, int32_t ho, int32_t wo, int32_t hov,
                             int32_t wov, int32_t hc, int32_t wc, void* stream);
int xmc_maxpool3x3s2(const void* x, void* y, void* idx, int32_t n, int32_t hc, int32_t wc, int32_t c, int32_t hv,
                     int32_t wv, int32_t dtype, void* stream);
int xmc_maxpool3x3s2_bwd(const void* dy, const void* idx, void* dx, int32_t n, int32_t hc, int32_t wc, int32_t c,
                         int32_t hv, int32_t wv, int32_t dtype, void* stream);
int xmc_zero_margin(void* x, int32_t n, int32_t hc, int32_t wc, int32_t c, int32_t hv, int32_t wv,
                    int32_t dtype, void* stream);
int xmc_subsample2(void* large, void* small, int32_t n, int32_t hc, int32_t wc, int32_t c, int32_t off,
                   int32_t scatter, int32_t dtype, void* stream);
int xmc_add_relu(const void* a, const void* b, void* o, int64_t n, int32_t dtype, void* stream);
int xmc_relu_bwd(const void* dy, const void* dy2, const void* out, void* g, int64_t n, int32_t dtype,
                 void* stream);

/* -------------------------------------------------------- Inception-v3 feature path (FID / Inception Score)
 * xmcgan/utils/inception_arch.py, inception_utils.py:102-130, eval_metrics.py.  Feature maps 299^2 .. 8^2 in their true
 * sizes (no canvases); eval-mode BatchNorm is folded into the weights and biases by the caller.  dtype = XMC_F32 | XMC_BF16.
 *  - xmc_inception_conv: y[:, :, :, y_off : y_off + cout] (rows of ldy elements) = act(conv(x[:, :, :, x_off : x_off + cin]
 *    (rows of ldx elements), w) + bias), act = ReLU when relu != 0.  w: [cout][kh * kw][cin] in `dtype`, bias float32 (may
 *    be NULL).  kh, kw in 1..7, stride 1 or 2, pad_t / pad_l zero rows / columns before the input (SAME at stride 1:
 *    (k - 1) / 2; VALID: 0), any hi, wi, ho, wo.  cout, cin, ldx, ldy, x_off, y_off multiples of 8 (XMC_EINVAL otherwise),
 *    except first = 1: the network's first layer (cin < 8, contiguous input, no padding), whose gather applies
 *    clip(2 x - 1, -1, 1) to every loaded value (inception_utils.py:125-127).  Fixed tiles, no split-K: the summation
 *    order of an output depends on the layer geometry only, never on n.  Channels outside the slice are not written.
 *  - xmc_maxpool3x3s2_valid: nn.max_pool((3, 3), (2, 2), "VALID") of x (n, hi, wi, c) into the channel slice
 *    [y_off, y_off + c) of y (n, (hi - 3) / 2 + 1, (wi - 3) / 2 + 1, ldy); c, ldy, y_off multiples of 8.
 *  - xmc_avgpool3x3_same: tensorflow_style_avg_pooling(x, (3, 3), (1, 1), "SAME") (inception_arch.py:48-67): the sum over
 *    the in-bounds taps divided by their count; x, y (n, h, w, c), c % 8 == 0, x != y.
 *  - xmc_mean_hw: y[i][ch] = mean over the hw pixels of x[i] (n, hw, c) -> float32, summed in pixel order per image. */
typedef struct {
    int32_t n, hi, wi, cin;   /* x rows: (n, hi, wi) pixels of ldx elements, channels [x_off, x_off + cin) */
    int32_t ho, wo, cout;     /* y rows: (n, ho, wo) pixels of ldy elements, channels [y_off, y_off + cout) */
    int32_t kh, kw, stride, pad_t, pad_l;
    int32_t ldx, x_off, ldy, y_off;
    int32_t relu, first, dtype;
} xmc_iconv_desc;
int xmc_inception_conv(const xmc_iconv_desc* d, const void* x, const void* w, const float* bias, void* y, void* stream);
int xmc_maxpool3x3s2_valid(const void* x, void* y, int32_t n, int32_t hi, int32_t wi, int32_t c, int32_t ldy,
                           int32_t y_off, int32_t dtype, void* stream);
int xmc_avgpool3x3_same(const void* x, void* y, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);
int xmc_mean_hw(const void* x, float* y, int32_t n, int32_t hw, int32_t c, int32_t dtype, void* stream);

/* ------------------------------------------------------------------ BERT caption encoder (text in, embeddings out)
 * The reference's preprocess_data.py:36-58 (get_bert_for_captions): bert_en_uncased_L-12_H-768_A-12 on [CLS] .. [SEP] rows of
 * T = max_text_length ids, zero padded.  Everything here is float32; activations are [rows = n * t][h] and ALL t positions of
 * every caption are computed (the reference's sentence embedding sums over the padded positions too, :57, and
 * caption/embedding stores them).  The dense layers are xmc_gemm_f32 / xmc_gemm_f32_bf16mfma on the (out, in) weights; their
 * biases are added by the kernels below that consume the products.  No result depends on which captions share a launch.
 * Pointers are 16-byte aligned; XMC_EINVAL otherwise and for every size outside the stated domain (nothing is launched).
 *
 *  - xmc_bert_embed_ln: y[r] = LayerNorm(word[ids[r]] + pos[r mod t] + type[0]) * gamma + beta, the input of the first layer
 *    (:55, segment ids all zero :53).  word (vocab, h), pos (npos, h) with t <= npos, type (>= 1, h).  The CALLER checks
 *    0 <= ids[r] < vocab on the host before the launch; the kernel clamps an id into the table, so it never reads outside it.
 *  - xmc_bias_residual_ln: y[r] = LayerNorm(x[r] + bias + res[r]) * gamma + beta (the two post-LN sites of a layer).
 *    Both LayerNorms: biased variance as mean((v - mean)^2) over the row held in registers (two passes; with eps = 1e-12 the
 *    one-pass E[v^2] - mean^2 gives variance 0 for a near-constant row), y = (v - mean) / sqrt(var + eps).  h % 4 == 0,
 *    h <= 1024.  y may be x or res.
 *  - xmc_bias_gelu: y = 0.5 v (1 + erf(v / sqrt 2)), v = x + bias[column] -- the exact-erf GELU of TF / HF, evaluated as
 *    0.5 v erfc(-v / sqrt 2) in float64 and rounded once.  x, y (rows, f), f % 4 == 0; y may be x.
 *  - xmc_bert_attention: qkv (n * t, 3 h) = the fused 3h-wide product [q | k | v] WITHOUT its bias, bias_qkv (3 h),
 *    ctx (n * t, h).  Per caption and head (head dimension 64, heads = h / 64):
 *    ctx = softmax_j((q + b_q)(k + b_k)^T / 8)(v + b_v), the softmax over the keys j < max_len[caption] only (in float32
 *    identical to the reference's additive -10000 on the padded keys), for all t query rows, padded ones included.  The
 *    scores stay in LDS.  Domain: 2 <= max_len[i] <= t <= 32, h % 64 == 0.  max_len (DEVICE, int32 [n]) is what the kernel
 *    reads; max_len_host is the caller's HOST copy of the same n values, which this call validates before it launches
 *    (XMC_EINVAL, nothing runs).  The kernel clamps what it reads to [1, t]: a stale device copy cannot index outside a tile.
 *  - xmc_bert_attention_long: the same arguments, semantics and checks for 2 <= max_len[i] <= t <= 64 (64-token captions):
 *    one 256-thread workgroup per (caption, head), the probabilities [t][65] in LDS, float32 throughout.
 *  - xmc_bert_sentence: out[i] = (sum over ALL t rows of emb[i], in row order) / max_len[i] (:56-57; max_len on the device),
 *    emb (n * t, h), out (n, h), h % 4 == 0. */
int xmc_bert_embed_ln(const int32_t* ids, const float* word, const float* pos, const float* type, const float* gamma,
                      const float* beta, float* y, int32_t rows, int32_t t, int32_t h, int32_t vocab, int32_t npos, float eps,
                      void* stream);
int xmc_bias_residual_ln(const float* x, const float* bias, const float* res, const float* gamma, const float* beta, float* y,
                         int32_t rows, int32_t h, float eps, void* stream);
int xmc_bias_gelu(const float* x, const float* bias, float* y, int32_t rows, int32_t f, void* stream);
int xmc_bert_attention(const float* qkv, const float* bias_qkv, const int32_t* max_len, const int32_t* max_len_host, float* ctx,
                       int32_t n, int32_t t, int32_t h, void* stream);
int xmc_bert_attention_long(const float* qkv, const float* bias_qkv, const int32_t* max_len, const int32_t* max_len_host,
                            float* ctx, int32_t n, int32_t t, int32_t h, void* stream);
int xmc_bert_sentence(const float* emb, const int32_t* max_len, float* out, int32_t n, int32_t t, int32_t h, void* stream);

/* ---- running sums of a training step's scalar metrics (the training loop; train_utils.MetricAccumulator) ----
 * `vals` is a HOST array of n (1 <= n <= 8) device pointers to float32 scalars; they are passed to the kernel by value, so
 * the array need not outlive the call.  One launch, one thread: sums[i] += (double)*vals[i] for i = 0 .. n-1 in index order
 * (float64 adds), info[0] += 1, and if any value is NaN or +-inf and info[1] == 0, info[1] = info[0] (the 1-based call that
 * first saw one).  sums: n doubles, info: 2 int32, both device memory the caller zeroes to start a window.  Captured into a
 * hipGraph it accumulates once per replay. */
int xmc_metrics_accum(const float* const* vals, int32_t n, double* sums, int32_t* info, void* stream);

/* ---- in-graph training statistics (config.train_statistics; train_statistics.TrainStatistics; csrc/train_stats.hip, ABI 30) ----
 * xmc_segment_sumsq: x is a flat float32 buffer of n elements, segs a DEVICE table of nseg (offset, length) int64 pairs in
 *   elements; per segment s it writes sumsq[s] = sum of x[i]^2 over the segment (products and adds in float64) and
 *   nonfinite[s] = its number of NaN / +-inf elements (int32, saturating).  Offsets and lengths need no alignment, a length may
 *   be 0, segments may overlap.  Two kernels through the caller's workspace `ws` (xmc_segment_sumsq_ws_bytes of the table, 16-byte
 *   aligned): pieces of 8192 elements summed in a fixed order by one workgroup each, then one wave per segment adds its pieces
 *   in a fixed order.  No atomics: two runs are bit-identical.  segs_host is the caller's HOST copy of the table, which this
 *   call validates before it launches (every segment inside [0, n), the workspace large enough: XMC_EINVAL, nothing runs) and
 *   sizes the grid from; the kernels read the device table and clamp what they read to the buffer.  x is 16-byte aligned.
 * xmc_train_stats: ONE workgroup gathers the XMC_TRAIN_STATS_N float32 scalars of a training step into `vec` --
 *   [3h + 0 / 1 / 2] = loss_vec[h], head_stats[h][0] (accuracy), head_stats[h][1] (entropy) of the five contrastive heads;
 *   [15 .. 18] = mean of the b real logits (logits[0 .. b)), mean of the b generated ones, share of real logits < 1, share of
 *   generated logits > -1; [19 .. 22] = d_grad_scale * sqrt(sum leaf_gsq[0 .. n_d)), g_grad_scale * sqrt(sum leaf_gsq[n_d ..
 *   n_leaves)), sqrt(sum leaf_psq[0 .. n_d)), sqrt(sum leaf_psq[n_d .. n_leaves)); [23], [24] = min and max of scal[2 i] over
 *   the n_sigma {sigma, 1 / (sigma + eps)} pairs (0 when there are none) -- and in the same launch adds vec to the float64
 *   `sums`, adds leaf_gsq * grad_scale^2 / leaf_psq / leaf_bad to the window tables win_gsq / win_psq (float64) / win_bad
 *   (int64), info[0] += 1, and if info[1] == 0 and a leaf_bad entry is non-zero: info[1] = info[0], info[2] = the first such
 *   leaf.  The caller zeroes sums, info (4 int32) and the window tables to start a window.  Plain loads and stores. */
#define XMC_TRAIN_STATS_N 25
typedef struct {
    const float* logits;      /* 2 b float32: D's logits, the real half first */
    const float* scal;        /* 2 n_sigma float32 (may be NULL when n_sigma == 0) */
    const float* loss_vec;    /* 5 float32 */
    const float* head_stats;  /* 5 x 2 float32 */
    const double* leaf_gsq;   /* n_leaves: per-tensor sum of squares of the gradient, D's n_d tensors first */
    const double* leaf_psq;   /* n_leaves: ... of the parameters */
    const int32_t* leaf_bad;  /* n_leaves: non-finite gradient elements */
    float* vec;               /* XMC_TRAIN_STATS_N float32 */
    double* sums;             /* XMC_TRAIN_STATS_N float64 */
    int32_t* info;            /* 4 int32 */
    double* win_gsq;          /* n_leaves */
    double* win_psq;          /* n_leaves */
    int64_t* win_bad;         /* n_leaves */
    int32_t b, n_sigma, n_leaves, n_d;
    float d_grad_scale, g_grad_scale;
} xmc_train_stats_args;
int64_t xmc_segment_sumsq_ws_bytes(const int64_t* segs_host, int32_t nseg);
int xmc_segment_sumsq(const float* x, int64_t n, const int64_t* segs, const int64_t* segs_host, int32_t nseg, double* sumsq,
                      int32_t* nonfinite, void* ws, int64_t ws_bytes, void* stream);
int xmc_train_stats(const xmc_train_stats_args* a, void* stream);

/* ---- device-resident dataset cache (config.device_dataset_cache; libml/device_cache.py; csrc/dataset_cache.hip, ABI 31) ----
 * The cache holds every example once, decoded: img [slots][h][w][3] the resized UNFLIPPED image in [0, 1], emb [slots][s][t][e]
 * the word embeddings of its s captions, sent [slots][s][e] their sentence features, mlen [slots][s] their lengths (all float32,
 * device memory, 64-bit offsets throughout).  xmc_cache_gather builds a batch of n examples from a plan of
 * XMC_CACHE_PLAN_STRIDE int32 per example -- {slot, caption, flip, aug_dy, aug_dx, aug_flip, 0, 0} -- in ONE launch:
 *   image[i, y, x, :]     = img[slot, y, flip ? w-1-x : x, :]
 *   image_aug[i, y, x, :] = image[i, r(y + aug_dy - pad, h), r((aug_flip ? w-1-x : x) + aug_dx - pad, w), :]   (skipped when NULL)
 *                           with r(j, L) = j < 0 ? -j : (j >= L ? 2 (L - 1) - j : j): reflect-pad by `pad`, crop at (aug_dy, aug_dx),
 *                           then the flip (augmentation.augment_shift / augment)
 *   embedding[i] = emb[slot, caption]   sentence[i] = sent[slot, caption]   max_len[i] = mlen[slot, caption]
 * Pure data movement (the outputs are bit copies), one writer per output element, no atomics.  `plan` is the DEVICE copy the
 * kernel reads, `plan_host` the caller's HOST copy, which this call validates before it launches (xmc_cache_plan_check:
 * 0 <= slot < slots, 0 <= caption < s, 0 <= aug_dy, aug_dx <= 2 pad, h > pad, w > pad; XMC_EINVAL and nothing runs otherwise);
 * the kernel clamps what it reads from the device copy to the same ranges.  e % 4 == 0 (caption rows move as 16-byte vectors);
 * every pointer but mlen / max_len / plan is 16-byte aligned; n <= 65535. */
#define XMC_CACHE_PLAN_STRIDE 8
int xmc_cache_plan_check(const int32_t* plan_host, int32_t n, int64_t slots, int32_t s, int32_t h, int32_t w, int32_t pad);
int xmc_cache_gather(const float* img, const float* emb, const float* sent, const float* mlen, int64_t slots, const int32_t* plan,
                     const int32_t* plan_host, float* image, float* image_aug, float* embedding, float* sentence, float* max_len,
                     int32_t n, int32_t h, int32_t w, int32_t s, int32_t t, int32_t e, int32_t pad, void* stream);

/* ---- pairwise sample metrics: KID and improved precision / recall (config.eval_extra_metrics; utils/sample_metrics.py is the
 *      specification; csrc/sample_metrics.hip, ABI 32) ----
 * Pools are row-major float32 [rows][d].  One workgroup owns 128 rows and walks every 128-row tile of the other pool: the dot
 * products run on the exact-fp32 MFMA (one rounding per product, a k-ordered fmaf chain), everything after them is float64 --
 * the squared norms (sums of the float32 squares), d2(a, b) = max(0, |a|^2 + |b|^2 - 2 (double)dot), the comparison with a
 * radius, (dot / d + 1)^3 and every sum.  No n x m matrix is written anywhere; each row's state lives in one thread's registers
 * and is updated in column order; no atomics: two launches on the same inputs give the same bits.
 *   xmc_knn_radii:  radii2[i] = the k-th smallest d2(x_i, x_j) over j != i (exclusion by INDEX: a duplicate row is a neighbour at
 *                   distance 0).  1 <= k <= 8, k < n.
 *   xmc_ball_hits:  hit[i] = 1 when d2(a_i, b_j) <= radii2_b[j] for some j < m, else 0 (n bytes).  A workgroup stops walking once
 *                   all its rows are hit (the result does not depend on it).
 *   xmc_poly3_sums: per subset s < subsets, with X_p = x[xi[s * msub + p]] and Y_q = y[yi[s * msub + q]] (rows gathered through the
 *                   index arrays, no copies; x and y may be the same buffer) and k(u, v) = (u.v / d + 1)^3:
 *                   sums[3 s + 0] = sum over p != q of k(X_p, X_q), [3 s + 1] = the same over Y, [3 s + 2] = sum over all p, q of
 *                   k(X_p, Y_q).  Subsets are the grid's second dimension; every row block leaves a float64 partial in ws and a
 *                   last kernel adds them in block order.  nx, ny: rows of x and y -- the CALLER validates its host copy of the
 *                   indices against them before the launch (ops.py); the kernel clamps what it reads from the device copy.
 * Workspace: xmc_sample_metrics_ws_bytes(n, m, d, subsets) bytes, 16-byte aligned, owned by the caller -- 8 (n + m) for the
 * squared norms of xmc_knn_radii (m = 0) / xmc_ball_hits, and 24 * subsets * ceil(max(n, m) / 128) for the partials of
 * xmc_poly3_sums (n = m = msub), whichever is larger; XMC_EINVAL (negative) outside the domain.
 * Domain: n, m, nx, ny >= 1; d >= 32, d % 32 == 0; 1 <= k <= 8 and k < n; msub >= 2; 1 <= subsets <= 65535; no NULL pointer; every
 * pointer 16-byte aligned.  Anything else returns XMC_EINVAL and launches nothing.  The caller owns every buffer; the calls are
 * asynchronous on `stream`. */
int64_t xmc_sample_metrics_ws_bytes(int32_t n, int32_t m, int32_t d, int32_t subsets);
int xmc_knn_radii(const float* x, int32_t n, int32_t d, int32_t k, double* radii2, void* ws, void* stream);
int xmc_ball_hits(const float* a, int32_t n, const float* b, const double* radii2_b, int32_t m, int32_t d, uint8_t* hit, void* ws,
                  void* stream);
int xmc_poly3_sums(const float* x, int32_t nx, const int32_t* xi, const float* y, int32_t ny, const int32_t* yi, int32_t subsets,
                   int32_t msub, int32_t d, double* sums, void* ws, void* stream);

/* ---- differentiable augmentation of the discriminator's inputs (config.diff_augment; libml/diff_augment.py is the
 *      specification; csrc/diff_augment.hip, ABI 33) ----
 * A plan row is eight float32 {b, s, k, ty, tx, y0, x0, c}: brightness shift, saturation and contrast factors, the integer
 * translation, origin and side of the cutout box (integers as exact floats).  flags: bit 0 brightness, bit 1 saturation, bit 2
 * contrast; translation and cutout are always applied (a zero shift / a side of 0 is the identity).  Per sample, in float32 with
 * one rounding on store:
 *   xmc_diffaug_fwd: u = x + b;  u = (u - mean_c u) s + mean_c u;  u = (u - mu) k + mu with mu = mean_{h,w,c} x + b;
 *                    out[p] = u[p - t] where p - t lies inside the image and p outside [y0, y0 + c) x [x0, x0 + c), else 0.
 *                    real, fake: (b, h, w, 3); out: (2b, h, w, 3), the real half first; plan: (2b, 8), rows 0..b-1 the real half.
 *   xmc_diffaug_bwd: the exact transpose of the linear part on b samples: h[q] = g[q + t] where q + t lies inside the image and
 *                    outside the box, else 0;  h = k h + (1 - k) mean_{h,w,c} h;  dimg = s h + (1 - s) mean_c h.  g != dimg.
 * dtype: XMC_F32 or XMC_BF16, of real / fake / out / g / dimg.  `plan` is the DEVICE copy the kernels read, `plan_host` the caller's
 * HOST copy, validated before anything is launched (every value finite, |ty| < h, |tx| < w, c >= 0; XMC_EINVAL and nothing runs
 * otherwise); the kernels clamp what they read from the device copy and bounds-check every load.  One launch per call, two with
 * bit 2 (a fixed-order reduction of the per-sample mean through `workspace`: xmc_diffaug_workspace_bytes(b, h, w) bytes, 4-byte
 * aligned, may be NULL without bit 2; no atomics).  Rows move as 16-byte vectors when 3 w sizeof(T) is a multiple of 16 and the
 * image pointers are 16-byte aligned, element by element otherwise.  Domain: 1 <= b, 2 b <= 65535, 1 <= h, w <= 16384,
 * 3 h w < 2^31, no NULL pointer. */
int64_t xmc_diffaug_workspace_bytes(int32_t b, int32_t h, int32_t w);
int xmc_diffaug_fwd(const void* real, const void* fake, const float* plan, const float* plan_host, void* out, int32_t b, int32_t h,
                    int32_t w, int32_t flags, int32_t dtype, void* workspace, void* stream);
int xmc_diffaug_bwd(const void* g, const float* plan, const float* plan_host, void* dimg, int32_t b, int32_t h, int32_t w,
                    int32_t flags, int32_t dtype, void* workspace, void* stream);

/* ---- CLIP dual encoder and the text-image alignment scores (config.eval_extra_metrics "clip"; utils/clip_utils.py,
 *      utils/alignment_metrics.py is the specification of the scores and of the preprocessing; csrc/clip.hip, ABI 34) ----
 * The transformers.CLIPModel network: a ViT image tower and a causal text tower of pre-LN blocks (LN, fused q | k | v product,
 * attention, out-projection, residual, LN, fc1, QuickGELU, fc2, residual), LayerNorm eps 1e-5, head dimension 64.  Everything
 * is float32 on activations [rows = n * t][h]; the dense layers are xmc_gemm_f32 / xmc_gemm_f32_bf16mfma on the (out, in)
 * weights and their biases are added by the kernels below.  Cross-lane reductions are fixed xor trees and nothing is
 * accumulated with atomics: two launches on the same inputs give the same bits, and no sequence depends on what shares its
 * launch.  Pointers are 16-byte aligned; XMC_EINVAL otherwise and for every size outside the stated domain (nothing is
 * launched).  LayerNorm rows: h % 4 == 0, h <= 1024, biased variance as mean((v - mean)^2) over the row held in registers.
 *
 *  - xmc_clip_preprocess: images (n, hw, hw, 3), dtype XMC_F32 or XMC_BF16, values in [0, 1] -> the s x s separable Keys cubic
 *    resize (a = -0.5) with Pillow's BICUBIC rule: the support is 2 max(1, hw / s) input pixels around (o + 0.5) hw / s, the
 *    window is clipped to the image and the weights (computed in double, rounded to float32) are normalised per output pixel;
 *    then (v - mean3[c]) / std3[c] (HOST arrays of three floats, std3 > 0).  No uint8 round trip (OpenAI's preprocessing
 *    quantises the resized image to bytes; this one does not).  Output: patches (n * (s / p)^2, 3 p p), row = image, patch row,
 *    patch column, column = (c, ky, kx) -- the flattened patch-embedding weight's order, so the patch convolution is one GEMM.
 *    Domain: 32 <= hw <= 512, p >= 1, s % p == 0, s <= 448.
 *  - xmc_clip_vision_embed: y[i, 0] = LN(cls + pos[0]), y[i, 1 + j] = LN(patch[i, j] + pos[1 + j]) for j < t - 1 (pre_layrnorm);
 *    patch (n * (t - 1), h), pos (t, h), y (n * t, h), t >= 2.
 *  - xmc_clip_text_embed: x[r] = tok[ids[r]] + pos[r mod t]; tok (vocab, h), pos (npos, h), t <= npos.  The CALLER checks
 *    0 <= ids[r] < vocab on the host before the launch; the kernel clamps an id into the table.
 *  - xmc_bias_add_ln: s[r] = x[r] + bias + res[r] and y[r] = LayerNorm(s[r]) * gamma + beta.  bias and res may be NULL (terms
 *    left out: with both NULL this is plain LayerNorm), s may be NULL (not written) or alias res; y may alias x, never s.
 *  - xmc_bias_quick_gelu: y = v sigmoid(1.702 v) = v / (1 + exp(-1.702 v)), v = x + bias[column], evaluated in float64 and
 *    rounded once.  x, y (rows, f), f % 4 == 0; y may be x.
 *  - xmc_mha_attention: qkv (n * t, 3 h) = the fused product [q | k | v] WITHOUT its bias, bias_qkv (3 h), ctx (n * t, h).  Per
 *    sequence and head: ctx = softmax_j((q + b_q)(k + b_k)^T / 8)(v + b_v) over the keys j < len[i], and with causal != 0 also
 *    j <= query row; all t query rows are computed.  One 256-thread workgroup per (sequence, head), k and v rows and the
 *    probabilities [t][t + 1] in LDS (135,680 bytes at t = 128).  Domain: 1 <= len[i] <= t <= 128, h % 64 == 0.  len (DEVICE,
 *    int32 [n]) is what the kernel reads; len_host is the caller's HOST copy, validated before the launch; the kernel clamps
 *    what it reads to [1, t].
 *  - xmc_gather_rows_ln: y[i] = LayerNorm(x[i * t + idx[i]]) * gamma + beta; x (n * t, h), y (n, h).  idx (DEVICE int32 [n]) and
 *    idx_host (its HOST copy, validated: 0 <= idx < t) are both NULL for row 0 of every sequence (the image tower's class row);
 *    with idx = the end-of-text positions this is the text tower's pooled row.  The kernel clamps what it reads.
 *  - xmc_pair_cosine: cos[i] = a[i].b[i] / (|a[i]| |b[i]|) as float64, a, b (n, d): the float32 values multiplied and added in
 *    float64 -- lane l of the row's wave adds elements l, l + 64, .. in index order, then a fixed xor tree.  A zero row gives 0.
 *  - xmc_rprecision_hits: img (n, d), txt (m, d), truth int32 [n], cand int32 [n, c]: hit[i] = 1 iff the cosine of (img[i],
 *    txt[truth[i]]) is STRICTLY greater than that of (img[i], txt[cand[i, j]]) for every j < c, else 0 (n bytes); the arithmetic
 *    of xmc_pair_cosine.  A candidate that duplicates the true caption ties with it and makes the row a miss.  truth / cand are
 *    the DEVICE copies, truth_host / cand_host the HOST copies, validated before the launch (0 <= . < m); the kernel clamps. */
int xmc_clip_preprocess(const void* images, float* patches, int32_t n, int32_t hw, int32_t s, int32_t p, const float* mean3,
                        const float* std3, int32_t dtype, void* stream);
int xmc_clip_vision_embed(const float* patch, const float* cls, const float* pos, const float* gamma, const float* beta, float* y,
                          int32_t n, int32_t t, int32_t h, float eps, void* stream);
int xmc_clip_text_embed(const int32_t* ids, const float* tok, const float* pos, float* x, int32_t rows, int32_t t, int32_t h,
                        int32_t vocab, int32_t npos, void* stream);
int xmc_bias_add_ln(const float* x, const float* bias, const float* res, const float* gamma, const float* beta, float* s, float* y,
                    int32_t rows, int32_t h, float eps, void* stream);
int xmc_bias_quick_gelu(const float* x, const float* bias, float* y, int32_t rows, int32_t f, void* stream);
int xmc_mha_attention(const float* qkv, const float* bias_qkv, const int32_t* len, const int32_t* len_host, float* ctx, int32_t n,
                      int32_t t, int32_t h, int32_t causal, void* stream);
int xmc_gather_rows_ln(const float* x, const int32_t* idx, const int32_t* idx_host, const float* gamma, const float* beta, float* y,
                       int32_t n, int32_t t, int32_t h, float eps, void* stream);
int xmc_pair_cosine(const float* a, const float* b, double* cos, int32_t n, int32_t d, void* stream);
int xmc_rprecision_hits(const float* img, const float* txt, const int32_t* truth, const int32_t* truth_host, const int32_t* cand,
                        const int32_t* cand_host, uint8_t* hit, int32_t n, int32_t m, int32_t d, int32_t c, void* stream);

/* ---- Data gradient of the CLIP image tower (config.clip_guidance_weight; utils/clip_utils.ClipEncoder.image_backward;
 *      utils/clip_grad.py is the specification; csrc/clip_grad.hip, ABI 35) ----
 * The adjoints of the kernels above that the pullback from an image embedding to the pixels crosses.  The weights are frozen:
 * there is no weight gradient, and the dense adjoints dX = dY W run on xmc_gemm_f32 / xmc_gemm_f32_bf16mfma.  float32
 * arithmetic (float64 inside the QuickGELU derivative, as in xmc_bias_quick_gelu), fixed xor trees across lanes, sums in
 * ascending index order, no float atomics: two launches on the same inputs give the same bits.  Pointers are 16-byte aligned;
 * XMC_EINVAL otherwise and for every size outside the stated domain (nothing is launched).
 *
 *  - xmc_mha_attention_bwd: qkv, bias_qkv, len, len_host, n, t, h, causal as xmc_mha_attention; dctx (n * t, h) -> dqkv
 *    (n * t, 3 h), every element written, dqkv != qkv.  The probabilities P are recomputed from qkv with the forward kernel's
 *    arithmetic; dP = dctx V^T, dS = P o (dP - rowsum(P o dP)) / 8, dQ = dS K, dK = dS^T Q, dV = P^T dctx.  Masked keys
 *    contribute exactly 0.  One 256-thread workgroup per (sequence, head); k and v rows, 32 query rows of q and dctx and their
 *    P and dS rows in LDS (120,064 bytes at t = 128).  Domain: 1 <= len[i] <= t <= 128, h % 64 == 0.
 *  - xmc_ln_bwd_add: with y = LayerNorm(x) * gamma + beta and g = dy gamma: dx = rstd (g - mean(g) - xhat mean(g xhat)) + dres,
 *    mean and biased variance of the row in two passes as the forward kernels.  dres may be NULL or alias dx; dx aliases neither
 *    x nor dy.  h % 4 == 0, h <= 1024.  mode selects the forward kernel's row map:
 *      XMC_LN_BWD_ROWS   (xmc_bias_add_ln)     x, dy, dres, dx (rows, h); pos NULL, t = 1.
 *      XMC_LN_BWD_GATHER (xmc_gather_rows_ln on row 0) x, dres, dx (rows = n t, h), dy (n, h): row i t of dx takes the gradient
 *                        of pooled row i, every other row 0 (+ dres); pos NULL.
 *      XMC_LN_BWD_VISION (xmc_clip_vision_embed) x = the patch products (rows = n (t - 1), h), pos (t, h), dy (n t, h) -> dx
 *                        (rows, h): row (i, j - 1) = LN-backward(x[i, j - 1] + pos[j], dy[i t + j]); the class row's gradient
 *                        is dropped.  dres NULL, t >= 2.
 *  - xmc_bias_quick_gelu_bwd: dv = dy (s + 1.702 v s (1 - s)), v = x + bias[column], s = 1 / (1 + exp(-1.702 v)); x is the
 *    product WITHOUT its bias (what xmc_bias_quick_gelu read).  x, dy, dv (rows, f), f % 4 == 0; dv may be dy, never x.
 *  - xmc_clip_preprocess_bwd: the exact transpose of xmc_clip_preprocess: dpatches (n (s / p)^2, 3 p p) -> dimages
 *    (n, hw, hw, 3) float32 or bf16 (dtype), dX_c = Ry^T dY_c Rx / std3[c] with the same float32 taps.  Gather form: every
 *    input pixel adds the output pixels whose window holds it, in ascending order, first along y, then along x.  One workgroup
 *    per (image, input row).  Domain as xmc_clip_preprocess. */
#define XMC_LN_BWD_ROWS 0
#define XMC_LN_BWD_GATHER 1
#define XMC_LN_BWD_VISION 2
int xmc_mha_attention_bwd(const float* qkv, const float* bias_qkv, const int32_t* len, const int32_t* len_host, const float* dctx,
                          float* dqkv, int32_t n, int32_t t, int32_t h, int32_t causal, void* stream);
int xmc_ln_bwd_add(const float* x, const float* pos, const float* gamma, const float* dy, const float* dres, float* dx, int32_t rows,
                   int32_t t, int32_t h, float eps, int32_t mode, void* stream);
int xmc_bias_quick_gelu_bwd(const float* x, const float* bias, const float* dy, float* dv, int32_t rows, int32_t f, void* stream);
int xmc_clip_preprocess_bwd(const float* dpatches, void* dimages, int32_t n, int32_t hw, int32_t s, int32_t p, const float* std3,
                            int32_t dtype, void* stream);

/* ---- skipping optimiser updates with non-finite gradients (config.skip_nonfinite_updates; libml/nonfinite_guard.py;
 *      csrc/nonfinite_guard.hip and the GUARD instantiations of the optimiser kernels, ABI 36) ----
 * A half step of training becomes a transaction: one verdict, taken on the device after its backward passes, decides whether
 * ALL of its state changes are applied or none.
 *  - xmc_nonfinite_verdict scans nseg (1 .. XMC_NONFINITE_MAX_SEGMENTS) float32 segments: `ptrs` is a HOST array of nseg device
 *    pointers, `n_host` a HOST array of their element counts (both passed to the kernel by value; a count may be 0, and then the
 *    pointer is not read; every other pointer is 16-byte aligned, XMC_EINVAL otherwise).  An element is bad when its exponent bits
 *    are all ones (NaN, +inf, -inf; denormals and 0x7f7fffff are fine).  Two launches, no atomics: chunks of 8192 elements are
 *    dealt round-robin to at most 1024 workgroups, each of which writes one (count, first segment) pair into the workspace `ws`
 *    (xmc_nonfinite_verdict_workspace_bytes of the same n_host, 16-byte aligned); one workgroup adds the pairs and writes
 *        verdict[0] = 1 if any element was bad, else 0;   verdict[1] = the number of bad elements (saturating);
 *        verdict[2] = the index of the first segment that held one, or -1;   verdict[3] = 0
 *    and updates the persistent counters[4] (the caller zeroes them once):
 *        [0] += 1 on a bad verdict (half steps skipped in total);   [1] = the current run of consecutive bad verdicts (0 after a
 *        clean one);   [2] = max([2], [1]) (the longest run since the caller last zeroed it);   [3] is not touched.
 *  - xmc_commit_if: dst[i] = src[i] for i < n unless verdict[0] != 0 (16-byte copies when both pointers allow).
 *  - xmc_adam_ema_dev_guarded / xmc_adam_ema_dev_sn_guarded / xmc_adam_wprep_tiles_guarded: the entry point of the same name with
 *    `verdict` in front of `stream`.  verdict[0] == 0: the same arithmetic, bit for bit.  verdict[0] != 0: p, m, v, ema,
 *    step_state (Adam's t does not advance) and the prepared copies / partial rows are left as they are; the gradient is still
 *    overwritten with zeros where zero_grads == 1 would do so (zero_grads == 2 and 0 then write nothing).
 *  - xmc_metrics_accum_if: xmc_metrics_accum unless verdict[0] != 0 (nothing is added, the call is not counted). */
#define XMC_NONFINITE_MAX_SEGMENTS 8
int64_t xmc_nonfinite_verdict_workspace_bytes(const int64_t* n_host, int32_t nseg);
int xmc_nonfinite_verdict(const float* const* ptrs, const int64_t* n_host, int32_t nseg, int32_t* verdict, int32_t* counters,
                          void* ws, int64_t ws_bytes, void* stream);
int xmc_commit_if(float* dst, const float* src, int64_t n, const int32_t* verdict, void* stream);
int xmc_adam_ema_dev_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, double beta1,
                             double beta2, float eps, float* step_state, float grad_scale, float ema_decay,
                             const int32_t* verdict, void* stream);
int xmc_adam_ema_dev_sn_guarded(float* p, float* g, float* m, float* v, float* ema, int64_t n, float lr, double beta1,
                                double beta2, float eps, float* step_state, float grad_scale, float ema_decay,
                                int32_t zero_grads, const void* map, const void* table, int32_t n_entries,
                                const float* kvec, const float* scal, const float* u, const float* vv,
                                const int32_t* verdict, void* stream);
int xmc_adam_wprep_tiles_guarded(const void* table, int32_t n, int32_t blocks, float* p, float* g, float* m, float* v, float* ema,
                                 float lr, double beta1, double beta2, float eps, const float* step_state, float grad_scale,
                                 float ema_decay, int32_t zero_grads, const float* kvec, const float* scal, const float* u,
                                 const float* vv, void* wf_buf, void* wd_buf, void* pf_buf, void* pd_buf, float* part,
                                 const int32_t* verdict, void* stream);
int xmc_metrics_accum_if(const float* const* vals, int32_t n, double* sums, int32_t* info, const int32_t* verdict, void* stream);

/* ---- adaptive discriminator augmentation (config.ada_target; libml/ada.py is the specification; csrc/ada.hip) ----
 * XMC_ABI_VERSION stays 36: this section only ADDS entry points, no existing signature or structure changes, and a library built
 * before it fails loudly at symbol resolution when it is loaded (every declared symbol must resolve).
 * `state` is the controller's persistent float64[8] in device memory, 8-byte aligned (the caller zeroes it once):
 *     [0] p   [1] sign_sum   [2] count   [3] ticks   [4] last_r   [5] adjustments   [6], [7] not touched
 *  - xmc_ada_gate: rows[2b][8] from plan[b][2][8] and the uniforms u[b][2][5] (index 1: real / generated), real rows first (the
 *    layout xmc_diffaug_fwd reads).  Part g (brightness, saturation, contrast, translation, cutout: columns {0}, {1}, {2}, {3, 4},
 *    {5, 6, 7}) of a row keeps the plan's values iff (double)u < state[0], read on the device; otherwise its columns take the
 *    identity values (0, 1, 1, 0, 0, 0, 0, 0).  One thread per row, two 16-byte stores, one writer per element.
 *    Domain: 1 <= b, 2 b <= 65535; plan and rows 16-byte aligned, u 4-byte aligned.
 *  - xmc_ada_update: one half step of the controller over logit[0 .. b), the REAL half of D's float32 logit vector (nothing
 *    behind it is read).  Over the finite logits: sign_sum += #(x > 0) - #(x < 0), count += #finite (+-0 has sign 0); ticks += 1.
 *    When ticks >= interval: if count > 0, in IEEE double and in this order, r = sign_sum / count, sgn = (r > target) - (r < target),
 *    p = min(max(p + sgn * (count / images_to_full), 0), p_max), last_r = r, adjustments += 1; in every case sign_sum = count =
 *    ticks = 0.  One workgroup, no atomics: the counts are integers, so the result is bit-equal to the specification.
 *    Domain: 1 <= b, 1 <= interval, images_to_full > 0, p_max >= 0, target not NaN.
 * Anything else returns XMC_EINVAL and launches nothing. */
int xmc_ada_gate(const float* plan, const float* u, const double* state, float* rows, int32_t b, void* stream);
int xmc_ada_update(const float* logit, int32_t b, double* state, double target, double images_to_full, int32_t interval,
                   double p_max, void* stream);

/* ---- LeCam discriminator regulariser (config.lecam_weight; libml/lecam.py is the specification; csrc/lecam.hip) ----
 * XMC_ABI_VERSION stays 36: this section only ADDS an entry point, as the section above did.
 * `state` is the regulariser's persistent float64[8] in device memory, 8-byte aligned (the caller zeroes it once):
 *     [0] anchor_real   [1] anchor_fake   [2] ticks (half steps seen)   [3] last R   [4] updates (anchor updates applied)
 *     [5] .. [7] not touched
 *  - xmc_lecam: one half step over logit[0 .. 2b) = D's float32 logits [real; fake] and dld[0 .. 2b), the gradient xmc_hinge has
 *    just written.  In IEEE double, in this order, no multiply fused with an add; S is the fixed-order sum "lane j of 256 adds
 *    elements j, j + 256, ... in rising order onto +0, then the tree v[j] += v[j + s] for s = 128 ... 1":
 *      1. active = ticks >= start and updates > 0.
 *      2. if active: dr_i = real_i - anchor_fake, df_i = fake_i - anchor_real (one_sided: dr_i = dr_i > 0 ? dr_i : 0 and
 *         df_i = df_i < 0 ? df_i : 0);  R = (S(dr^2) + S(df^2)) / b;  c = (2 lam) / b;  dld_i = float32(double(dld_i) + c d_i), one
 *         rounding per element.  Otherwise R = 0 and dld is not written.  last R = R, loss[0] = float32(R): the UNWEIGHTED value,
 *         written, not added.  A NaN that is written (an element of dld, R) is the canonical quiet NaN (sign 0, payload 0).
 *      3. if all 2b logits are finite: m_R = S(real) / b, m_F = S(fake) / b;  g = active ? decay : 0;  anchor = g * anchor +
 *         (1 - g) * m for both anchors, from the values read in 1 (two multiplies and an add, each rounded);  updates += 1.
 *      4. ticks += 1.
 *    One workgroup of 256, no atomics: bit-equal to the specification.  Writes dld[0 .. 2b), loss[0], state[0 .. 5), nothing else.
 *    Domain: 1 <= b, 2 b <= 2147483647; lam finite and >= 0; 0 <= decay < 1; start >= 0; one_sided 0 or 1; logit, dld and loss
 *    4-byte aligned.  Anything else returns XMC_EINVAL and launches nothing. */
int xmc_lecam(const float* logit, float* dld, int32_t b, double* state, float* loss, double lam, double decay, int32_t start,
              int32_t one_sided, void* stream);

/* ---- the three controllers with data-parallel replicas (dp.GradSync(schedule="exclusive").gather_rows; the specifications are
 *      libml/ada.update_rows, libml/lecam.step_rows and libml/nonfinite_guard.merge_rows) ----
 * XMC_ABI_VERSION stays 36: this section only ADDS entry points, as the two sections above did.
 * Each rank contributes one small row, the rows are all-gathered in rank order, and every rank runs the same single-workgroup
 * kernel over the same rows[w][...]: the same bits everywhere, whatever the backend of the exchange.  No atomics, plain vector
 * stores, no host read.  `state`, `verdict` and `counters` are the buffers of the sections above.
 *  - xmc_ada_update_rows: rows[w][2b] are the ranks' float32 logit vectors [real; fake]; xmc_ada_update over the concatenation of
 *    the real halves rows[r][0 .. b), r = 0 .. w - 1 (the generated halves are not read): the same integer counts, then the same
 *    IEEE double tail.  images_to_full counts GLOBAL images.  w = 1: bit-equal to xmc_ada_update.  Writes state[0 .. 6), nothing else.
 *    Domain: 1 <= w, 1 <= b, w * 2 b <= 2147483647, 1 <= interval, images_to_full > 0, p_max >= 0, target not NaN; rows 4-byte
 *    and state 8-byte aligned.
 *  - xmc_lecam_rows: steps 1 - 4 of xmc_lecam with X_R / X_F = the concatenation, in rank order, of the real halves
 *    rows[r][0 .. b) / the generated halves rows[r][b .. 2b) (w b elements each; S runs over them in that order):
 *    R = (S(dr^2) + S(df^2)) / (w b), m_R = S(X_R) / (w b), m_F = S(X_F) / (w b), and "all finite" is tested over all w * 2 b logits
 *    -- so loss[0] and state are identical on every rank.  dld[0 .. 2b) is THIS rank's gradient: dld_i = float32(double(dld_i) +
 *    c d_i) with c = (2 lam) / b, the LOCAL b, and d_i from row `rank` (the optimiser's 1 / w gradient scale makes the sum over the
 *    ranks the gradient of lam R).  The same canonical quiet NaN; no multiply fused with an add.  w = 1: bit-equal to xmc_lecam.
 *    Writes dld[0 .. 2b), loss[0], state[0 .. 5), nothing else.
 *    Domain: 1 <= w, 0 <= rank < w, 1 <= b, w * 2 b <= 2147483647; lam finite and >= 0; 0 <= decay < 1; start >= 0; one_sided 0 or
 *    1; rows, dld and loss 4-byte, state 8-byte aligned.
 *  - xmc_verdict_merge: rows[w][4] are the ranks' LOCAL verdicts (xmc_nonfinite_verdict into a local row and scratch counters).
 *    With r* = the lowest r whose rows[r][0] != 0:
 *        verdict[0] = 1 if there is an r*, else 0;   verdict[1] = min(sum of rows[r][1] in int64, 2147483647);
 *        verdict[2] = rows[r*][2], or -1;   verdict[3] = r*, or 0
 *    and the persistent counters[4] advance from the merged verdict[0] by the rule of xmc_nonfinite_verdict.  w = 1 reproduces
 *    the local verdict.  Writes verdict[0 .. 4) and counters[0 .. 3), nothing else.
 *    Domain: 1 <= w, 4 w <= 2147483647; all three pointers 4-byte aligned.
 * Anything else returns XMC_EINVAL and launches nothing. */
int xmc_ada_update_rows(const float* rows, int32_t w, int32_t b, double* state, double target, double images_to_full,
                        int32_t interval, double p_max, void* stream);
int xmc_lecam_rows(const float* rows, int32_t w, int32_t rank, float* dld, int32_t b, double* state, float* loss, double lam,
                   double decay, int32_t start, int32_t one_sided, void* stream);
int xmc_verdict_merge(const int32_t* rows, int32_t w, int32_t* verdict, int32_t* counters, void* stream);

/* ---- learning-rate and EMA-decay schedules evaluated on the device (config.lr_schedule, config.ema_ramp, ...;
 *      libml/opt_schedule.py is the specification; csrc/pointwise.hip, csrc/spectral_batched.hip) ----
 * XMC_ABI_VERSION stays 36: this section only ADDS entry points and a structure, as the sections above did.
 * `step_state` is float32[8] here: [0] t (int32 bits)  [1] 1 / (1 - beta1^t)  [2] 1 / (1 - beta2^t)  [3] not touched
 *     [4] lr_t   [5] d_t (the EMA decay of this update)   [6] float32(w f), the rate's factor   [7] not touched
 * The entry points above read and write slots 0 .. 2 only; they never touch 4 .. 7.
 * For the update that makes the counter t (t >= 1), in IEEE double, in this order, no multiply fused with an add:
 *     w = t / warmup if warmup > 0 and t < warmup, else 1
 *     x = 0 if t <= decay_start;  1 if t >= decay_end;  otherwise (t - decay_start) / (decay_end - decay_start)
 *     f = 1 (CONSTANT);  1 + (final_ratio - 1) x (LINEAR);  final_ratio + (1 - final_ratio) (0.5 (1 + cos(pi x))) (COSINE)
 *     lr_t = float32((base w) f);   slot 6 = float32(w f)
 *     d_t = 0 if t <= ema_start;  else float32(min(ema_decay, (1 + t) / (ema_ramp + t))) if ema_ramp > 0;  else float32(ema_decay)
 * A CONSTANT schedule without warm-up yields exactly the float32 the host arguments `lr` / `ema_decay` of the parents yield.
 *  - xmc_adam_ema_dev_sched / xmc_adam_ema_dev_sn_sched: the entry point of the same name without its `lr` and `ema_decay`; ONE
 *    thread advances t and the two corrections exactly as the parent does and writes slots 4 .. 6 from `sched` (read on the host
 *    at launch: it travels in the kernel arguments); the Adam kernel behind it is the parent's, with lr and d taken from slots 4
 *    and 5 -- the same arithmetic on the same values, bit for bit.  `verdict` may be NULL (the unguarded form); otherwise it is
 *    the int32[4] of xmc_nonfinite_verdict, and verdict[0] != 0 leaves p, m, v, ema and ALL of step_state as they are and zeroes the
 *    gradient where the parent's guarded form would.
 *  - xmc_adam_wprep_tiles_sched: xmc_adam_wprep_tiles(_guarded) without `lr` and `ema_decay`, on a step_state that
 *    xmc_adam_ema_dev_sn_sched has ALREADY advanced for this update; `verdict` may be NULL.
 * XMC_EINVAL, nothing launched: whatever the parent refuses; sched NULL; an unknown kind; reserved != 0; base not finite or <= 0; a negative warmup,
 * decay_start, decay_end or ema_start; decay_end <= decay_start on a decaying kind; final_ratio outside [0, 1] or not finite;
 * ema_decay outside [0, 1); ema_ramp negative or not finite; a verdict that is not 4-byte aligned. */
#define XMC_SCHED_CONSTANT 0
#define XMC_SCHED_LINEAR 1
#define XMC_SCHED_COSINE 2
typedef struct xmc_opt_schedule {
    int32_t kind;                /* XMC_SCHED_* */
    int32_t reserved;            /* 0 */
    double base;                 /* the base learning rate */
    int64_t warmup;              /* W: the horizons count updates of THIS optimiser */
    int64_t decay_start;         /* T0 */
    int64_t decay_end;           /* T1 (read by the decaying kinds only) */
    double final_ratio;          /* r */
    double ema_decay;
    double ema_ramp;
    int64_t ema_start;           /* S */
} xmc_opt_schedule;
int xmc_adam_ema_dev_sched(float* p, const float* g, float* m, float* v, float* ema, int64_t n, double beta1, double beta2,
                           float eps, float* step_state, float grad_scale, const xmc_opt_schedule* sched, const int32_t* verdict,
                           void* stream);
int xmc_adam_ema_dev_sn_sched(float* p, float* g, float* m, float* v, float* ema, int64_t n, double beta1, double beta2, float eps,
                              float* step_state, float grad_scale, int32_t zero_grads, const void* map, const void* table,
                              int32_t n_entries, const float* kvec, const float* scal, const float* u, const float* vv,
                              const xmc_opt_schedule* sched, const int32_t* verdict, void* stream);
int xmc_adam_wprep_tiles_sched(const void* table, int32_t n, int32_t blocks, float* p, float* g, float* m, float* v, float* ema,
                               double beta1, double beta2, float eps, const float* step_state, float grad_scale,
                               int32_t zero_grads, const float* kvec, const float* scal, const float* u, const float* vv,
                               void* wf_buf, void* wd_buf, void* pf_buf, void* pd_buf, float* part, const int32_t* verdict,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XMCGAN_HIP_H_ */
