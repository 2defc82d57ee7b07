/* Image codec kernels of the MI355X build: the pixel half of a JPEG decode and the PNG scanline filter, for the dataset
 * builder (xmcgan_image_generation_amd/preprocess_data.py).  NOT part of the product ABI (include/xmcgan_hip.h,
 * libxmcgan_hip.so): built into a separate libxmc_codec.so (csrc_codec/), never needed by a training step.  Same conventions
 * as the product ABI: caller-owned buffers, a *_workspace_bytes function per call, an explicit stream, 0 / negative
 * errno-style return codes (-22 invalid argument, <= -1000: HIP error 1000 + code), no environment variables, no atomics.
 *
 * Both calls work on a BATCH of images of different sizes, described by one table of XMC_CODEC_DESC_WORDS int64 per image in
 * HOST memory (the calls validate every row against the arena sizes before anything is launched, and copy the table into
 * the front of their workspace on the stream).  LIFETIME: that copy is a hipMemcpyAsync from the caller's memory, ordered on
 * `stream`; the table must stay allocated and unchanged until the stream has passed it -- synchronise the stream, or wait on an
 * event recorded after the call, before freeing or rewriting it.  The rows:
 *   [0] coef_off   first int16 of the image in the coefficient arena, a multiple of 8; the component planes follow each
 *                  other, each [block_row][block_col][64] in natural order, padded to whole MCUs (xmc_jpeg_coefficients)
 *   [1] qt_off     first uint16 of the image's [ncomp][64] quantisation tables (natural order), a multiple of 8
 *   [2] plane_off  byte offset of the image's clamped component planes in the decode workspace (after the table), a
 *                  multiple of 8; they take xmc_jpeg_plane_bytes() bytes
 *   [3] out_off    byte offset of the image's tightly packed uint8 (height, width, 3) pixels in the pixel arena, a
 *                  multiple of 4
 *   [4] width  [5] height  (1 .. 16384, width * height <= 2^26)
 *   [6] ncomp      1 (grey, written to all three channels) or 3 (YCbCr)
 *   [7] hs  [8] vs luma sampling: 1x1, 2x1 or 2x2 (chroma is 1x1); 1x1 for grey
 *   [9] filt_off   byte offset of the image's filtered scanlines (height * (1 + 3 * width) bytes) in the stream arena, a
 *                  multiple of 4                                                     (xmc_png_filter_batch only)
 *   [10] row_off   index of the image's first row among the rows of the batch      (xmc_png_filter_batch only)
 *   [11..15]       0
 */
#ifndef XMC_CODEC_H_
#define XMC_CODEC_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XMC_CODEC_ABI_VERSION 1
#define XMC_CODEC_DESC_WORDS 16
#define XMC_CODEC_MAX_BATCH 65535
#define XMC_CODEC_MAX_SIDE 16384
#define XMC_CODEC_MAX_PIXELS (1 << 26)
/* dequantised coefficients are clamped to +-XMC_JPEG_DEQUANT_CLAMP and the row pass of the inverse DCT (four fraction bits)
 * to +-XMC_JPEG_PASS1_CLAMP: with them no int16 coefficient and no table entry up to 65535 can overflow the kernel's int32
 * arithmetic (the derivation is in libml/jpeg.py, the specification) */
#define XMC_JPEG_DEQUANT_CLAMP 8191
#define XMC_JPEG_PASS1_CLAMP 65535

int xmc_codec_abi_version(void);

/* bytes of the clamped component planes of one image (a multiple of 64), or -22 */
int64_t xmc_jpeg_plane_bytes(int32_t width, int32_t height, int32_t ncomp, int32_t hs, int32_t vs);
/* workspace of xmc_jpeg_decode_batch for this table: the table itself plus the farthest plane end; or -22 */
int64_t xmc_jpeg_decode_workspace_bytes(const int64_t* desc, int32_t n);
/* Quantised coefficients + tables -> RGB pixels, bit-equal to libml/jpeg.py: decode_coefficients_np.  Two launches over the
 * whole batch: dequantise + 8x8 inverse DCT into the planes, then chroma upsampling + YCbCr -> RGB.  coef / qt / out: device
 * pointers, ws: device, 16-byte aligned.  desc: HOST. */
int xmc_jpeg_decode_batch(const int16_t* coef, int64_t coef_elems, const uint16_t* qt, int64_t qt_elems, const int64_t* desc,
                          int32_t n, uint8_t* out, int64_t out_bytes, void* ws, int64_t ws_bytes, void* stream);

/* workspace of xmc_png_filter_batch: the table plus one int32 per image row; or -22 */
int64_t xmc_png_filter_workspace_bytes(const int64_t* desc, int32_t n);
/* Per image of the pixel arena (rows [3] [4] [5] [9] [10] of the table), per row: the PNG filter (0 None, 1 Sub, 2 Up, 3
 * Average, 4 Paeth) whose filtered bytes, read as signed, have the smallest sum of absolute values, ties to the lowest id;
 * writes the filter byte and the filtered row -- the stream zlib takes.  Bit-equal to libml/png.py: filter_rows_np.  Two
 * launches: choose per row, then write.  px / out: device, ws: device, 16-byte aligned.  desc: HOST. */
int xmc_png_filter_batch(const uint8_t* px, int64_t px_bytes, const int64_t* desc, int32_t n, uint8_t* out, int64_t out_bytes,
                         void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XMC_CODEC_H_ */
