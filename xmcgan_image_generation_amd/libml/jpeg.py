"""JPEG decoding in two halves, the way hardware decoders split it.

* ``info`` / ``coefficients``: the serial entropy decoder on the host (``csrc_host/xmc_jpeg.c``) -- JPEG bytes -> QUANTISED
  coefficients (int16, natural order, ``[block_row][block_col][64]`` per component, padded to whole MCUs) and the
  quantisation tables.  8-bit Huffman baseline, extended sequential and progressive; grey or YCbCr; luma sampling 1x1, 2x1,
  2x2 with 1x1 chroma.  Everything else is refused with its own code (``JpegError.code``).
* ``decode_coefficients_np``: the SPECIFICATION of the pixel half (``csrc_codec/jpeg.hip``: ``xmc_jpeg_decode_batch``) and the
  host fallback when no GPU is present.  Integer arithmetic only, evaluated in int64, so the kernel's int32 arithmetic is held
  to it bit for bit.

The pixel half, stated once (the kernel and this module follow it to the bit):

1. dequantise: ``d = clamp(c * q, -DEQUANT_CLAMP, DEQUANT_CLAMP)``;
2. inverse DCT, separable, as two 8 x 8 integer matrix products with ``IDCT_MATRIX[x][u] = round(2^13 * c(u)/2 *
   cos((2x + 1) u pi / 16))``, ``c(0) = 1/sqrt(2)``: rows first (along u, the 8 values of one stored row), ``t = clamp((sum +
   2^8) >> 9, -PASS1_CLAMP, PASS1_CLAMP)`` (four fraction bits kept), then columns, ``s = (sum + 2^16) >> 17``; the sample is
   ``clamp(s + 128, 0, 255)``; every shift is arithmetic (floor), so the rounding is half up;
3. chroma upsampling, centred linear ("fancy"): per subsampled axis the nearer sample weighs 3/4 and the farther 1/4, an axis
   that is not subsampled weighs 4/4 and 0; ``v = (wx0 * wy0 * A + wx1 * wy0 * B + wx0 * wy1 * C + wx1 * wy1 * D + 8) >> 4``
   with the weights in quarters; neighbours outside the component's ceil(W / h) x ceil(H / v) samples are the edge sample;
4. YCbCr -> RGB, JFIF, 16 fraction bits, ``cb = Cb - 128``, ``cr = Cr - 128``: ``R = Y + ((91881 * cr + 32768) >> 16)``,
   ``G = Y + ((-22553 * cb - 46802 * cr + 32768) >> 16)``, ``B = Y + ((116130 * cb + 32768) >> 16)``, clamped to [0, 255];
5. a grey image writes Y to all three channels.

Why the two clamps keep int32 safe for ANY int16 coefficient and any table entry up to 65535.  Every row of absolute values of
``IDCT_MATRIX`` sums to ``IDCT_ROW_ABS_MAX`` = 21641 (computed below, asserted at import).  First pass, with ``DEQUANT_CLAMP``
= 8191: |sum| <= 21641 * 8191 + 2^8 = 177,261,687 < 2^31.  Second pass, with ``PASS1_CLAMP`` = 65535: |sum| <= 21641 * 65535 +
2^16 = 1,418,308,471 < 2^31 - 1 = 2,147,483,647.  The product c * q itself needs no care: |c| <= 32768 and q <= 65535 give at
most 32768 * 65535 = 2^31 - 32768, inside int32.  Neither clamp touches a file an encoder made: an 8-bit JPEG's true coefficients stay
within about +-1024 * 1.3 plus half a quantisation step (the clamp is four to six times that), and the row pass of samples
within +-300 stays below 2.83 * 300 = 850 (``PASS1_CLAMP`` is 4095.9 in sample units).  Four fraction bits between the passes
are what IEEE 1180-1990 needs here: with two, the overall mean square error on the [-5, 5] blocks is 0.038 against the 0.02
allowed; with four it is 0.009 (tests/test_jpeg.py).  Upsampling: <= 16 * 255 + 8; colour: <= 116130 * 128 + 32768 < 2^24.
"""
from __future__ import annotations

import math

import numpy as np

from . import _io

INFO_WORDS = 16
MAX_SIDE, MAX_PIXELS = 16384, 1 << 26

E_MALFORMED, E_TRUNCATED, E_HUFFMAN, E_RUN, E_RESTART, E_TABLE, E_BUFFER, E_RANGE, E_SCANS = -1, -2, -3, -4, -5, -6, -7, -8, -9
E_ARITHMETIC, E_PRECISION, E_PROCESS, E_COMPONENTS, E_SAMPLING, E_SIZE = -10, -11, -12, -13, -14, -15
UNSUPPORTED = (E_ARITHMETIC, E_PRECISION, E_PROCESS, E_COMPONENTS, E_SAMPLING, E_SIZE)
_MESSAGES = {
    E_MALFORMED: "not a JPEG, or a malformed marker segment", E_TRUNCATED: "truncated stream",
    E_HUFFMAN: "invalid Huffman code, or a scan that runs into a marker", E_RUN: "zero run past the end of the block",
    E_RESTART: "missing or wrong restart marker", E_TABLE: "table index out of range or table not defined",
    E_BUFFER: "buffer too small", E_RANGE: "coefficient out of the int16 range", E_SCANS: "more than 256 scans",
    E_ARITHMETIC: "arithmetic coding is not supported", E_PRECISION: "only 8-bit samples are supported",
    E_PROCESS: "lossless and hierarchical processes are not supported",
    E_COMPONENTS: "only 1 (grey) or 3 (YCbCr) components are supported (CMYK / YCCK refused)",
    E_SAMPLING: "only luma sampling 1x1, 2x1, 2x2 with 1x1 chroma is supported",
    E_SIZE: f"larger than the decoder's cap ({MAX_SIDE} per side, {MAX_PIXELS} pixels)"}


class JpegError(ValueError):
    def __init__(self, code: int):
        self.code = code
        super().__init__(f"JPEG: {_MESSAGES.get(code, 'error')} ({code})")

    @property
    def unsupported(self) -> bool:
        """a well-formed file of a kind this decoder refuses (as opposed to damaged data)"""
        return self.code in UNSUPPORTED


class Info:
    """frame header of one file.  ``planes``: per component (block rows, block columns) of the padded coefficient plane"""
    __slots__ = ("width", "height", "ncomp", "process", "hs", "vs", "mcus_x", "mcus_y", "coef_bytes", "qt_bytes")

    def __init__(self, words):
        (self.width, self.height, self.ncomp, self.process, self.hs, self.vs, self.mcus_x, self.mcus_y, self.coef_bytes,
         self.qt_bytes) = (int(x) for x in words[:10])

    @property
    def planes(self):
        return plane_blocks(self.ncomp, self.hs, self.vs, self.mcus_x, self.mcus_y)


def plane_blocks(ncomp, hs, vs, mcus_x, mcus_y):
    return [(mcus_y * vs, mcus_x * hs)] + [(mcus_y, mcus_x)] * (ncomp - 1)


def info(data) -> Info:
    a, p = _io._buf(data)
    words = np.zeros(INFO_WORDS, np.int32)
    rc = _io.load().xmc_jpeg_info(p, a.size, words.ctypes.data)
    if rc != 0:
        raise JpegError(rc)
    return Info(words)


def coefficients_into(data, coef: np.ndarray, qt: np.ndarray) -> int:
    """entropy-decode into caller-owned int16 / uint16 buffers (views of a shared arena); -> the return code, no exception"""
    a, p = _io._buf(data)
    return int(_io.load().xmc_jpeg_coefficients(p, a.size, coef.ctypes.data, coef.nbytes, qt.ctypes.data, qt.nbytes))


def coefficients(data):
    """-> (Info, coefficients int16 flat (the planes one after the other), tables uint16 (ncomp, 64) in natural order)"""
    nfo = info(data)
    coef = np.empty(nfo.coef_bytes // 2, np.int16)
    qt = np.empty((nfo.ncomp, 64), np.uint16)
    rc = coefficients_into(data, coef, qt)
    if rc != 0:
        raise JpegError(rc)
    return nfo, coef, qt


# ------------------------------------------------------------------------------------------------- the specification
DEQUANT_CLAMP = 8191
PASS1_CLAMP = 65535
IDCT_BITS, PASS1_SHIFT, PASS2_SHIFT = 13, 9, 17
IDCT_MATRIX = np.array([[round((1 << IDCT_BITS) * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16))
                         for u in range(8)] for x in range(8)], np.int64)
IDCT_ROW_ABS_MAX = int(np.abs(IDCT_MATRIX).sum(axis=1).max())
assert IDCT_ROW_ABS_MAX == 21641 and IDCT_ROW_ABS_MAX * DEQUANT_CLAMP + (1 << (PASS1_SHIFT - 1)) < 2 ** 31
assert IDCT_ROW_ABS_MAX * PASS1_CLAMP + (1 << (PASS2_SHIFT - 1)) < 2 ** 31
CR_R, CB_G, CR_G, CB_B = 91881, 22553, 46802, 116130          # round(2^16 * (1.402, 0.344136, 0.714136, 1.772))


def idct_signed_np(coef, qt) -> np.ndarray:
    """steps 1-2 without the level shift and the final clamp: coefficients (..., 8, 8) [v][u] and a table (8, 8) or (64,) ->
    int64 (..., 8, 8) [y][x] (what IEEE 1180-1990 measures)"""
    c = np.asarray(coef).astype(np.int64)
    q = np.asarray(qt).astype(np.int64).reshape(8, 8)
    d = np.clip(c * q, -DEQUANT_CLAMP, DEQUANT_CLAMP)
    t = (np.einsum("...vu,xu->...vx", d, IDCT_MATRIX) + (1 << (PASS1_SHIFT - 1))) >> PASS1_SHIFT
    t = np.clip(t, -PASS1_CLAMP, PASS1_CLAMP)
    return (np.einsum("...vx,yv->...yx", t, IDCT_MATRIX) + (1 << (PASS2_SHIFT - 1))) >> PASS2_SHIFT


def idct_blocks_np(coef, qt) -> np.ndarray:
    """steps 1-2: -> samples uint8 (..., 8, 8) [y][x]"""
    return np.clip(idct_signed_np(coef, qt) + 128, 0, 255).astype(np.uint8)


def component_planes_np(coef, qt, ncomp, hs, vs, mcus_x, mcus_y):
    """the clamped component planes (what the kernel keeps in its workspace between its two launches): uint8
    (8 * block rows, 8 * block columns) each"""
    coef = np.asarray(coef).reshape(-1)
    qt = np.asarray(qt).reshape(ncomp, 64)
    out, off = [], 0
    for c, (bh, bw) in enumerate(plane_blocks(ncomp, hs, vs, mcus_x, mcus_y)):
        blocks = coef[off:off + bh * bw * 64].reshape(bh, bw, 8, 8)
        off += bh * bw * 64
        out.append(idct_blocks_np(blocks, qt[c]).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _axis_taps(n_out, factor, n_samples):
    """per output position: (nearer sample, farther sample, weights in quarters)"""
    i = np.arange(n_out)
    if factor == 1:
        return i, i, 4, 0
    near = i >> 1
    far = np.clip(near + np.where(i & 1, 1, -1), 0, n_samples - 1)
    return near, far, 3, 1


def upsample_plane_np(plane, width, height, hs, vs) -> np.ndarray:
    """step 3: a chroma plane -> int64 (height, width)"""
    p = np.asarray(plane).astype(np.int64)
    cw, ch = -(-width // hs), -(-height // vs)
    x0, x1, wx0, wx1 = _axis_taps(width, hs, cw)
    y0, y1, wy0, wy1 = _axis_taps(height, vs, ch)
    a, b = p[y0][:, x0], p[y0][:, x1]
    c, d = p[y1][:, x0], p[y1][:, x1]
    return (wx0 * wy0 * a + wx1 * wy0 * b + wx0 * wy1 * c + wx1 * wy1 * d + 8) >> 4


def ycc_to_rgb_np(y, cb, cr) -> np.ndarray:
    """step 4: int64 planes -> uint8 (H, W, 3)"""
    cb, cr = cb - 128, cr - 128
    r = y + ((CR_R * cr + 32768) >> 16)
    g = y + ((-CB_G * cb - CR_G * cr + 32768) >> 16)
    b = y + ((CB_B * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode_coefficients_np(coef, qt, width, height, ncomp, hs, vs) -> np.ndarray:
    """quantised coefficients + tables -> uint8 (height, width, 3): the whole device stage"""
    mcus_x, mcus_y = -(-width // (8 * hs)), -(-height // (8 * vs))
    planes = component_planes_np(coef, qt, ncomp, hs, vs, mcus_x, mcus_y)
    y = planes[0][:height, :width].astype(np.int64)
    if ncomp == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    return ycc_to_rgb_np(y, upsample_plane_np(planes[1], width, height, hs, vs), upsample_plane_np(planes[2], width, height, hs, vs))


def decode_np(data) -> np.ndarray:
    """JPEG bytes -> uint8 (H, W, 3) on the host: the entropy decoder and the specification"""
    nfo, coef, qt = coefficients(data)
    return decode_coefficients_np(coef, qt, nfo.width, nfo.height, nfo.ncomp, nfo.hs, nfo.vs)
