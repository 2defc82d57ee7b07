"""The codec library (include/xmc_codec.h, libxmc_codec.so) is its own ABI: header, exports and ctypes table agree, and the
product library and its ABI version know nothing of it.  No GPU needed (no compute calls)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\bint(?:64_t)?\s+(xmc_\w+)\s*\(", src)))


def test_codec_header_exports_and_table_agree():
    from xmcgan_image_generation_amd import _lib
    names = _declared("xmc_codec.h")
    assert sorted(_lib.CODEC_SIGNATURES) == names and len(names) == 6
    assert os.path.exists(_lib.CODEC_LIB_PATH), "build it first: make -C xmcgan_image_generation_amd/csrc_codec"
    lib = _lib.load_codec()
    assert lib.xmc_codec_abi_version() == _lib.CODEC_ABI_VERSION == 1
    product = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert not hasattr(product, n), f"{n} is exported by the product library"
    assert not set(names) & set(_declared("xmcgan_hip.h")) and not set(names) & set(_declared("xmc_probe.h"))
    assert _lib.ABI_VERSION == 36 and product.xmc_abi_version() == 36


def test_host_library_abi_is_5():
    from xmcgan_image_generation_amd.libml import _io
    assert _io.load().xmc_io_abi_version() == 5


def test_workspace_functions_validate_the_table_on_the_host():
    """(host arithmetic only: nothing is launched)"""
    from xmcgan_image_generation_amd import _lib
    from xmcgan_image_generation_amd.libml import codec
    lib = _lib.load_codec()
    assert lib.xmc_jpeg_plane_bytes(37, 29, 3, 2, 2) == (3 * 2 * 2 * 2 + 2 * 3 * 2) * 64
    assert lib.xmc_jpeg_plane_bytes(37, 29, 3, 1, 2) == -22 and lib.xmc_jpeg_plane_bytes(0, 29, 1, 1, 1) == -22
    layout = codec.BatchLayout([(37, 29, 3, 2, 2), (1, 1, 1, 1, 1), (17, 9, 3, 2, 1)])
    d = np.ascontiguousarray(layout.desc)
    assert lib.xmc_jpeg_decode_workspace_bytes(d.ctypes.data, 3) == 512 + layout.plane_bytes
    assert lib.xmc_png_filter_workspace_bytes(d.ctypes.data, 3) == 512 + 4 * layout.rows
    assert layout.rows == 29 + 1 + 9 and layout.coef_elems == layout.plane_bytes
    bad = d.copy()
    bad[1, codec.D_H] = 16385
    assert lib.xmc_jpeg_decode_workspace_bytes(bad.ctypes.data, 3) == -22 and lib.xmc_png_filter_workspace_bytes(bad.ctypes.data, 3) == -22
    assert lib.xmc_jpeg_decode_workspace_bytes(d.ctypes.data, 0) == -22
