#!/usr/bin/env python
"""Record what the host-side geometry queries of the convolution launchers answer (tests/golden/conv_geometry.npz, replayed by
tests/test_conv_geometry.py).  The queries are pure host functions: no GPU needed.

Record from a library built from the PARENT of the change under test, never from the code under test:
    python tools/record_conv_geometry.py --lib /path/to/parent/libxmcgan_hip.so [--out tests/golden/conv_geometry.npz]
"""
import argparse
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xmcgan_image_generation_amd import _lib  # noqa: E402

CONV_QUERIES = ("xmc_conv2d_workspace_bytes", "xmc_conv2d_phase_supported", "xmc_conv2d_mx8_workspace_bytes",
                "xmc_conv2d_mx8_phase_supported", "xmc_conv2d_mx8_phase_in_supported", "xmc_conv2d_mx8_phase_in_workspace_bytes")
TUNING_DEFAULTS = {"ksplit_target": 256, "ksplit_target_phase": 384, "ksplit_target_pw": 256, "tile64_pct": 100,
                   "wgrad_target_hi": 384, "wgrad_target_lo": 512, "wgrad_target_phase": 384}
WGRAD_NO_PHASE = 0x100               # xmc_wgrad_desc.variant bit 8 (XMC_WGRAD_NO_PHASE)


def conv_grid():
    """rows (n, h = w, cin, cout, ks, ups, pool_out, w_packed)"""
    return [(n, h, cin, cout, ks, ups, pool, wp) for n, h, cin, cout, ks, (ups, pool, wp) in itertools.product(
        (1, 2, 3, 56, 112), (2, 4, 8, 16, 32, 64, 128), (32, 64, 96, 192, 768, 1536, 2048), (3, 32, 64, 96, 192, 512, 1536), (1, 3),
        ((0, 0, 1), (1, 0, 1), (1, 0, 17), (0, 1, 17), (0, 1, 1), (1, 0, 49), (1, 0, 145)))]


def wgrad_grid():
    """rows (n, h = w, cin, cout, ks, x_ups, dy_ups, variant)"""
    return [(n, h, cin, cout, ks, xu, du, v) for n, h, cin, cout, ks, (xu, du), v in itertools.product(
        (1, 2, 8, 56), (4, 8, 16, 32, 64, 128), (32, 96, 192, 768, 1536), (32, 96, 192, 768, 1536), (1, 3),
        ((0, 0), (1, 0), (0, 1)), (1, 1 | WGRAD_NO_PHASE))]


def network_layers():
    """(n, h_in, cin, cout, ks, ups, pool_out) of the forward convolutions of the C1 (128 px, batch 56) and C3 (256 px, batch 32)
    networks; the discriminator sees real and generated images (2 x batch)"""
    out = []
    for size, b, g_ch, d_ch in ((128, 56, (16, 8, 4, 2, 1), ((2, 1), (4, 1), (8, 1), (16, 1), (16, 0))),
                                (256, 32, (16, 8, 8, 4, 2, 1), ((2, 1), (4, 1), (8, 1), (8, 1), (16, 1), (16, 0)))):
        cin, h = 96 * 16, 4
        for c in g_ch:                                   # generator block: conv3x3(upsample), conv3x3, 1x1 shortcut
            out += [(b, h, cin, 96 * c, 3, 1, 0), (b, 2 * h, 96 * c, 96 * c, 3, 0, 0), (b, h, cin, 96 * c, 1, 0, 0)]
            cin, h = 96 * c, 2 * h
        out += [(b, h, 96, 3, 3, 0, 0), (b, 16, 1024, 768, 1, 0, 0)]
        out += [(2 * b, size, 96, 96, 3, 0, 1)]          # discriminator: optimized block's second convolution, then the blocks
        cin, h = 96, size // 2
        for c, down in d_ch:
            out += [(2 * b, h, cin, 96 * c, 3, 0, 0), (2 * b, h, 96 * c, 96 * c, 3, 0, down), (2 * b, h, cin, 96 * c, 1, 0, 0)]
            cin, h = 96 * c, h // 2 if down else h
    return out


def network_conv_rows():
    """forward and data-gradient descriptors of network_layers(), on plain and on phase weights"""
    rows = []
    for n, h, cin, cout, ks, ups, pool in network_layers():
        ho = 2 * h if ups else h // 2 if pool else h
        for wp in (1, 17):
            rows.append((n, h, cin, cout, ks, ups, pool, wp))
            rows.append((n, ho, cout, cin, ks, pool, ups, wp))       # the adjoint: pooled <-> upsampled
    return rows


def network_wgrad_rows():
    return [(n, h, cin, cout, ks, ups, pool, v) for n, h, cin, cout, ks, ups, pool in network_layers() if cout % 32 == 0
            for v in (1, 1 | WGRAD_NO_PHASE)]


def conv_desc(row):
    n, h, cin, cout, ks, ups, pool, wp = (int(v) for v in row)
    return _lib.ConvDesc(n, h, h, cin, cout, ks, ups, 0, 0, 0, _lib.XMC_BF16, 1.0, 1.0, wp, pool, 0, 0, 0, 0, None)


def wgrad_desc(row):
    n, h, cin, cout, ks, xu, du, v = (int(v) for v in row)
    return _lib.WgradDesc(n, h, h, cin, cout, ks, xu, 0, du, _lib.XMC_BF16, v, 1.0)


def answers(lib, conv_rows, wgrad_rows):
    """-> (len(conv_rows), 6) and (len(wgrad_rows),) int64: what the queries of ``lib`` (a ctypes.CDLL) answer"""
    fns = []
    for name in CONV_QUERIES + ("xmc_conv2d_wgrad_workspace_bytes",):
        fn = getattr(lib, name)
        fn.restype = C.c_int64 if name.endswith("workspace_bytes") else C.c_int
        fns.append(fn)
    conv = np.zeros((len(conv_rows), len(CONV_QUERIES)), np.int64)
    for i, row in enumerate(conv_rows):
        d = C.byref(conv_desc(row))
        conv[i] = [fn(d) for fn in fns[:-1]]
    wgrad = np.array([fns[-1](C.byref(wgrad_desc(row))) for row in wgrad_rows], np.int64)
    return conv, wgrad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libxmcgan_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_geometry.npz"))
    args = ap.parse_args()
    lib = C.CDLL(args.lib)
    for key, want in TUNING_DEFAULTS.items():
        v = C.c_int32()
        assert lib.xmc_get_tuning(key.encode(), C.byref(v)) == 0 and v.value == want, (key, v.value, want)
    conv_rows, wgrad_rows = conv_grid() + network_conv_rows(), wgrad_grid() + network_wgrad_rows()
    conv, wgrad = answers(lib, conv_rows, wgrad_rows)
    ng, nw = len(conv_grid()), len(wgrad_grid())
    print("conv grid", ng, "non-zero", (conv[:ng] != 0).sum(0).tolist(), "distinct workspace values",
          [len(np.unique(conv[:ng, j])) for j in (0, 2, 5)], "| network rows", len(conv_rows) - ng)
    print("wgrad grid", nw, "non-zero", int((wgrad[:nw] != 0).sum()), "distinct", len(np.unique(wgrad[:nw])),
          "| network rows", len(wgrad_rows) - nw)
    np.savez_compressed(args.out, conv_desc=np.array(conv_rows, np.int32), conv_answers=conv,
                        wgrad_desc=np.array(wgrad_rows, np.int32), wgrad_answers=wgrad)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
