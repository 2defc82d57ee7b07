"""config.conv_fp8_phase_in (the "in"-form phase launches of the MX-fp8 mode, avg_pool2(conv3x3(.)), on the MX-fp8 "in" phase
kernel): the switch is off in every shipped configuration, is rejected without config.conv_fp8, and its C entry points are in
the ctypes table and the header.  The fixture of the GPU parity tests (tests/test_gpu_mx8_phase_in.py) is checked here too: its
"in"-form tap sums quantise exactly, and the tap sets themselves reproduce float64 avg_pool2d(conv2d(.)).  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("xmc_conv2d_mx8_phase_in_supported", "xmc_conv2d_mx8_phase_in_workspace_bytes", "xmc_conv2d_mx8_phase_in",
                "xmc_conv2d_mx8_phase_in_bits")


def _getters():
    from xmcgan_image_generation_amd.configs import coco_xmc
    return [getattr(coco_xmc, n) for n in sorted(dir(coco_xmc)) if n.startswith("get_") and n.endswith("config")]


def test_every_shipped_config_leaves_the_switch_off():
    getters = _getters()
    assert len(getters) >= 5
    for get in getters:
        cfg = get()
        assert "conv_fp8_phase_in" in cfg and cfg.conv_fp8_phase_in is False, get.__name__


def test_check_config_wants_conv_fp8_with_conv_fp8_phase_in():
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.nets import xmc_net
    cfg = coco_xmc.get_c1_config()
    cfg.conv_fp8_phase_in = True
    cfg.conv_fp8 = False
    with pytest.raises(ValueError, match="conv_fp8_phase_in"):
        xmc_net.check_config(cfg)
    cfg.conv_fp8 = True
    xmc_net.check_config(cfg)                              # independent of conv_fp8_phase: either, both or neither
    cfg.conv_fp8_phase = True
    xmc_net.check_config(cfg)
    cfg = coco_xmc.get_c4_config()
    cfg.conv_fp8_phase_in = True
    xmc_net.check_config(cfg)


def test_in_form_entry_points_are_in_the_ctypes_table_and_the_header():
    from xmcgan_image_generation_amd import _lib
    assert _lib.ABI_VERSION >= 25
    src = open(os.path.join(ROOT, "include", "xmcgan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint(?:64_t)?\s+" + name + r"\s*\(", src), name
    assert _lib.SIGNATURES["xmc_conv2d_mx8_phase_in_supported"] == _lib.SIGNATURES["xmc_conv2d_mx8_phase_supported"]
    assert _lib.SIGNATURES["xmc_conv2d_mx8_phase_in_workspace_bytes"] == _lib.SIGNATURES["xmc_conv2d_mx8_workspace_bytes"]
    assert "xmc_conv2d_mx8_phase_in_workspace_bytes" in _lib._INT64_RETURNS
    assert len(_lib.SIGNATURES["xmc_conv2d_mx8_phase_in_bits"]) == len(_lib.SIGNATURES["xmc_conv2d_mx8_phase_in"]) + 1


def test_in_taps_reproduce_avg_pool_of_conv3x3_in_float64():
    """the identity the kernel is built on, with exactly the helper the GPU reference is checked with: decomposed by the parity
    of the input pixel, 16 tap sums per output pixel -- against F.avg_pool2d(F.conv2d(pad(x), w), 2) at magnitude ~5e5"""
    from tests.test_gpu_mx8_phase_in import in_form_by_parity, in_taps, ref_pooled
    gen = np.random.default_rng(11)
    for n, h, w_, c, rows in ((2, 4, 4, 5, 3), (1, 6, 10, 8, 4), (3, 2, 2, 4, 2)):
        x = torch.from_numpy(gen.standard_normal((n, 2 * h, 2 * w_, c)) * 700.0)
        wl = gen.standard_normal((rows, 9, c)) * 700.0
        f16 = in_taps(wl)
        assert np.allclose(f16.sum(1), 4 * wl.sum(1), rtol=1e-12, atol=1e-9)       # every 3x3 tap is counted four times
        got = in_form_by_parity(x, f16)
        wt = torch.from_numpy(wl).reshape(rows, 3, 3, c).permute(0, 3, 1, 2).contiguous()
        ref = F.avg_pool2d(F.conv2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)), wt), 2).permute(0, 2, 3, 1)
        assert float(ref.abs().max()) > 1e5
        assert float((got - ref).abs().max()) < 1e-8 * float(ref.abs().max()), (n, h, w_, c, rows)
        if h == w_:                                                                # the banded reference of the GPU tests agrees too
            (r0, r1, full), = ref_pooled(x, wl, None)
            assert (r0, r1) == (0, h) and float((full - ref).abs().max()) < 1e-8 * float(ref.abs().max())
            lo = ref_pooled(x, wl, [(0, 1), (h - 1, h)])
            assert torch.equal(lo[0][2], full[:, 0:1]) and torch.equal(lo[1][2], full[:, h - 1:h])


def test_in_form_parity_fixture_quantises_exactly_under_both_scale_rules():
    """integers in [-3, 3] times one power of two per (row, 32-channel block): every "in"-form tap sum is an integer of
    magnitude <= 12 times that power -- exact in bf16 and in e4m3 under the next-binade and the OCP floor scale rule"""
    from tests.test_gpu_mx8_phase import exact_master
    from tests.test_gpu_mx8_phase_in import assert_in_fixture_is_lossless, in_taps
    gen = np.random.default_rng(0)
    for layout in ("fwd", "dgrad"):
        master, wl = exact_master(64, 128, gen, layout)
        f16 = in_taps(wl)
        assert np.array_equal(f16.sum(1), 4 * wl.sum(1))
        blocks = np.abs(f16).reshape(64, 16, 4, 32)
        unit = np.abs(wl).reshape(64, 9, 4, 32)
        unit = np.where(unit > 0, unit, np.inf).min(axis=(1, 3))                   # <= 3 x the block's power of two
        assert (blocks.max(axis=(1, 3)) <= 12 * unit).all()
        assert assert_in_fixture_is_lossless(wl) <= 448.0
    # and the emulation does notice a weight that is NOT exact
    bad = wl.copy()
    bad[0, 0, 0] = 1.0 + 2.0 ** -6
    with pytest.raises(AssertionError):
        assert_in_fixture_is_lossless(bad)
