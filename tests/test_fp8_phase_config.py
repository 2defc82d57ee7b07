"""config.conv_fp8_phase (the "out"-form phase launches of the MX-fp8 mode on the MX-fp8 phase kernel): the switch is off
in every shipped configuration, is rejected without config.conv_fp8, and its C entry point is in the ctypes table.  The
fixture of the GPU parity tests (tests/test_gpu_mx8_phase.py) is checked here too: its tap sums quantise exactly.  No GPU needed."""
import numpy as np
import pytest


def _getters():
    from xmcgan_image_generation_amd.configs import coco_xmc
    return [getattr(coco_xmc, n) for n in sorted(dir(coco_xmc)) if n.startswith("get_") and n.endswith("config")]


def test_every_shipped_config_leaves_the_switch_off():
    getters = _getters()
    assert len(getters) >= 5
    for get in getters:
        cfg = get()
        assert "conv_fp8_phase" in cfg and cfg.conv_fp8_phase is False, get.__name__


def test_check_config_wants_conv_fp8_with_conv_fp8_phase():
    from xmcgan_image_generation_amd.configs import coco_xmc
    from xmcgan_image_generation_amd.nets import xmc_net
    cfg = coco_xmc.get_c1_config()
    cfg.conv_fp8_phase = True
    cfg.conv_fp8 = False
    with pytest.raises(ValueError, match="conv_fp8_phase"):
        xmc_net.check_config(cfg)
    cfg.conv_fp8 = True
    xmc_net.check_config(cfg)
    cfg = coco_xmc.get_c4_config()
    cfg.conv_fp8_phase = True
    xmc_net.check_config(cfg)


def test_phase_supported_entry_point_is_in_the_ctypes_table():
    from xmcgan_image_generation_amd import _lib
    assert "xmc_conv2d_mx8_phase_supported" in _lib.SIGNATURES
    assert _lib.SIGNATURES["xmc_conv2d_mx8_phase_supported"] == _lib.SIGNATURES["xmc_conv2d_phase_supported"]


def test_parity_fixture_quantises_exactly_under_both_scale_rules():
    """integers in [-3, 3] times one power of two per (row, 32-channel block): every "out"-form tap sum is an integer of
    magnitude <= 12 times that power -- exact in bf16 and in e4m3 under the next-binade and the OCP floor scale rule"""
    from tests.test_gpu_mx8_phase import assert_fixture_is_lossless, exact_master, phase_taps
    gen = np.random.default_rng(0)
    for layout in ("fwd", "dgrad"):
        master, wl = exact_master(64, 128, gen, layout)
        assert master.shape == ((64, 9, 128) if layout == "fwd" else (128, 9, 64)) and master.dtype == np.float32
        assert np.array_equal(master.astype(np.float64), wl if layout == "fwd" else wl[:, ::-1, :].transpose(2, 1, 0))
        e16 = phase_taps(wl)
        # the four phases of a window position partition the 3x3 taps: the 16 entries sum to the 9 taps
        assert np.array_equal(e16.sum(1), 4 * wl.sum(1))
        assert_fixture_is_lossless(wl)
    # and the emulation does notice a weight that is NOT exact
    bad = wl.copy()
    bad[0, 0, 0] = 1.0 + 2.0 ** -6
    with pytest.raises(AssertionError):
        assert_fixture_is_lossless(bad)
