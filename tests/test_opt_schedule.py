"""libml/opt_schedule.py on the CPU: the specification at its breakpoints, the constant descriptor's bits, the configuration
errors, and two C0 training steps on the CPU operator table whose optimiser calls receive the specification's rates.

The breakpoint constants are the issue's: W = 3, T0 = 4, T1 = 8, r = 0.25."""
import json
import os

import numpy as np
import pytest
import torch

from tests.cpu_ops import CpuOps
from tests.cpu_ops_guard import CpuOpsGuard
from xmcgan_image_generation_amd import synthetic as syn
from xmcgan_image_generation_amd import train_utils, xmc_gan
from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.libml import opt_schedule as OS
from xmcgan_image_generation_amd.nets import xmc_net

W, T0, T1, R = 3, 4, 8, 0.25
BASE = 2e-4


def _sched(kind, **kw):
    return OS.Schedule(**{**dict(kind=kind, base=BASE, warmup=W, decay_start=T0, decay_end=T1, final_ratio=R), **kw}).validate()


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _f(s, t):
    """the decay factor f alone: slot 6 of a schedule without warm-up"""
    return OS.evaluate(OS.Schedule(**{**vars(s), "warmup": 0}), t)[2]


# ------------------------------------------------------------------------------------------------------ the specification
def test_linear_exact_values_at_the_breakpoints():
    s = _sched(OS.LINEAR)
    # t: (w, f) written out by hand; x = (t - 4) / 4 between the horizons
    want = {1: (1.0 / 3.0, 1.0), 3: (1.0, 1.0), 4: (1.0, 1.0), 6: (1.0, 1.0 + (0.25 - 1.0) * 0.5), 8: (1.0, 0.25), 9: (1.0, 0.25)}
    assert want[6][1] == 0.625
    for t, (w, f) in want.items():
        lr, _, scale = OS.evaluate(s, t)
        assert lr.dtype == np.float32 and scale.dtype == np.float32
        assert _bits(lr) == _bits(np.float32((np.float64(BASE) * np.float64(w)) * np.float64(f))), t
        assert _bits(scale) == _bits(np.float32(np.float64(w) * np.float64(f))), t
    assert float(OS.evaluate(s, 2)[2]) == float(np.float32(2.0 / 3.0))


@pytest.mark.parametrize("kind", [OS.LINEAR, OS.COSINE])
def test_decaying_kinds_start_at_one_end_at_r_and_never_rise(kind):
    s = _sched(kind)
    assert float(_f(s, T0)) == 1.0 and float(_f(s, T1)) == R
    assert float(_f(s, 1)) == 1.0 and float(_f(s, T1 + 100)) == R
    fs = [float(_f(s, t)) for t in range(1, 14)]
    assert all(b <= a for a, b in zip(fs, fs[1:])), fs
    assert fs[T0 - 1] > fs[T0] > fs[T1 - 2] > fs[T1 - 1], "strictly falling between the horizons"
    if kind == OS.COSINE:                            # half way: r + (1 - r) / 2 up to cos(pi / 2)'s 6e-17
        assert abs(float(_f(s, 6)) - (R + (1 - R) * 0.5)) < 1e-7


def test_constant_descriptor_returns_the_bits_of_the_host_floats():
    for base, decay in ((1e-4, 0.999), (4e-4, 0.9999), (0.1, 0.0), (3.3333e-5, 0.5)):
        s = OS.Schedule(kind=OS.CONSTANT, base=base, ema_decay=decay).validate()
        for t in (1, 2, 1000, 2 ** 31 - 1):
            lr, d, scale = OS.evaluate(s, t)
            assert _bits(lr) == _bits(np.float32(base)) and _bits(d) == _bits(np.float32(decay)) and float(scale) == 1.0


def test_ema_decay_is_zero_up_to_the_start_then_ramps_to_the_cap():
    s = OS.Schedule(base=BASE, ema_decay=0.999, ema_ramp=10.0, ema_start=3).validate()
    ds = [float(OS.evaluate(s, t)[1]) for t in range(1, 40000, 7)]
    for t in (1, 2, 3):
        assert float(OS.evaluate(s, t)[1]) == 0.0
    assert _bits(OS.evaluate(s, 4)[1]) == _bits(np.float32(np.float64(5.0) / np.float64(14.0)))
    assert all(b >= a for a, b in zip(ds, ds[1:])), "never falls"
    assert max(ds) == float(np.float32(0.999)) == ds[-1], "capped at polyak_decay"
    # (1 + t) / (10 + t) >= 0.999 from t = 8990 on
    assert float(OS.evaluate(s, 8989)[1]) < float(np.float32(0.999)) == float(OS.evaluate(s, 8990)[1])
    plain = OS.Schedule(base=BASE, ema_decay=0.999, ema_start=3).validate()
    assert float(OS.evaluate(plain, 3)[1]) == 0.0 and _bits(OS.evaluate(plain, 4)[1]) == _bits(np.float32(0.999))


# (r, t) of a linear schedule with T0 = 0, T1 = 7 and no warm-up at which the specification's f = 1 + (r - 1) x, a rounded product
# and a rounded sum, and the same expression with ONE rounding (a fused multiply-add) land on different float32 values: the
# double results sit on either side of a float32 rounding boundary.  Found by a search over random r; tests/test_gpu_opt_schedule.py
# runs them on the device, where they tell a contracted v_fma_f64 in the advance kernel from the multiply and add it must be.
CONTRACTION_CASES = [("0x1.8816da7fffffep-1", 2), ("0x1.352dfb9999998p-3", 5), ("0x1.4f40f40000004p-3", 3)]


def contraction_schedule(r_hex):
    return OS.Schedule(kind=OS.LINEAR, base=2e-4, decay_end=7, final_ratio=float.fromhex(r_hex)).validate()


@pytest.mark.parametrize("r_hex,t", CONTRACTION_CASES)
def test_specification_rounds_the_product_and_the_sum_separately(r_hex, t):
    from fractions import Fraction
    r = float.fromhex(r_hex)
    x = float(np.float64(t) / np.float64(7))
    fused = float(Fraction(1) + Fraction(r - 1.0) * Fraction(x))       # exact, then ONE rounding to double: what an fma returns
    unfused = 1.0 + (r - 1.0) * x
    assert _bits(np.float32(fused)) != _bits(np.float32(unfused)), "the case must tell the two apart in float32"
    assert _bits(OS.evaluate(contraction_schedule(r_hex), t)[2]) == _bits(np.float32(unfused))


def _cfg(**kw):
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = 2
    cfg.update(kw)
    return cfg


def test_horizons_of_d_are_scaled_by_its_updates_per_step():
    cfg = _cfg(lr_schedule="linear", lr_warmup_steps=W, lr_decay_start_step=T0, lr_decay_end_step=T1, lr_final_ratio=R, ema_ramp=10.0,
               ema_start_step=2, d_step_per_g_step=3)
    g = OS.for_optimizer(cfg, "g", cfg.g_lr, cfg.polyak_decay)
    d = OS.for_optimizer(cfg, "d", cfg.d_lr, 0.0)
    assert (g.warmup, g.decay_start, g.decay_end, g.ema_start, g.ema_ramp, g.ema_decay) == (W, T0, T1, 2, 10.0, cfg.polyak_decay)
    assert (d.warmup, d.decay_start, d.decay_end) == (3 * W, 3 * T0, 3 * T1)
    assert (d.ema_start, d.ema_ramp, d.ema_decay) == (0, 0.0, 0.0), "the EMA keys act on G's optimiser only"
    assert g.base == cfg.g_lr and d.base == cfg.d_lr and g.kind == d.kind == OS.LINEAR
    # D's third update of training step s has the factor of G's update s
    for step in (1, 3, 4, 6, 8, 9):
        assert _bits(OS.evaluate(d, 3 * step)[2]) == _bits(OS.evaluate(g, step)[2])
    with pytest.raises(ValueError):
        OS.for_optimizer(cfg, "x", 1e-4)


def test_feature_is_off_without_its_keys():
    cfg = _cfg()
    assert not OS.enabled(cfg) and OS.for_optimizer(cfg, "g", cfg.g_lr, cfg.polyak_decay) is None
    assert not OS.enabled(_cfg(lr_final_ratio=0.5, lr_decay_start_step=3)), "these keys alone switch nothing on"
    for kw in (dict(lr_schedule="constant"), dict(lr_warmup_steps=1), dict(ema_ramp=1.0), dict(ema_start_step=1)):
        assert OS.enabled(_cfg(**kw)), kw
    assert OS.resolve(cfg, 100) is cfg
    dec = _cfg(lr_schedule="cosine")
    assert OS.resolve(dec, 100).lr_decay_end_step == 100 and "lr_decay_end_step" not in dec
    assert OS.resolve(_cfg(lr_schedule="cosine", lr_decay_end_step=7), 100).lr_decay_end_step == 7


@pytest.mark.parametrize("kw", [dict(lr_schedule="exponential"), dict(lr_schedule="linear"),       # (no end step outside train())
                                dict(lr_schedule="linear", lr_decay_start_step=5, lr_decay_end_step=5),
                                dict(lr_schedule="cosine", lr_decay_end_step=9, lr_final_ratio=1.5),
                                dict(lr_schedule="cosine", lr_decay_end_step=9, lr_final_ratio=float("nan")),
                                dict(lr_schedule="constant", lr_warmup_steps=-1), dict(lr_warmup_steps=2.5),
                                dict(lr_schedule="linear", lr_decay_start_step=-1, lr_decay_end_step=4),
                                dict(ema_ramp=-1.0, lr_schedule="constant"), dict(ema_ramp=float("inf")),
                                dict(ema_start_step=-2, lr_schedule="constant"), dict(ema_ramp=1.0, polyak_decay=1.0),
                                dict(lr_schedule="constant", g_lr=0.0), dict(lr_schedule="constant", g_lr=float("nan"))])
def test_configuration_errors_raise_value_error(kw):
    cfg = _cfg(**kw)
    with pytest.raises(ValueError):
        OS.for_optimizer(cfg, "g", cfg.g_lr, cfg.polyak_decay)


def test_create_train_state_refuses_a_bad_key_and_descriptor_errors():
    with pytest.raises(ValueError, match="lr_schedule"):
        train_utils.create_train_state(_cfg(lr_schedule="exponential"), 0, ops=CpuOps(torch.float32))
    OS.check_config(_cfg(lr_schedule="linear"))      # (the end step is train()'s to fill in)
    for bad in (dict(g_lr=0.0), dict(d_lr=float("nan")), dict(d_lr=-1e-4), dict(polyak_decay=1.0)):     # the descriptors' base values
        with pytest.raises(ValueError, match=next(iter(bad))):
            train_utils.create_train_state(_cfg(lr_warmup_steps=2, **bad), 0, ops=CpuOps(torch.float32))
        OS.check_config(_cfg(**bad))                 # (without a schedule they are not this module's to judge)
    good = dict(kind=OS.LINEAR, base=1e-4, warmup=0, decay_start=0, decay_end=5, final_ratio=0.0, ema_decay=0.9, ema_ramp=0.0,
                ema_start=0)
    OS.Schedule(**good).validate()
    for bad in (dict(kind=3), dict(base=0.0), dict(base=float("inf")), dict(warmup=-1), dict(decay_start=-1), dict(decay_end=-1),
                dict(ema_start=-1), dict(decay_end=0), dict(final_ratio=-0.1), dict(final_ratio=float("nan")), dict(ema_decay=1.0),
                dict(ema_decay=-0.1), dict(ema_decay=float("nan")), dict(ema_ramp=-1.0), dict(ema_ramp=float("nan"))):
        with pytest.raises(ValueError):
            OS.Schedule(**{**good, **bad}).validate()
    with pytest.raises(ValueError):
        OS.evaluate(OS.Schedule(**good), 0)


# ------------------------------------------------------------------------------------- the training step on the CPU table
class RecordingOps(CpuOps):
    """the CPU table with its ``adam_ema`` wrapped: (number of elements, lr, ema_decay, step, has EMA) of every call"""

    def __init__(self, dtype=torch.float32):
        super().__init__(dtype)
        self.calls = []

    def adam_ema(self, p, g, m, v, ema, *, lr, ema_decay=0.0, step, **kw):
        self.calls.append((p.numel(), lr, ema_decay, step, ema is not None))
        return super().adam_ema(p, g, m, v, ema, lr=lr, ema_decay=ema_decay, step=step, **kw)


def _two_steps(cfg):
    ops = RecordingOps(torch.float32)
    gen, disc, state = train_utils.create_train_state(cfg, 0, ops=ops)
    for step in (1, 2):
        batch = {k: torch.as_tensor(v) for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size, seed=step).items()}
        state, _ = train_utils.train_step(step, state, batch, xmc_gan, gen, disc, cfg, {})
    g_n, d_n = state.g_optimizer.arena.params.numel(), state.d_optimizer.arena.params.numel()
    assert g_n != d_n
    g = [c[1:] for c in ops.calls if c[0] == g_n]
    d = [c[1:] for c in ops.calls if c[0] == d_n]
    assert len(g) + len(d) == len(ops.calls)
    return g, d, state


def test_two_training_steps_pass_the_specifications_rates():
    """fails on a step that hands the optimiser config.g_lr / d_lr / polyak_decay: the rates move with Adam's t"""
    cfg = _cfg(lr_schedule="linear", lr_warmup_steps=2, lr_decay_start_step=1, lr_decay_end_step=3, lr_final_ratio=0.25, ema_ramp=10.0)
    n = cfg.d_step_per_g_step
    assert n == 2
    g, d, state = _two_steps(cfg)
    sg, sd = OS.for_optimizer(cfg, "g", cfg.g_lr, cfg.polyak_decay), OS.for_optimizer(cfg, "d", cfg.d_lr, 0.0)
    assert [c[2] for c in g] == [1, 2] and [c[2] for c in d] == [1, 2, 3, 4] and all(c[3] for c in g) and not any(c[3] for c in d)
    for calls, s, has_ema in ((g, sg, True), (d, sd, False)):
        for lr, decay, t, _ in calls:
            want_lr, want_d, _ = OS.evaluate(s, t)
            assert isinstance(lr, float) and lr == float(want_lr), (t, lr, float(want_lr))
            assert decay == (float(want_d) if has_ema else 0.0), (t, decay)
    assert len({c[0] for c in d}) == 4 and len({c[0] for c in g}) == 2 and len({c[1] for c in g}) == 2, "the rates really move"
    assert g[0][0] == float(np.float32(cfg.g_lr * 0.5)) and g[0][1] == float(np.float32(2.0 / 11.0))
    rates = train_utils.optimizer_rates(state, cfg)
    assert rates == {"opt/g_lr": g[-1][0], "opt/ema_decay": g[-1][1], "opt/d_lr": d[-1][0]}


def test_two_training_steps_without_the_keys_pass_the_constants():
    cfg = _cfg()
    g, d, _ = _two_steps(cfg)
    assert [c[:2] for c in g] == [(cfg.g_lr, cfg.polyak_decay)] * 2
    assert [c[:2] for c in d] == [(cfg.d_lr, 0.0)] * 4


def test_device_counter_without_scheduled_forms_is_an_error_not_a_constant_rate():
    cfg = _cfg(lr_schedule="constant", lr_warmup_steps=2, skip_nonfinite_updates=True)
    ops = CpuOpsGuard(torch.float32)
    assert hasattr(ops, "adam_ema_dev") and not hasattr(ops, "adam_ema_dev_sched")
    gen, disc, state = train_utils.create_train_state(cfg, 0, ops=ops)
    assert state.g_optimizer.arena.step_state is not None and state.g_optimizer.arena.step_state.numel() == OS.STATE_WIDTH
    batch = {k: torch.as_tensor(v) for k, v in syn.make_batch(cfg, per_device_batch=cfg.batch_size, seed=1).items()}
    with pytest.raises(ValueError, match="adam_ema_dev_sched"):
        train_utils.train_step(1, state, batch, xmc_gan, gen, disc, cfg, {})


def test_train_resolves_the_end_step_and_writes_the_rates(tmp_path):
    """``train`` on the CPU table, 3 steps of a cosine schedule without lr_decay_end_step: it ends with the run, and every line of
    metrics.jsonl carries the rates of the window's last update"""
    from tests.test_train_loop import synthetic_datasets
    xmc_net.set_ops_factory(lambda dtype: CpuOps(dtype))
    try:
        cfg = _cfg(num_train_steps=3, eval_every_steps=1, checkpoint_every_steps=100, lr_schedule="cosine", lr_final_ratio=0.5,
                   ema_start_step=1)
        state = train_utils.train(cfg, str(tmp_path), datasets=synthetic_datasets())
    finally:
        xmc_net.set_ops_factory(None)
    assert "lr_decay_end_step" not in cfg
    assert json.load(open(os.path.join(str(tmp_path), "config.json")))["lr_decay_end_step"] == 3
    lines = [json.loads(line) for line in open(os.path.join(str(tmp_path), "metrics.jsonl"))]
    assert [line["step"] for line in lines] == [1, 2, 3]
    full = dict(cfg, lr_decay_end_step=3)
    full = coco_xmc.ConfigDict(full)
    sg, sd = OS.for_optimizer(full, "g", cfg.g_lr, cfg.polyak_decay), OS.for_optimizer(full, "d", cfg.d_lr, 0.0)
    for line in lines:
        t = line["step"]
        assert line["opt/g_lr"] == float(OS.evaluate(sg, t)[0]) and line["opt/d_lr"] == float(OS.evaluate(sd, 2 * t)[0])
        assert line["opt/ema_decay"] == (0.0 if t == 1 else float(np.float32(cfg.polyak_decay)))
    assert lines[-1]["opt/g_lr"] == float(np.float32(cfg.g_lr * 0.5)) and lines[0]["opt/g_lr"] > lines[1]["opt/g_lr"]
    assert state.g_optimizer.arena.opt_step == 3
