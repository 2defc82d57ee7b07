"""Learning-rate and EMA-decay schedules evaluated on the device.  Not part of the reference.

A schedule is a pure function of an optimiser's own update count ``t`` (Adam's t, already in device memory:
``ParamArena.step_state``) and of constants.  The kernel that advances ``t`` evaluates it in double precision and leaves the
float32 results in ``step_state``; the Adam kernels read them there instead of taking host floats that a captured graph would
freeze.  One graph launch per step and no host read stay true, and nothing new goes into a checkpoint: ``t`` is saved already.

This module is NumPy first: ``evaluate`` is the written specification of the scheduled advance kernel (csrc/pointwise.hip) --
IEEE double, every operation written out in a fixed order, no multiply fused with an add -- and the host fallback of an operator
table without a device counter.

Configuration (every key absent = off; ``enabled``):

* ``lr_schedule``: ``"constant"``, ``"linear"`` or ``"cosine"``, for G and D alike (the base rates stay ``g_lr`` / ``d_lr``);
* ``lr_warmup_steps`` (0), ``lr_decay_start_step`` (0), ``lr_decay_end_step`` (``train`` fills in the number of training steps;
  elsewhere a decaying schedule without it is an error), ``lr_final_ratio`` (0.0);
* ``ema_ramp`` (0 = off) and ``ema_start_step`` (0): G's optimiser only.

Step counts in the config are TRAINING steps; the kernel counts the updates of one optimiser.  ``for_optimizer`` converts by the
updates that optimiser receives per training step: 1 for G, ``d_step_per_g_step`` for D.  Under ``skip_nonfinite_updates`` a
skipped update does not advance ``t``: the schedule counts APPLIED updates and may lag ``state.step``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

CONSTANT, LINEAR, COSINE = 0, 1, 2                 # xmc_opt_schedule.kind (include/xmcgan_hip.h)
KINDS = {"constant": CONSTANT, "linear": LINEAR, "cosine": COSINE}
STATE_WIDTH = 8                                    # step_state: [t, ic1, ic2, pad, lr_t, d_t, w * f, pad] as float32
SLOT_LR, SLOT_DECAY, SLOT_SCALE = 4, 5, 6
KEYS = ("lr_schedule", "lr_warmup_steps", "lr_decay_start_step", "lr_decay_end_step", "lr_final_ratio", "ema_ramp", "ema_start_step")


@dataclass(frozen=True)
class Schedule:
    """The descriptor of one optimiser's schedule, horizons in UPDATES of that optimiser (xmc_opt_schedule)"""
    kind: int = CONSTANT
    base: float = 1.0              # the base learning rate
    warmup: int = 0                # W
    decay_start: int = 0           # T0
    decay_end: int = 0             # T1 (read by the decaying kinds only)
    final_ratio: float = 0.0       # r
    ema_decay: float = 0.0         # polyak_decay (0 where the optimiser keeps no EMA copy)
    ema_ramp: float = 0.0
    ema_start: int = 0             # S

    def validate(self):
        """ValueError for whatever the library answers with XMC_EINVAL -> self"""
        if self.kind not in (CONSTANT, LINEAR, COSINE):
            raise ValueError(f"opt_schedule: unknown kind {self.kind}")
        if not (math.isfinite(self.base) and self.base > 0.0):
            raise ValueError(f"opt_schedule: the base rate must be finite and > 0, got {self.base}")
        for name in ("warmup", "decay_start", "decay_end", "ema_start"):
            v = getattr(self, name)
            if int(v) != v or v < 0:
                raise ValueError(f"opt_schedule: {name} must be an integer >= 0, got {v}")
        if self.kind != CONSTANT and self.decay_end <= self.decay_start:
            raise ValueError(f"opt_schedule: a decaying schedule needs decay_end > decay_start, got {self.decay_end} <= "
                             f"{self.decay_start}")
        if not (math.isfinite(self.final_ratio) and 0.0 <= self.final_ratio <= 1.0):
            raise ValueError(f"opt_schedule: final_ratio must be in [0, 1], got {self.final_ratio}")
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError(f"opt_schedule: ema_decay must be in [0, 1), got {self.ema_decay}")
        if not (math.isfinite(self.ema_ramp) and self.ema_ramp >= 0.0):
            raise ValueError(f"opt_schedule: ema_ramp must be finite and >= 0, got {self.ema_ramp}")
        return self


def evaluate(s: Schedule, t: int):
    """The specification: the update that makes the counter ``t`` (t >= 1) -> (lr_t, d_t, w * f), each a float32"""
    t = int(t)
    if t < 1:
        raise ValueError(f"opt_schedule.evaluate: t counts updates from 1, got {t}")
    f64 = np.float64
    td = f64(t)
    with np.errstate(all="ignore"):
        w = td / f64(s.warmup) if (s.warmup > 0 and t < s.warmup) else f64(1.0)
        if t <= s.decay_start:
            x = f64(0.0)
        elif t >= s.decay_end:
            x = f64(1.0)
        else:
            x = f64(t - s.decay_start) / f64(s.decay_end - s.decay_start)
        r = f64(s.final_ratio)
        if s.kind == LINEAR:
            f = f64(1.0) + (r - f64(1.0)) * x
        elif s.kind == COSINE:
            f = r + (f64(1.0) - r) * (f64(0.5) * (f64(1.0) + np.cos(f64(np.pi) * x)))
        else:
            f = f64(1.0)
        lr = np.float32((f64(s.base) * w) * f)
        scale = np.float32(w * f)
        if t <= s.ema_start:
            d = np.float32(0.0)
        elif s.ema_ramp > 0.0:
            d = np.float32(min(f64(s.ema_decay), (f64(1.0) + td) / (f64(s.ema_ramp) + td)))
        else:
            d = np.float32(f64(s.ema_decay))
    return lr, d, scale


# ------------------------------------------------------------------------------------------------------- configuration
def enabled(config) -> bool:
    return bool(config.get("lr_schedule", "") or config.get("lr_warmup_steps", 0) > 0 or config.get("ema_ramp", 0) > 0
                or config.get("ema_start_step", 0) > 0)


def _steps(config, key, default=0):
    v = config.get(key, default)
    if isinstance(v, bool) or int(v) != v or int(v) < 0:
        raise ValueError(f"config.{key} must be an integer >= 0 (training steps), got {v!r}")
    return int(v)


def settings(config, need_end=True):
    """-> dict(kind, warmup, decay_start, decay_end, final_ratio, ema_ramp, ema_start), in TRAINING steps, validated; ValueError
    on a value outside its domain.  ``need_end``: a decaying schedule without ``lr_decay_end_step`` is an error (``train``
    resolves the key before the first step; ``create_train_state`` runs before that and passes False)"""
    name = config.get("lr_schedule", "") or "constant"
    if name not in KINDS:
        raise ValueError(f"config.lr_schedule must be one of {sorted(KINDS)} (or absent), got {name!r}")
    kind = KINDS[name]
    warmup, start = _steps(config, "lr_warmup_steps"), _steps(config, "lr_decay_start_step")
    end = _steps(config, "lr_decay_end_step") if config.get("lr_decay_end_step", None) is not None else None
    ratio, ramp = float(config.get("lr_final_ratio", 0.0)), float(config.get("ema_ramp", 0.0) or 0.0)
    if not (math.isfinite(ratio) and 0.0 <= ratio <= 1.0):
        raise ValueError(f"config.lr_final_ratio must be in [0, 1], got {ratio}")
    if not (math.isfinite(ramp) and ramp >= 0.0):
        raise ValueError(f"config.ema_ramp must be finite and >= 0, got {ramp}")
    if kind != CONSTANT:
        if end is None:
            if need_end:
                raise ValueError(f"config.lr_schedule = {name!r} needs config.lr_decay_end_step (train() fills in the number of "
                                 "training steps; outside it the key must be set)")
        elif end <= start:
            raise ValueError(f"config.lr_decay_end_step ({end}) must be greater than config.lr_decay_start_step ({start})")
    return dict(kind=kind, warmup=warmup, decay_start=start, decay_end=end if end is not None else 0, final_ratio=ratio,
                ema_ramp=ramp, ema_start=_steps(config, "ema_start_step"))


def check_config(config) -> None:
    """what ``create_train_state`` checks before it allocates anything: the keys that are present are inside their domains, and
    with the feature on so are the base values the descriptors are built from (``g_lr``, ``d_lr``, ``polyak_decay``)"""
    if any(k in config for k in KEYS):
        settings(config, need_end=False)
    if enabled(config):
        for key in ("g_lr", "d_lr"):
            base = float(config[key])
            if not (math.isfinite(base) and base > 0.0):
                raise ValueError(f"config.{key} must be finite and > 0 under a schedule, got {base}")
        decay = float(config.polyak_decay)
        if config.get("ema", True) and not 0.0 <= decay < 1.0:
            raise ValueError(f"config.polyak_decay must be in [0, 1) under a schedule, got {decay}")


def resolve(config, num_train_steps):
    """``train``: a decaying schedule without ``lr_decay_end_step`` ends at the resolved number of training steps -> the config
    itself, or a copy that carries the key"""
    if not enabled(config) or KINDS.get(config.get("lr_schedule", "") or "constant", CONSTANT) == CONSTANT:
        return config
    if config.get("lr_decay_end_step", None) is not None:
        return config
    config = config.copy()
    config["lr_decay_end_step"] = int(num_train_steps)
    return config


def updates_per_step(config, role) -> int:
    """updates the ``role`` ("g" | "d") optimiser receives per training step, as ``train_step`` issues them"""
    if role not in ("g", "d"):
        raise ValueError(f"opt_schedule: role must be 'g' or 'd', got {role!r}")
    return 1 if role == "g" else int(config.d_step_per_g_step)


def for_optimizer(config, role, base, ema_decay=0.0):
    """-> the ``Schedule`` of the ``role`` optimiser, horizons in its own updates, or None when the feature is off.  ``base``: its
    base rate (``g_lr`` / ``d_lr``); ``ema_decay``: ``polyak_decay`` where the update keeps an EMA copy (G), else 0 -- the two
    EMA keys act on G's optimiser only."""
    if not enabled(config):
        return None
    s, k = settings(config), updates_per_step(config, role)
    ema = role == "g"
    return Schedule(kind=s["kind"], base=float(base), warmup=s["warmup"] * k, decay_start=s["decay_start"] * k,
                    decay_end=s["decay_end"] * k, final_ratio=s["final_ratio"], ema_decay=float(ema_decay) if ema else 0.0,
                    ema_ramp=s["ema_ramp"] if ema else 0.0, ema_start=s["ema_start"] * k if ema else 0).validate()


def read_slots(step_state):
    """``step_state`` (a float32[8] tensor; a host synchronisation) -> dict(lr, ema_decay, scale) as the last update left them"""
    s = step_state.detach().cpu().tolist()
    return dict(lr=s[SLOT_LR], ema_decay=s[SLOT_DECAY], scale=s[SLOT_SCALE])
