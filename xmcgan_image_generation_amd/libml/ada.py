"""Adaptive discriminator augmentation (``config.ada_target``; Karras et al., "Training Generative Adversarial Networks with
Limited Data", NeurIPS 2020): the strength of ``config.diff_augment`` is decided on the device, per image and per part, from
the discriminator's own logits.  Not part of the reference.

Every part of a plan row (libml/diff_augment.py) is applied with probability ``p``: the batch carries, next to the plan ``d_aug``,
one uniform per (sample, real / generated, part) under ``d_aug_u`` (``draw_gates``), and a part whose uniform is not below ``p``
takes its identity value (``gate``).  A controller moves ``p`` so that the overfitting heuristic r_t = E[sign(D(real))] stays at
``ada_target`` (``update``): every ``ada_interval`` half steps ``p`` goes up or down by (real images seen since the last
adjustment) / (``ada_kimg`` * 1000), clamped to [0, ``P_MAX``].

This module is NumPy first: ``gate`` and ``update`` are the written specification of ``xmc_ada_gate`` / ``xmc_ada_update``
(csrc/ada.hip).  Both are exact -- a select on a float64 comparison, integer counts, and five IEEE double operations in a fixed
order -- so the kernels are held to them bit for bit.  ``AdaController`` owns the persistent state in device memory and calls
the operator table's ``ada_gate`` and ``ada_update_rows``.  The signs are counted over logit rows, one per replica
(DESIGN.md 9f.3): ``update_rows`` is the specification of ``xmc_ada_update_rows``, bit-equal to ``xmc_ada_update`` with one row.
"""
from __future__ import annotations

import numpy as np

from . import diff_augment

# The largest p the controller reaches.  A policy default, not a measurement: the paper's argument is that the transforms stay
# invertible in distribution (and so do not leak into the generated images) while they are skipped with a probability that is
# safely above zero, and it takes p < 0.8 as that region.  The kernel takes the bound as an argument.
P_MAX = 0.8
PARTS = ("brightness", "saturation", "contrast", "translation", "cutout")
N_PARTS = len(PARTS)
PART_OF_COLUMN = (0, 1, 2, 3, 3, 4, 4, 4)          # the part that owns each of the eight columns of a plan row
STATE_WIDTH = 8                                    # [p, sign_sum, count, ticks, last_r, adjustments, 0, 0] as float64
P, SIGN_SUM, COUNT, TICKS, LAST_R, ADJUSTMENTS = range(6)
_GATE_STREAM = 0x6ADA                              # the extra seed word that keeps draw_gates apart from draw_plan


def target(config) -> float:
    """``config.ada_target`` (absent or 0 = off)"""
    return float(config.get("ada_target", 0.0) or 0.0)


def enabled(config) -> bool:
    return target(config) > 0.0


def settings(config):
    """-> dict(target, images_to_full, interval), validated; ValueError on a value outside its domain"""
    t = target(config)
    kimg, interval = float(config.get("ada_kimg", 500)), int(config.get("ada_interval", 4))
    if not 0.0 < t < 1.0:
        raise ValueError(f"config.ada_target must be in (0, 1) (r_t = E[sign(D(real))] never exceeds 1), got {t}")
    if not kimg > 0.0:
        raise ValueError(f"config.ada_kimg must be > 0, got {kimg}")
    if interval < 1:
        raise ValueError(f"config.ada_interval must be >= 1, got {interval}")
    return dict(target=t, images_to_full=kimg * 1000.0, interval=interval)


def check_config(config) -> None:
    """what ``create_train_state`` checks before it allocates anything: with ``ada_target`` > 0 the policy is not empty and the
    controller's settings are inside their domains"""
    if not enabled(config):
        if target(config) < 0.0:
            raise ValueError(f"config.ada_target must be in [0, 1), got {target(config)}")
        return
    if not diff_augment._parts(config.get("diff_augment", "")):
        raise ValueError("config.ada_target > 0 needs a non-empty config.diff_augment: the controller decides how often the "
                         "policy's parts are applied, and there is nothing to apply")
    settings(config)


def draw_gates(seed, step, rank, n) -> np.ndarray:
    """float32 ``[n, 2, 5]`` uniforms in [0, 1), multiples of 2^-24: one per sample, real (0) / generated (1) and part
    (``PARTS``).  A pure function of its arguments, on a ``SeedSequence`` of its own: ``draw_plan``'s numbers do not move."""
    ss = np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(rank), _GATE_STREAM])
    return np.random.default_rng(ss).random((int(n), 2, N_PARTS), dtype=np.float32)


def gate(plan, u, p) -> np.ndarray:
    """The specification of ``xmc_ada_gate``.  ``plan``: float32 [n, 2, 8], ``u``: float32 [n, 2, 5], ``p``: a double ->
    float32 rows [2n, 8], the n real rows first (the layout ``xmc_diffaug_fwd`` reads).  Part g of a row keeps the plan's values
    iff float64(u) < p (strict, compared in float64); otherwise its columns take their ``IDENTITY_ROW`` values."""
    plan, u = np.asarray(plan, np.float32), np.asarray(u, np.float32)
    n = plan.shape[0]
    if plan.shape != (n, 2, diff_augment.PLAN_WIDTH) or u.shape != (n, 2, N_PARTS):
        raise ValueError(f"ada.gate: plan must be (n, 2, 8) and u (n, 2, 5), got {plan.shape} and {u.shape}")
    on = (u.astype(np.float64) < np.float64(p))[..., list(PART_OF_COLUMN)]
    rows = np.where(on, plan, np.asarray(diff_augment.IDENTITY_ROW, np.float32))
    return np.ascontiguousarray(rows.transpose(1, 0, 2).reshape(2 * n, diff_augment.PLAN_WIDTH))


def initial_state() -> np.ndarray:
    return np.zeros((STATE_WIDTH,), np.float64)


def update(state, real_logits, target, images_to_full, interval, p_max) -> np.ndarray:
    """The specification of ``xmc_ada_update``: one half step of the controller.  ``state``: float64[8], ``real_logits``: the
    float32 logits of the REAL half.  Only finite logits count; a zero counts with sign 0.  All values but p and last_r are
    integers held exactly; the tail is IEEE double arithmetic in this order."""
    s = np.array(state, np.float64).reshape(STATE_WIDTH).copy()
    x = np.asarray(real_logits, np.float32).reshape(-1)
    finite = np.isfinite(x)
    s[SIGN_SUM] += float(int(np.count_nonzero(finite & (x > 0))) - int(np.count_nonzero(finite & (x < 0))))
    s[COUNT] += float(int(np.count_nonzero(finite)))
    s[TICKS] += 1.0
    if s[TICKS] >= float(int(interval)):
        if s[COUNT] > 0.0:
            r = s[SIGN_SUM] / s[COUNT]
            sgn = np.float64(float(r > target) - float(r < target))
            p = s[P] + sgn * (s[COUNT] / np.float64(images_to_full))
            p = np.float64(0.0) if p < 0.0 else p
            p = np.float64(p_max) if p > p_max else p
            s[P], s[LAST_R] = p, r
            s[ADJUSTMENTS] += 1.0
        s[SIGN_SUM] = s[COUNT] = s[TICKS] = 0.0
    return s


def update_rows(state, rows, b, target, images_to_full, interval, p_max) -> np.ndarray:
    """The specification of ``xmc_ada_update_rows``: the controller with data-parallel replicas.  ``rows``: float32 (w, 2b), the
    logit vectors [real; fake] of all w ranks in rank order.  Exactly ``update`` on the concatenation of the real halves
    ``rows[r, :b]`` in rank order -- the counts are integers, so every rank computes the same bits from the same rows.
    ``images_to_full`` counts GLOBAL images, as the paper's ``ada_kimg`` means."""
    rows, b = np.asarray(rows, np.float32), int(b)
    if rows.ndim != 2 or b < 1 or rows.shape[0] < 1 or rows.shape[1] != 2 * b:
        raise ValueError(f"ada.update_rows: rows must be (w, 2b) with w, b >= 1, got {rows.shape}, b = {b}")
    return update(state, rows[:, :b].reshape(-1), target, images_to_full, interval, p_max)


class AdaController:
    """The controller's persistent ``float64[8]`` state in device memory (outside the step's pool, so a captured step replays
    on it) and the two launches that use it.  On ``HipOps`` ``gate`` is ``xmc_ada_gate`` and ``update`` is
    ``xmc_ada_update_rows``: no host read, one graph launch per step stays true.  ``read`` is the only synchronisation."""

    def __init__(self, device, config=None, p_max=P_MAX):
        import torch
        self.state = torch.zeros((STATE_WIDTH,), dtype=torch.float64, device=device)
        self.p_max = float(p_max)
        self.settings = settings(config) if config is not None else None

    # ------------------------------------------------------------------------------------------------ device side
    def gate(self, ops, aug, u):
        """``aug``: the plan (B, 2, 8), ``u``: the uniforms (B, 2, 5), both float32 on the table's device -> rows (2B, 8)"""
        import torch
        return ops.ada_gate(aug.to(torch.float32).contiguous(), u.to(torch.float32).contiguous(), self.state)

    def update(self, ops, logit, b, replicas=None, rows=None):
        """one half step: ``logit`` is D's (2B,) float32 logit vector, whose first ``b`` entries are the real half.  ``replicas``
        (the step's ``dp.GradSync``, exclusive schedule): the signs are counted over the real halves of ALL ranks' logits
        (``dp.logit_rows``; ``rows``: already gathered), so every rank holds the same p.  Without: over the one row ``logit``"""
        from .. import dp
        if self.settings is None:
            raise ValueError("AdaController.update needs the controller's settings (built without a config)")
        s = self.settings
        rows, _ = dp.logit_rows(logit, b, replicas, rows)
        ops.ada_update_rows(rows, b, self.state, s["target"], s["images_to_full"], s["interval"], self.p_max)

    # -------------------------------------------------------------------------------------------------- host side
    def read(self):
        """-> dict(p, r_t = the r of the last adjustment, adjustments = how many there were).  A host synchronisation."""
        s = self.state.cpu().tolist()
        return dict(p=s[P], r_t=s[LAST_R], adjustments=int(s[ADJUSTMENTS]))

    def state_dict(self):
        return {"state": self.state.cpu().numpy().astype(np.float64)}

    def load_state_dict(self, d):
        import torch
        self.state.copy_(torch.from_numpy(np.asarray(d["state"], dtype=np.float64).reshape(STATE_WIDTH).copy()))
