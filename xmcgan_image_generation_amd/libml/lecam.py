"""The LeCam discriminator regulariser (``config.lecam_weight``; Tseng et al., "Regularizing Generative Adversarial Networks under
Limited Data", CVPR 2021), with its two anchors kept in device memory.  Not part of the reference.

The term R = mean((D(real) - a_F)^2) + mean((D(fake) - a_R)^2) pulls D's real logits towards a moving average a_F of its GENERATED
logits and the generated ones towards the moving average a_R of the real ones.  lambda * R is added to D's objective: its whole
effect on the backward pass is ``dld += 2 * lambda / b * (logit - anchor)`` on the gradient the hinge launch has just written.
``d_loss`` keeps meaning hinge + contrastive; the unweighted R is reported under ``d_loss_lecam``.

This module is NumPy first: ``step`` is the written specification of ``xmc_lecam`` (csrc/lecam.hip).  It is IEEE double arithmetic
in a fixed order -- the sums included (``fixed_sum``) -- so the kernel is held to it bit for bit.  ``LecamController`` owns the
persistent state in device memory and calls the operator table's ``lecam_rows``.  R and the anchors come from logit rows, one per
replica: ``step_rows`` is the specification of ``xmc_lecam_rows``, bit-equal to ``xmc_lecam`` with one row.

``lecam_decay`` = 0.99 is the paper's decay as far as it can be recalled here, and 0.3 (CIFAR scale) / 0.01 (ImageNet scale) are its
weights: policy defaults, NOT tuned in this project.
"""
from __future__ import annotations

import math

import numpy as np

DECAY = 0.99
STATE_WIDTH = 8                                    # [anchor_real, anchor_fake, ticks, last_r, updates, 0, 0, 0] as float64
ANCHOR_REAL, ANCHOR_FAKE, TICKS, LAST_R, UPDATES = range(5)
LANES = 256                                        # the lanes of ``fixed_sum`` = the threads of the kernel's one workgroup
METRIC_KEY = "d_loss_lecam"
_QNAN64 = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]
_QNAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def weight(config) -> float:
    """``config.lecam_weight`` = lambda (absent or 0 = off)"""
    return float(config.get("lecam_weight", 0.0) or 0.0)


def enabled(config) -> bool:
    return weight(config) > 0.0


def settings(config):
    """-> dict(weight, decay, start, one_sided), validated; ValueError on a value outside its domain"""
    lam, decay = weight(config), float(config.get("lecam_decay", DECAY))
    start, one_sided = config.get("lecam_start", 0), bool(config.get("lecam_one_sided", False))
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"config.lecam_weight must be finite and >= 0, got {lam}")
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"config.lecam_decay must be in [0, 1), got {decay}")
    if int(start) != start or int(start) < 0:
        raise ValueError(f"config.lecam_start must be an integer >= 0 (half steps of warm-up), got {start}")
    return dict(weight=lam, decay=decay, start=int(start), one_sided=one_sided)


def check_config(config) -> None:
    """what ``create_train_state`` checks before it allocates anything: the four keys are inside their domains (a bad
    ``lecam_weight`` is an error even where it would read as "off")"""
    if any(k in config for k in ("lecam_weight", "lecam_decay", "lecam_start", "lecam_one_sided")):
        settings(config)


def fixed_sum(x) -> np.float64:
    """S: the fixed-order float64 sum the kernel computes.  Lane j of 256 adds elements j, j + 256, ... in rising order onto +0;
    then the tree v[j] += v[j + s] for s = 128 ... 1."""
    x = np.asarray(x, np.float64).reshape(-1)
    # (a lane's accumulator starts at +0 and is therefore never -0: adding the +0 padding changes no bit)
    rows = np.concatenate([x, np.zeros((-len(x)) % LANES, np.float64)]).reshape(-1, LANES)
    v = np.zeros((LANES,), np.float64)
    with np.errstate(all="ignore"):
        for row in rows:
            v = v + row
        s = LANES // 2
        while s >= 1:
            v[:s] = v[:s] + v[s:2 * s]
            s //= 2
    return v[0]


def initial_state() -> np.ndarray:
    return np.zeros((STATE_WIDTH,), np.float64)


def step(state, logit, b, dld, lam, decay, start, one_sided=False):
    """The specification of ``xmc_lecam``: one half step.  ``state``: float64[8]; ``logit``: D's float32 logits [real; fake],
    (2b,); ``dld``: the float32 (2b,) gradient the hinge launch wrote.  -> (new state, new dld, float32 R).  Everything is IEEE
    double in this order; a NaN that is WRITTEN (an element of dld, R) is the canonical quiet NaN (sign 0, payload 0), since IEEE
    leaves the payload of an operation's NaN result open."""
    s = np.array(state, np.float64).reshape(STATE_WIDTH).copy()
    b = int(b)
    x32 = np.asarray(logit, np.float32).reshape(-1)
    g32 = np.asarray(dld, np.float32).reshape(-1).copy()
    if b < 1 or x32.shape != (2 * b,) or g32.shape != (2 * b,):
        raise ValueError(f"lecam.step: logit and dld must be (2b,) with b >= 1, got {x32.shape}, {g32.shape}, b = {b}")
    x = x32.astype(np.float64)
    real, fake = x[:b], x[b:]
    a_r, a_f, ticks, updates = s[ANCHOR_REAL], s[ANCHOR_FAKE], s[TICKS], s[UPDATES]
    bb = np.float64(b)
    with np.errstate(all="ignore"):
        # 1. active test
        active = ticks >= np.float64(int(start)) and updates > 0.0
        # 2. penalty
        r = np.float64(0.0)
        if active:
            dr, df = real - a_f, fake - a_r
            if one_sided:                                  # relu(real - a_F) and -relu(a_R - fake): where the populations overlap
                dr, df = np.where(dr > 0.0, dr, 0.0), np.where(df < 0.0, df, 0.0)
            r = (fixed_sum(dr * dr) + fixed_sum(df * df)) / bb
            c = (np.float64(2.0) * np.float64(lam)) / bb
            new = (g32.astype(np.float64) + c * np.concatenate([dr, df])).astype(np.float32)
            g32 = np.where(np.isnan(new), _QNAN32, new)
            r = _QNAN64 if np.isnan(r) else r
        s[LAST_R] = r
        # 3. anchor update, from the anchors read above
        if bool(np.isfinite(x32).all()):
            m_r, m_f = fixed_sum(real) / bb, fixed_sum(fake) / bb
            g = np.float64(0.0) if (ticks < np.float64(int(start)) or updates == 0.0) else np.float64(decay)
            k = np.float64(1.0) - g
            s[ANCHOR_REAL] = g * a_r + k * m_r
            s[ANCHOR_FAKE] = g * a_f + k * m_f
            s[UPDATES] = updates + 1.0
        # 4. tick
        s[TICKS] = ticks + 1.0
        return s, g32, np.float32(r)


def step_rows(state, rows, rank, dld, lam, decay, start, one_sided=False):
    """The specification of ``xmc_lecam_rows``: one half step with data-parallel replicas.  ``rows``: float32 (w, 2b), the logit
    vectors [real; fake] of all w ranks in rank order; ``dld``: THIS rank's float32 (2b,) hinge gradient; ``rank``: its row.
    -> (new state, new dld, float32 R).  Steps 1 - 4 of ``step`` with X_R / X_F = the ranks' real / generated halves concatenated
    in rank order (w b elements each): R and the two means divide by w b, and "all finite" covers all w * 2b logits, so the state
    and R are the same bits on every rank.  Only this rank's gradient takes the term: c = (2 lam) / b with the LOCAL b and the
    d_i of row ``rank`` -- the optimiser's 1 / w gradient scale makes the ranks' sum the gradient of lam * R."""
    s = np.array(state, np.float64).reshape(STATE_WIDTH).copy()
    x32 = np.asarray(rows, np.float32)
    g32 = np.asarray(dld, np.float32).reshape(-1).copy()
    if x32.ndim != 2 or x32.shape[0] < 1 or x32.shape[1] < 2 or x32.shape[1] % 2:
        raise ValueError(f"lecam.step_rows: rows must be (w, 2b) with w, b >= 1, got {x32.shape}")
    w, b = x32.shape[0], x32.shape[1] // 2
    rank = int(rank)
    if not 0 <= rank < w or g32.shape != (2 * b,):
        raise ValueError(f"lecam.step_rows: rank must be in [0, {w}) and dld ({2 * b},), got {rank}, {g32.shape}")
    x = x32.astype(np.float64)
    real, fake = x[:, :b].reshape(-1), x[:, b:].reshape(-1)
    own = slice(rank * b, (rank + 1) * b)
    a_r, a_f, ticks, updates = s[ANCHOR_REAL], s[ANCHOR_FAKE], s[TICKS], s[UPDATES]
    bb, nn = np.float64(b), np.float64(w * b)
    with np.errstate(all="ignore"):
        # 1. active test
        active = ticks >= np.float64(int(start)) and updates > 0.0
        # 2. penalty
        r = np.float64(0.0)
        if active:
            dr, df = real - a_f, fake - a_r
            if one_sided:
                dr, df = np.where(dr > 0.0, dr, 0.0), np.where(df < 0.0, df, 0.0)
            r = (fixed_sum(dr * dr) + fixed_sum(df * df)) / nn
            c = (np.float64(2.0) * np.float64(lam)) / bb
            new = (g32.astype(np.float64) + c * np.concatenate([dr[own], df[own]])).astype(np.float32)
            g32 = np.where(np.isnan(new), _QNAN32, new)
            r = _QNAN64 if np.isnan(r) else r
        s[LAST_R] = r
        # 3. anchor update, from the anchors read above
        if bool(np.isfinite(x32).all()):
            m_r, m_f = fixed_sum(real) / nn, fixed_sum(fake) / nn
            g = np.float64(0.0) if (ticks < np.float64(int(start)) or updates == 0.0) else np.float64(decay)
            k = np.float64(1.0) - g
            s[ANCHOR_REAL] = g * a_r + k * m_r
            s[ANCHOR_FAKE] = g * a_f + k * m_f
            s[UPDATES] = updates + 1.0
        # 4. tick
        s[TICKS] = ticks + 1.0
        return s, g32, np.float32(r)


class LecamController:
    """The regulariser's persistent ``float64[8]`` state in device memory (outside the step's pool, so a captured step replays on
    it) and the one launch that uses it.  On ``HipOps`` ``apply`` is ``xmc_lecam_rows``: no host read, one graph launch per step
    stays true.  ``read`` is the only synchronisation."""

    def __init__(self, device, config=None):
        import torch
        self.state = torch.zeros((STATE_WIDTH,), dtype=torch.float64, device=device)
        self.settings = settings(config) if config is not None else None

    # ------------------------------------------------------------------------------------------------ device side
    def apply(self, ops, logit, dld, b, replicas=None, rows=None):
        """one half step: ``logit`` is D's (2B,) float32 logit vector [real; fake], ``dld`` the (2B,) float32 gradient the hinge
        launch has just written, which takes the term IN PLACE.  -> (1,) float32: the unweighted R.  ``replicas`` (the step's
        ``dp.GradSync``, exclusive schedule): R and the anchors come from ALL ranks' logits (``dp.logit_rows``; ``rows``:
        already gathered), so every rank holds the same anchors and reports the same R.  Without: from the one row ``logit``"""
        from .. import dp
        if self.settings is None:
            raise ValueError("LecamController.apply needs the controller's settings (built without a config)")
        s = self.settings
        rows, rank = dp.logit_rows(logit, b, replicas, rows)
        return ops.lecam_rows(rows, rank, dld, b, self.state, s["weight"], s["decay"], s["start"], s["one_sided"])

    # -------------------------------------------------------------------------------------------------- host side
    def read(self):
        """-> dict(anchor_real, anchor_fake, updates = anchor updates applied, ticks, last_r).  A host synchronisation."""
        s = self.state.cpu().tolist()
        return dict(anchor_real=s[ANCHOR_REAL], anchor_fake=s[ANCHOR_FAKE], updates=int(s[UPDATES]), ticks=int(s[TICKS]),
                    last_r=s[LAST_R])

    def state_dict(self):
        return {"state": self.state.cpu().numpy().astype(np.float64)}

    def load_state_dict(self, d):
        import torch
        self.state.copy_(torch.from_numpy(np.asarray(d["state"], dtype=np.float64).reshape(STATE_WIDTH).copy()))
