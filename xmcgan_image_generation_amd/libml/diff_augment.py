"""Differentiable augmentation of the discriminator's inputs (``config.diff_augment``; Zhao et al., "Differentiable Augmentation
for Data-Efficient GAN Training", NeurIPS 2020).  Not part of the reference: a remedy for a discriminator that memorises the real
images (``train_statistics`` shows the real logits drifting from the margin while recall falls).

The same random colour / translation / cutout transform is applied to every image the discriminator sees -- real and generated,
in both half steps -- and the generator's gradient is pulled back through it.  Per sample the transform is an affine map, so its
adjoint needs no tape, only the random parameters: the *plan*, drawn on the host (``draw_plan``) and carried in the batch under
``d_aug`` exactly like ``z``.

This module is NumPy first: ``apply`` / ``adjoint`` (float64) are the written specification of ``xmc_diffaug_fwd`` /
``xmc_diffaug_bwd`` (csrc/diff_augment.hip); ``apply_torch`` / ``adjoint_torch`` execute the same rules on torch tensors (CPU or
device) for operator tables without the kernel.

A plan row is eight float32: ``[b, s, k, ty, tx, y0, x0, c]`` -- brightness shift, saturation and contrast factors, the integer
translation, the origin and the side of the cutout box (integers stored as exact float32).  ``IDENTITY_ROW`` changes nothing.
"""
from __future__ import annotations

import numpy as np

PLAN_WIDTH = 8
IDENTITY_ROW = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
BRIGHTNESS, SATURATION, CONTRAST = 1, 2, 4           # flag bits of parse_policy (the ``flags`` argument of the kernels)
_PARTS = ("color", "translation", "cutout")
TRANSLATION_RATIO, CUTOUT_RATIO = 0.125, 0.5


def _parts(policy: str):
    """the names of a policy string, validated -> tuple (empty for the empty policy)"""
    if policy is None or not str(policy).strip():
        return ()
    names = [p.strip() for p in str(policy).split(",")]
    bad = [p for p in names if p not in _PARTS]
    if bad or not names:
        raise ValueError(f"diff_augment: unknown part {bad[0]!r} in {policy!r}; a policy is a comma-separated subset of "
                         f"{', '.join(_PARTS)}")
    return tuple(dict.fromkeys(names))


def parse_policy(policy: str) -> int:
    """``"color,translation,cutout"`` (any subset) -> the colour flags: bit 0 brightness, bit 1 saturation, bit 2 contrast
    (``color`` sets all three).  Translation and cutout need no flag: a zero shift / a box of side zero is an exact identity.
    An unknown name, or a non-empty policy in which nothing is recognised, raises ValueError; the empty policy gives 0."""
    parts = _parts(policy)
    return (BRIGHTNESS | SATURATION | CONTRAST) if "color" in parts else 0


def translation_range(size: int) -> int:
    return int(TRANSLATION_RATIO * size + 0.5)


def cutout_side(h: int) -> int:
    return int(CUTOUT_RATIO * h + 0.5)


def identity_plan(n: int) -> np.ndarray:
    """float32 [n, 2, 8] of ``IDENTITY_ROW``"""
    return np.tile(np.asarray(IDENTITY_ROW, np.float32), (int(n), 2, 1))


def draw_plan(seed, step, rank, n, h, w, policy) -> np.ndarray:
    """float32 ``[n, 2, 8]`` plan of ``n`` samples; index 1 is real (0) / generated (1), drawn independently.  A pure function of
    its arguments (``np.random.default_rng`` over a ``SeedSequence`` of seed, step and rank), so a resumed run draws what the
    uninterrupted one did.  Every part is always drawn -- switching one part on or off does not change the others' numbers --
    and the parts outside ``policy`` are then set to their identity value.
      b ~ U[-0.5, 0.5)   s ~ U[0, 2)   k ~ U[0.5, 1.5)
      ty, tx integers in [-r_h, r_h] x [-r_w, r_w], r = int(0.125 size + 0.5)
      c = int(0.5 h + 0.5);  y0 = cy - c // 2 with cy uniform in [0, h + 1 - c % 2), x0 likewise over w (both may be negative)"""
    parts = _parts(policy)
    n, h, w = int(n), int(h), int(w)
    ss = np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(rank)])
    rng = np.random.default_rng(ss)
    shape = (n, 2)
    u = rng.random((3,) + shape, dtype=np.float32)                  # multiples of 2^-24 in [0, 1)
    rh, rw = translation_range(h), translation_range(w)
    ty = rng.integers(-rh, rh + 1, shape)
    tx = rng.integers(-rw, rw + 1, shape)
    c = cutout_side(h)
    cy = rng.integers(0, h + 1 - c % 2, shape)
    cx = rng.integers(0, w + 1 - c % 2, shape)
    plan = identity_plan(n)
    if "color" in parts:
        plan[..., 0] = u[0] - np.float32(0.5)
        plan[..., 1] = u[1] * np.float32(2.0)
        # 0.5 + (1 - 2^-24) is a tie that rounds to 1.5 in float32: keep the interval half open
        plan[..., 2] = np.minimum(u[2] + np.float32(0.5), np.nextafter(np.float32(1.5), np.float32(0.0)))
    if "translation" in parts:
        plan[..., 3], plan[..., 4] = ty, tx
    if "cutout" in parts:
        plan[..., 5], plan[..., 6], plan[..., 7] = cy - c // 2, cx - c // 2, c
    return plan


def check_plan(plan_rows, h: int, w: int) -> None:
    """the checks the library makes on the host copy of a plan before it launches: ValueError otherwise"""
    p = np.asarray(plan_rows, np.float64)
    if p.ndim != 2 or p.shape[1] != PLAN_WIDTH or p.shape[0] < 1:
        raise ValueError(f"diff_augment: plan rows must be (n >= 1, {PLAN_WIDTH}), got shape {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError("diff_augment: a plan value is not finite")
    if (np.abs(p[:, 3]) >= h).any() or (np.abs(p[:, 4]) >= w).any():
        raise ValueError(f"diff_augment: a plan shift is outside the image ({h} x {w})")
    if (p[:, 7] < 0).any():
        raise ValueError("diff_augment: a plan cutout side is negative")


def _masks(plan_rows, h, w):
    """-> (ty, tx, box): integer shifts [n] and box[n, h, w] = pixel inside the cutout box"""
    p = np.asarray(plan_rows, np.float64)
    ty, tx, y0, x0, c = (p[:, i].astype(np.int64) for i in (3, 4, 5, 6, 7))
    ys, xs = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    box = ((ys >= y0[:, None, None]) & (ys < (y0 + c)[:, None, None])
           & (xs >= x0[:, None, None]) & (xs < (x0 + c)[:, None, None]))
    return ty, tx, box


def _shift(u, dy, dx):
    """y[n, p] = u[n, p - (dy, dx)[n]] where that pixel is inside the image, else 0 (u: [n, h, w, 3])"""
    n, h, w, _ = u.shape
    sy = np.arange(h)[None, :] - dy[:, None]
    sx = np.arange(w)[None, :] - dx[:, None]
    ok = ((sy >= 0) & (sy < h))[:, :, None] & ((sx >= 0) & (sx < w))[:, None, :]
    g = u[np.arange(n)[:, None, None], np.clip(sy, 0, h - 1)[:, :, None], np.clip(sx, 0, w - 1)[:, None, :]]
    return np.where(ok[..., None], g, 0.0)


def apply(x, plan_rows, flags: int) -> np.ndarray:
    """The specification of ``xmc_diffaug_fwd`` in float64.  ``x``: [n, h, w, 3], ``plan_rows``: [n, 8].  Per sample:
      1. u = x + b                                              (bit 0)
      2. m = mean_c(u);         u = (u - m) s + m               (bit 1)
      3. mu = mean_{h,w,c}(u);  u = (u - mu) k + mu             (bit 2)
      4. y[p] = u[p - t] if p - t is inside the image and p is outside the box [y0, y0 + c) x [x0, x0 + c), else 0
    mu = mean(x) + b: the saturation step keeps every pixel's channel mean, hence the image mean -- a kernel may therefore
    reduce ``x`` itself."""
    x = np.asarray(x, np.float64)
    p = np.asarray(plan_rows, np.float64)
    n, h, w, _ = x.shape
    assert p.shape == (n, PLAN_WIDTH)
    b, s, k = (p[:, i][:, None, None, None] for i in range(3))
    u = x
    if flags & BRIGHTNESS:
        u = u + b
    if flags & SATURATION:
        m = u.mean(axis=3, keepdims=True)
        u = (u - m) * s + m
    if flags & CONTRAST:
        mu = u.mean(axis=(1, 2, 3), keepdims=True)
        u = (u - mu) * k + mu
    ty, tx, box = _masks(p, h, w)
    return np.where(box[..., None], 0.0, _shift(u, ty, tx))


def adjoint(g, plan_rows, flags: int) -> np.ndarray:
    """The specification of ``xmc_diffaug_bwd`` in float64: the exact transpose of the linear part of ``apply``.
      1. h[q] = g[q + t] if that pixel is inside the image and outside the box, else 0
      2. h <- k h + (1 - k) mean_{h,w,c}(h)                     (bit 2)
      3. h <- s h + (1 - s) mean_c(h)                           (bit 1)
      4. brightness is the identity"""
    g = np.asarray(g, np.float64)
    p = np.asarray(plan_rows, np.float64)
    n, h, w, _ = g.shape
    assert p.shape == (n, PLAN_WIDTH)
    s, k = (p[:, i][:, None, None, None] for i in (1, 2))
    ty, tx, box = _masks(p, h, w)
    hh = _shift(np.where(box[..., None], 0.0, g), -ty, -tx)
    if flags & CONTRAST:
        hh = k * hh + (1.0 - k) * hh.mean(axis=(1, 2, 3), keepdims=True)
    if flags & SATURATION:
        hh = s * hh + (1.0 - s) * hh.mean(axis=3, keepdims=True)
    return hh


# ------------------------------------------------------------------------------------------------------ torch executors
def _torch_rows(plan_rows, device):
    import torch
    return torch.as_tensor(plan_rows).to(device=device, dtype=torch.float32)


def _torch_masks(p, h, w):
    import torch
    ty, tx, y0, x0, c = (p[:, i].long() for i in (3, 4, 5, 6, 7))
    ys = torch.arange(h, device=p.device)[None, :, None]
    xs = torch.arange(w, device=p.device)[None, None, :]
    box = ((ys >= y0[:, None, None]) & (ys < (y0 + c)[:, None, None])
           & (xs >= x0[:, None, None]) & (xs < (x0 + c)[:, None, None]))
    return ty, tx, box


def _torch_shift(u, dy, dx):
    import torch
    n, h, w, _ = u.shape
    sy = torch.arange(h, device=u.device)[None, :] - dy[:, None]
    sx = torch.arange(w, device=u.device)[None, :] - dx[:, None]
    ok = ((sy >= 0) & (sy < h))[:, :, None] & ((sx >= 0) & (sx < w))[:, None, :]
    g = u[torch.arange(n, device=u.device)[:, None, None], sy.clamp(0, h - 1)[:, :, None], sx.clamp(0, w - 1)[:, None, :]]
    return torch.where(ok[..., None], g, torch.zeros((), dtype=u.dtype, device=u.device))


def apply_torch(x, plan_rows, flags: int):
    """``apply`` on a torch tensor (CPU or device, float32 or bfloat16): float32 arithmetic, one rounding to ``x.dtype``;
    differentiable in ``x``.  With ``flags`` 0 and identity rows the result holds the bits of ``x``."""
    import torch
    p = _torch_rows(plan_rows, x.device)
    n, h, w, _ = x.shape
    assert p.shape == (n, PLAN_WIDTH)
    b, s, k = (p[:, i][:, None, None, None] for i in range(3))
    u = x.float()
    if flags & BRIGHTNESS:
        u = u + b
    if flags & SATURATION:
        m = u.mean(dim=3, keepdim=True)
        u = (u - m) * s + m
    if flags & CONTRAST:
        mu = u.mean(dim=(1, 2, 3), keepdim=True)
        u = (u - mu) * k + mu
    ty, tx, box = _torch_masks(p, h, w)
    y = torch.where(box[..., None], torch.zeros((), dtype=u.dtype, device=u.device), _torch_shift(u, ty, tx))
    return y.to(x.dtype)


def adjoint_torch(g, plan_rows, flags: int):
    """``adjoint`` on a torch tensor: float32 arithmetic, one rounding to ``g.dtype``"""
    import torch
    p = _torch_rows(plan_rows, g.device)
    n, h, w, _ = g.shape
    assert p.shape == (n, PLAN_WIDTH)
    s, k = (p[:, i][:, None, None, None] for i in (1, 2))
    ty, tx, box = _torch_masks(p, h, w)
    hh = _torch_shift(torch.where(box[..., None], torch.zeros((), dtype=torch.float32, device=g.device), g.float()), -ty, -tx)
    if flags & CONTRAST:
        hh = k * hh + (1.0 - k) * hh.mean(dim=(1, 2, 3), keepdim=True)
    if flags & SATURATION:
        hh = s * hh + (1.0 - s) * hh.mean(dim=3, keepdim=True)
    return hh.to(g.dtype)
