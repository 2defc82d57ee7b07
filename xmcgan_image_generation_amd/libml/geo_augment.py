"""A specification of geometric augmentation for the discriminator's inputs: x-flip, quarter turns, isotropic scaling and
arbitrary rotation as ONE affine warp per image with zero-padded bilinear sampling -- the transform families Karras et al.,
"Training Generative Adversarial Networks with Limited Data" (NeurIPS 2020) found to carry most of ADA's benefit (DESIGN.md
9f.4).  Not part of the reference.

A SPECIFICATION ONLY: nothing in the training step, the configuration or the library uses this module.  There is no config key
and there are no device kernels.  It is written the way libml/diff_augment.py and libml/ada.py are written for their kernels,
so that a later change can add kernels and hold them to it.

The warp is linear in the image, so its adjoint needs no tape, only the matrix.  A *plan* (``draw_plan``: float32 [n, 2, 8],
columns ``[flip, k, s, cos, sin, 0, 0, 0]``, index 1 = real / generated) and one uniform per (sample, real / generated, part)
(``draw_gates``) are turned by ``compose`` into one row of eight float32 per image: the matrix M that maps centred destination
coordinates to centred source coordinates and N = M^-1, composed from the same parts (never a numeric inverse).  ``compose`` is
exact (selects and single IEEE double operations: a kernel can be bit-equal); ``apply`` / ``adjoint`` are float64, the adjoint in
gather form (one owner per source pixel, a bounded candidate box, no scatter).  ``apply_torch`` / ``adjoint_torch`` execute the
same rules in float32 on torch tensors.
"""
from __future__ import annotations

import numpy as np

PLAN_WIDTH = 8
ROW_WIDTH = 8
PARTS = ("xflip", "rot90", "scale", "rotate")
N_PARTS = len(PARTS)
IDENTITY_PLAN_ROW = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0)       # flip, k, s, cos, sin
IDENTITY_ROW = (1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0)            # m00 m01 m10 m11 n00 n01 n10 n11 (as values: m10 is -0.0)
DEFAULT_SCALE_STD = 0.2                                            # the paper's value, not tuned
S_MIN, S_MAX = 0.5, 2.0
K_LIM = 1 << 20                                                    # |k| is clamped here before it becomes an integer
BOX_MAX = 9                                                        # the adjoint's candidate box is at most BOX_MAX x BOX_MAX
_PLAN_STREAM, _GATE_STREAM = 0x6E0A, 0x6E0B                        # extra seed words: streams apart from diff_augment's and ada's


def _parts(policy):
    """the names of a policy string, validated -> tuple (empty for the empty policy)"""
    if policy is None or not str(policy).strip():
        return ()
    names = [p.strip() for p in str(policy).split(",")]
    if "" in names:
        raise ValueError(f"geo_augment: an empty name in {policy!r}; a policy is a comma-separated subset of {', '.join(PARTS)}")
    bad = [p for p in names if p not in PARTS]
    if bad:
        raise ValueError(f"geo_augment: unknown part {bad[0]!r} in {policy!r}; a policy is a comma-separated subset of "
                         f"{', '.join(PARTS)}")
    return tuple(dict.fromkeys(names))


def identity_plan(n: int) -> np.ndarray:
    """float32 [n, 2, 8] of ``IDENTITY_PLAN_ROW``"""
    return np.tile(np.asarray(IDENTITY_PLAN_ROW, np.float32), (int(n), 2, 1))


def draw_plan(seed, step, rank, n, policy, scale_std=DEFAULT_SCALE_STD) -> np.ndarray:
    """float32 ``[n, 2, 8]`` plan of ``n`` samples; index 1 is real (0) / generated (1), drawn independently.  A pure function of
    its arguments, on a ``SeedSequence`` of its own (``diff_augment.draw_plan`` and ``ada.draw_gates`` do not move).  Every part
    is always drawn, and the parts outside ``policy`` are then set to their identity value.
      flip in {0, 1}   k in {0, 1, 2, 3}   s = 2^g, g ~ N(0, scale_std^2), clipped to [0.5, 2]
      theta ~ U[-pi, pi): cos and sin in float64, each rounded once to float32"""
    parts = _parts(policy)
    n = int(n)
    ss = np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(rank), _PLAN_STREAM])
    rng = np.random.default_rng(ss)
    shape = (n, 2)
    flip = rng.integers(0, 2, shape)
    k = rng.integers(0, 4, shape)
    g = rng.standard_normal(shape) * np.float64(scale_std)
    theta = (rng.random(shape) * 2.0 - 1.0) * np.pi
    plan = identity_plan(n)
    if "xflip" in parts:
        plan[..., 0] = flip
    if "rot90" in parts:
        plan[..., 1] = k
    if "scale" in parts:
        plan[..., 2] = np.clip(np.exp2(g).astype(np.float32), np.float32(S_MIN), np.float32(S_MAX))
    if "rotate" in parts:
        plan[..., 3], plan[..., 4] = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32)
    return plan


def draw_gates(seed, step, rank, n) -> np.ndarray:
    """float32 ``[n, 2, 4]`` uniforms in [0, 1), multiples of 2^-24: one per sample, real (0) / generated (1) and part
    (``PARTS``).  A pure function of its arguments, on another stream word than ``draw_plan``."""
    ss = np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(rank), _GATE_STREAM])
    return np.random.default_rng(ss).random((int(n), 2, N_PARTS), dtype=np.float32)


def compose(plan, u, p) -> np.ndarray:
    """The specification of the rows (what a device kernel has to reproduce bit for bit).  ``plan``: float32 [n, 2, 8], ``u``:
    float32 [n, 2, 4], ``p``: a double -> float32 rows [2n, 8], the n real rows first: ``[m00, m01, m10, m11, n00, n01, n10, n11]``.

    What is read from the plan is made safe first (a replayed plan would reach a kernel unvalidated): flip is "non-zero", k is
    int(clamp(k, -2^20, 2^20)) & 3, s is clamped to [0.5, 2], cos and sin to [-1, 1]; a row with any non-finite value is the
    identity.  Part g keeps its value iff float64(u) < p (strict); otherwise it takes its identity value.  Then, in float64, every
    step one IEEE operation (no additions: nothing can contract):
        r = 1 / s;  a = r cos;  b = r sin;  A = [[a, b], [-b, a]]
        M = F Q^-k A      (Q^-1 A = rows (A1, -A0); F = diag(-1, 1) negates row 0)
        sc = s cos;  ss = s sin;  B = s R(theta) = [[sc, -ss], [ss, sc]]
        N = B Q^k F       (B Q = columns (B1, -B0); F negates column 0)
    Q = [[0, -1], [1, 0]] is the quarter turn.  Each of the eight values is rounded once to float32."""
    plan, u = np.asarray(plan, np.float32), np.asarray(u, np.float32)
    n = plan.shape[0]
    if plan.shape != (n, 2, PLAN_WIDTH) or u.shape != (n, 2, N_PARTS):
        raise ValueError(f"geo_augment.compose: plan must be (n, 2, 8) and u (n, 2, 4), got {plan.shape} and {u.shape}")
    ok = np.isfinite(plan).all(axis=-1)
    on = (u.astype(np.float64) < np.float64(p)) & ok[..., None]
    safe = np.where(ok[..., None], plan, np.float32(0.0))
    flip = (safe[..., 0] != 0) & on[..., 0]
    k = np.where(on[..., 1], np.clip(safe[..., 1], -K_LIM, K_LIM).astype(np.int64) & 3, 0)
    s = np.where(on[..., 2], np.clip(safe[..., 2], np.float32(S_MIN), np.float32(S_MAX)), np.float32(1.0)).astype(np.float64)
    c = np.where(on[..., 3], np.clip(safe[..., 3], np.float32(-1.0), np.float32(1.0)), np.float32(1.0)).astype(np.float64)
    sn = np.where(on[..., 3], np.clip(safe[..., 4], np.float32(-1.0), np.float32(1.0)), np.float32(0.0)).astype(np.float64)
    r = 1.0 / s
    a, b = r * c, r * sn
    a0, a1 = (a, b), (-b, a)                                      # the rows of A
    m0 = [np.select([k == 0, k == 1, k == 2], [a0[i], a1[i], -a0[i]], -a1[i]) for i in range(2)]
    m1 = [np.select([k == 0, k == 1, k == 2], [a1[i], -a0[i], -a1[i]], a0[i]) for i in range(2)]
    m0 = [np.where(flip, -v, v) for v in m0]
    sc, ss = s * c, s * sn
    b0, b1 = (sc, ss), (-ss, sc)                                  # the columns of B
    n0 = [np.select([k == 0, k == 1, k == 2], [b0[i], b1[i], -b0[i]], -b1[i]) for i in range(2)]
    n1 = [np.select([k == 0, k == 1, k == 2], [b1[i], -b0[i], -b1[i]], b0[i]) for i in range(2)]
    n0 = [np.where(flip, -v, v) for v in n0]
    rows = np.stack([m0[0], m0[1], m1[0], m1[1], n0[0], n1[0], n0[1], n1[1]], axis=-1).astype(np.float32)
    return np.ascontiguousarray(rows.transpose(1, 0, 2).reshape(2 * n, ROW_WIDTH))


def _source(rows, h, w, px, py):
    """float64 source coordinates (ux, uy) of the destination pixels (px, py) (broadcast against rows[:, None, None])"""
    m = np.asarray(rows, np.float64)
    m00, m01, m10, m11 = (m[:, i][:, None, None] for i in range(4))
    cx, cy = px + 0.5 - w / 2.0, py + 0.5 - h / 2.0
    return m00 * cx + m01 * cy + (w / 2.0 - 0.5), m10 * cx + m11 * cy + (h / 2.0 - 0.5)


def _weight(u, q):
    return np.maximum(0.0, 1.0 - np.abs(u - q))


def apply(x, rows) -> np.ndarray:
    """The specification of the warp in float64.  ``x``: [n, h, w, 3], ``rows``: [n, 8].  Per sample, with
    cx = x + 0.5 - w/2, cy = y + 0.5 - h/2:
        ux = m00 cx + m01 cy + (w/2 - 0.5),  uy = m10 cx + m11 cy + (h/2 - 0.5)
        out[y, x] = sum over the four integer neighbours q of (ux, uy) of w(ux, qx) w(uy, qy) src[q],  w(u, q) = max(0, 1 - |u - q|)
    and a neighbour outside the image reads 0: zero-padded bilinear sampling, continuous in u everywhere."""
    x = np.asarray(x, np.float64)
    n, h, w, _ = x.shape
    assert np.shape(rows) == (n, ROW_WIDTH)
    ux, uy = _source(rows, h, w, np.arange(w)[None, None, :], np.arange(h)[None, :, None])
    x0, y0 = np.floor(ux), np.floor(uy)
    out = np.zeros_like(x)
    idx = np.arange(n)[:, None, None]
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            wgt = _weight(uy, qy) * _weight(ux, qx)
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            v = x[idx, np.clip(qy, 0, h - 1).astype(np.int64), np.clip(qx, 0, w - 1).astype(np.int64)]
            out += np.where(inside, wgt, 0.0)[..., None] * v
    return out


def _box(rows, h, w):
    """the adjoint's candidate box of every source pixel -> (x_lo, nx, y_lo, ny), integer arrays [n, h, w].  Centred at
    N (q - o) + o with half-extents |n00| + |n01| + 0.5 and |n10| + |n11| + 0.5, clipped to the image (a destination pixel exists
    only there), at most ``BOX_MAX`` per side"""
    m = np.asarray(rows, np.float64)
    n00, n01, n10, n11 = (m[:, i][:, None, None] for i in range(4, 8))
    qcx, qcy = np.arange(w)[None, None, :] + 0.5 - w / 2.0, np.arange(h)[None, :, None] + 0.5 - h / 2.0
    bx, by = n00 * qcx + n01 * qcy + (w / 2.0 - 0.5), n10 * qcx + n11 * qcy + (h / 2.0 - 0.5)
    ex, ey = np.abs(n00) + np.abs(n01) + 0.5, np.abs(n10) + np.abs(n11) + 0.5
    x_lo, x_hi = np.clip(np.ceil(bx - ex), 0, w), np.clip(np.floor(bx + ex), -1, w - 1)
    y_lo, y_hi = np.clip(np.ceil(by - ey), 0, h), np.clip(np.floor(by + ey), -1, h - 1)
    nx, ny = np.minimum(x_hi - x_lo + 1, BOX_MAX), np.minimum(y_hi - y_lo + 1, BOX_MAX)
    return x_lo.astype(np.int64), nx.astype(np.int64), y_lo.astype(np.int64), ny.astype(np.int64)


def adjoint(g, rows) -> np.ndarray:
    """The specification of the pullback in float64: the exact transpose of ``apply``, in gather form.  For every source
    pixel q it adds w(ux(p), qx) w(uy(p), qy) g[p] over the destination pixels p of q's candidate box (``_box``) in row-major
    order of p.  The box is a superset of the pixels that read q; the weight decides membership."""
    g = np.asarray(g, np.float64)
    n, h, w, _ = g.shape
    assert np.shape(rows) == (n, ROW_WIDTH)
    x_lo, nx, y_lo, ny = _box(rows, h, w)
    qx, qy = np.arange(w)[None, None, :], np.arange(h)[None, :, None]
    out = np.zeros_like(g)
    idx = np.arange(n)[:, None, None]
    for dy in range(BOX_MAX):
        for dx in range(BOX_MAX):
            live = (dy < ny) & (dx < nx)
            if not live.any():
                continue
            px, py = np.clip(x_lo + dx, 0, w - 1), np.clip(y_lo + dy, 0, h - 1)
            ux, uy = _source(rows, h, w, px, py)
            wgt = np.where(live, _weight(uy, qy) * _weight(ux, qx), 0.0)
            out += np.where(wgt != 0.0, wgt, 0.0)[..., None] * np.where((wgt != 0.0)[..., None], g[idx, py, px], 0.0)
    return out


# ------------------------------------------------------------------------------------------------------ torch executors
def _torch_taps(rows, h, w):
    """float32 -> the four taps of every destination pixel: [(flat source index [n, h, w] (clamped), weight [n, h, w] (0
    outside the image))]"""
    import torch
    m = rows.to(torch.float32)
    m00, m01, m10, m11 = (m[:, i][:, None, None] for i in range(4))
    cx = (torch.arange(w, device=m.device, dtype=torch.float32) + 0.5 - w / 2.0)[None, None, :]
    cy = (torch.arange(h, device=m.device, dtype=torch.float32) + 0.5 - h / 2.0)[None, :, None]
    ux, uy = m00 * cx + (m01 * cy + (w / 2.0 - 0.5)), m10 * cx + (m11 * cy + (h / 2.0 - 0.5))
    x0, y0 = torch.floor(ux), torch.floor(uy)
    fx, fy = ux - x0, uy - y0
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            wgt = (fy if j else 1.0 - fy) * (fx if i else 1.0 - fx)
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            flat = qy.clamp(0, h - 1).long() * w + qx.clamp(0, w - 1).long()
            taps.append((flat, torch.where(inside, wgt, torch.zeros((), dtype=wgt.dtype, device=wgt.device))))
    return taps


def apply_torch(x, rows):
    """``apply`` on a torch tensor (CPU or device, float32 or bfloat16): float32 arithmetic, one rounding to ``x.dtype``;
    differentiable in ``x``.  With identity rows the result holds the values of ``x``."""
    import torch
    rows = torch.as_tensor(rows).to(x.device)
    n, h, w, c = x.shape
    assert tuple(rows.shape) == (n, ROW_WIDTH)
    src = x.float().reshape(n, h * w, c)
    out = None
    for flat, wgt in _torch_taps(rows, h, w):
        v = torch.gather(src, 1, flat.reshape(n, h * w, 1).expand(n, h * w, c)) * wgt.reshape(n, h * w, 1)
        out = v if out is None else out + v
    return out.reshape(n, h, w, c).to(x.dtype)


def adjoint_torch(g, rows):
    """``adjoint`` on a torch tensor: the transpose of ``apply_torch`` as four ``index_add_`` (float32 arithmetic, one rounding
    to ``g.dtype``; a fixed order on the CPU, where the operator tables without the kernel live)"""
    import torch
    rows = torch.as_tensor(rows).to(g.device)
    n, h, w, c = g.shape
    assert tuple(rows.shape) == (n, ROW_WIDTH)
    gf = g.float().reshape(n * h * w, c)
    out = torch.zeros_like(gf)
    base = (torch.arange(n, device=g.device) * (h * w))[:, None, None]
    for flat, wgt in _torch_taps(rows, h, w):
        out.index_add_(0, (flat + base).reshape(-1), gf * wgt.reshape(-1, 1))
    return out.reshape(n, h, w, c).to(g.dtype)
