"""KID and improved precision / recall over two pools of features: the specification and the host path.

Definitions.

* **KID** (Binkowski et al. 2018): the unbiased estimate of MMD^2 with the kernel ``k(u, v) = (u.v / d + 1)^3``, averaged over
  ``subsets`` random subsets of ``m = min(subset_size, n_g, n_r)`` rows of each pool:
  ``sum_{p != q} k(x_p, x_q) / (m (m - 1)) + sum_{p != q} k(y_p, y_q) / (m (m - 1)) - 2 sum_{p, q} k(x_p, y_q) / m^2``.
* **Improved precision / recall** (Kynkaanniemi et al. 2019): a pool's manifold is the union of the balls around its rows whose
  radius is the distance to the row's k-th nearest OTHER row.  Precision is the share of generated rows inside the real manifold,
  recall the share of real rows inside the generated one.  "Other" is by index: a duplicate of a row is a neighbour at distance 0,
  so a row repeated more than k times has radius 0 -- and is still hit by its copies (``d2 <= radius``).

Everything here works on squared distances ``d2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b)`` and computes in float64, in row blocks of
at most 1024 rows: no n x m matrix is built.  The ``*_spec`` functions define the metrics; ``precision_recall`` and ``kid`` take
the device path (``xmc_knn_radii`` / ``xmc_ball_hits`` / ``xmc_poly3_sums``: fp32 dot products on the exact-fp32 MFMA, everything
after them in float64) when the operator table ``ops`` has the entry points, and the specification otherwise -- the pattern of
``libml/device_cache.execute_plan``.
"""
from __future__ import annotations

import numpy as np

BLOCK = 1024
KID_SALT = 0x4B4944          # "KID": the last word of the seed sequence of a pass's subsets (eval_metrics.calculate_metrics)


def _f64(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("a pool is an (n, d) array")
    return a


def _d2_block(a, na, b, nb):
    """(rows of a) x (rows of b) squared distances of one block pair"""
    return np.maximum(0.0, na[:, None] + nb[None, :] - 2.0 * (a @ b.T))


def knn_radii_spec(x, k):
    """(n,) float64: for row i the k-th smallest ``d2(x_i, x_j)`` over ``j != i`` (exclusion by index)"""
    x = _f64(x)
    n, k = x.shape[0], int(k)
    if k < 1 or n <= k:
        raise ValueError(f"knn_radii needs 1 <= k < n, got k={k}, n={n}")
    nx = np.einsum("ij,ij->i", x, x)
    out = np.empty((n,), np.float64)
    for r0 in range(0, n, BLOCK):
        r1 = min(n, r0 + BLOCK)
        best = np.full((r1 - r0, k), np.inf)                     # the k smallest so far, per row
        for c0 in range(0, n, BLOCK):
            c1 = min(n, c0 + BLOCK)
            d = _d2_block(x[r0:r1], nx[r0:r1], x[c0:c1], nx[c0:c1])
            lo, hi = max(r0, c0), min(r1, c1)
            if lo < hi:                                          # the pairs (i, i) of this block pair
                i = np.arange(lo, hi)
                d[i - r0, i - c0] = np.inf
            best = np.sort(np.concatenate([best, d], 1), 1)[:, :k]
        out[r0:r1] = best[:, k - 1]
    return out


def ball_hits_spec(a, b, radii_b):
    """(n,) bool: ``hit[i] = any_j d2(a_i, b_j) <= radii_b[j]``"""
    a, b, radii_b = _f64(a), _f64(b), np.asarray(radii_b, np.float64)
    if a.shape[1] != b.shape[1] or radii_b.shape != (b.shape[0],):
        raise ValueError("ball_hits: a (n, d), b (m, d), radii_b (m,)")
    na, nb = np.einsum("ij,ij->i", a, a), np.einsum("ij,ij->i", b, b)
    hit = np.zeros((a.shape[0],), bool)
    for r0 in range(0, a.shape[0], BLOCK):
        r1 = min(a.shape[0], r0 + BLOCK)
        for c0 in range(0, b.shape[0], BLOCK):
            c1 = min(b.shape[0], c0 + BLOCK)
            hit[r0:r1] |= (_d2_block(a[r0:r1], na[r0:r1], b[c0:c1], nb[c0:c1]) <= radii_b[None, c0:c1]).any(1)
    return hit


def precision_recall_spec(pool_g, pool_r, k=3):
    """-> (precision, recall)"""
    precision = float(np.mean(ball_hits_spec(pool_g, pool_r, knn_radii_spec(pool_r, k))))
    recall = float(np.mean(ball_hits_spec(pool_r, pool_g, knn_radii_spec(pool_g, k))))
    return precision, recall


def kid_subsets(n_g, n_r, subsets, subset_size, seed):
    """two int32 (subsets, m) index arrays, ``m = min(subset_size, n_g, n_r)``: each row is ``rng.choice(n, m, replace=False)`` of
    ONE ``default_rng(seed)``, drawn for g and then for r, subset by subset"""
    m = min(int(subset_size), int(n_g), int(n_r))
    if m < 2:
        raise ValueError(f"KID needs subsets of at least 2 rows, got m={m}")
    if int(subsets) < 1:
        raise ValueError("KID needs at least one subset")
    rng = np.random.default_rng(seed)
    gi, ri = np.empty((subsets, m), np.int32), np.empty((subsets, m), np.int32)
    for s in range(int(subsets)):
        gi[s] = rng.choice(int(n_g), m, replace=False)
        ri[s] = rng.choice(int(n_r), m, replace=False)
    return gi, ri


def _check_indices(idx, n, what):
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.dtype.kind not in "iu":
        raise ValueError(f"{what}: a (subsets, m) integer array")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise ValueError(f"{what}: an index outside [0, {n})")
    return idx


def poly3_sums_spec(x, xi, y, yi):
    """(subsets, 3) float64: per subset ``sum_{p != q} k(x[xi[p]], x[xi[q]])``, the same sum for y, and
    ``sum_{p, q} k(x[xi[p]], y[yi[q]])`` with ``k(u, v) = (u.v / d + 1)^3``"""
    x, y = _f64(x), _f64(y)
    xi, yi = _check_indices(xi, x.shape[0], "xi"), _check_indices(yi, y.shape[0], "yi")
    if x.shape[1] != y.shape[1] or xi.shape != yi.shape:
        raise ValueError("poly3_sums: pools of one width, index arrays of one shape")
    d, m = x.shape[1], xi.shape[1]

    def total(u, v, same):
        t = 0.0
        for r0 in range(0, m, BLOCK):
            r1 = min(m, r0 + BLOCK)
            for c0 in range(0, m, BLOCK):
                c1 = min(m, c0 + BLOCK)
                kk = (u[r0:r1] @ v[c0:c1].T / d + 1.0) ** 3
                lo, hi = max(r0, c0), min(r1, c1)
                if same and lo < hi:
                    i = np.arange(lo, hi)
                    kk[i - r0, i - c0] = 0.0
                t += float(kk.sum())
        return t

    out = np.empty((xi.shape[0], 3), np.float64)
    for s in range(xi.shape[0]):
        xs, ys = x[xi[s]], y[yi[s]]
        out[s] = total(xs, xs, True), total(ys, ys, True), total(xs, ys, False)
    return out


def kid_from_sums(sums, m):
    """-> (kid, per_subset): per subset ``sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2``; ``kid`` is their mean"""
    sums, m = np.asarray(sums, np.float64).reshape(-1, 3), int(m)
    if m < 2:
        raise ValueError("KID needs m >= 2")
    per = sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)
    return float(per.mean()), per


# ------------------------------------------------------------------------------------------------------------ dispatch
DEVICE_ENTRY_POINTS = ("knn_radii", "ball_hits", "poly3_sums")


def has_device_path(ops):
    return ops is not None and all(hasattr(ops, n) for n in DEVICE_ENTRY_POINTS)


def knn_radii(x, k, ops=None):
    return ops.knn_radii(x, k) if has_device_path(ops) else knn_radii_spec(x, k)


def ball_hits(a, b, radii_b, ops=None):
    return ops.ball_hits(a, b, radii_b) if has_device_path(ops) else ball_hits_spec(a, b, radii_b)


def precision_recall(pool_g, pool_r, k=3, ops=None, real_radii=None):
    """-> (precision, recall).  ``real_radii``: ``knn_radii(pool_r, k)`` of a real pool that does not change between calls"""
    if has_device_path(ops) and hasattr(ops, "sample_pool"):     # each pool is used three times: upload it once
        pool_g, pool_r = ops.sample_pool(pool_g), ops.sample_pool(pool_r)
    if real_radii is None:
        real_radii = knn_radii(pool_r, k, ops)
    precision = float(np.mean(ball_hits(pool_g, pool_r, real_radii, ops)))
    recall = float(np.mean(ball_hits(pool_r, pool_g, knn_radii(pool_g, k, ops), ops)))
    return precision, recall


def kid(pool_g, pool_r, subsets=100, subset_size=1000, seed=0, ops=None):
    """-> (kid, std over the subsets)"""
    gi, ri = kid_subsets(len(pool_g), len(pool_r), subsets, subset_size, seed)
    sums = ops.poly3_sums(pool_g, gi, pool_r, ri) if has_device_path(ops) else poly3_sums_spec(pool_g, gi, pool_r, ri)
    value, per = kid_from_sums(sums, gi.shape[1])
    return value, float(per.std())
