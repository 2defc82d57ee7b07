"""Text-image alignment scores over CLIP embeddings (``config.eval_extra_metrics`` ``"clip"``): CLIPScore and R-precision, and the
preprocessing that feeds the image tower.  This file is the NumPy float64 SPECIFICATION of ``xmc_clip_preprocess``,
``xmc_pair_cosine`` and ``xmc_rprecision_hits`` (``csrc/clip.hip``) and the host fallback: every public function takes an optional
``ops`` (a ``HipOps``) and runs its pass on the kernels when one is given, in NumPy otherwise.

* ``clip_score(img, txt) = mean_i 2.5 max(cos(img_i, txt_i), 0)`` (Hessel et al. 2021, "CLIPScore", w = 2.5).
* ``r_precision(img, txt, cand)``: the share of images i whose own caption ``txt[i]`` has a STRICTLY larger cosine with ``img[i]``
  than each of the candidate captions ``txt[cand[i, j]]`` (Xu et al. 2018 / XMC-GAN: 99 random mismatched captions, R = 1).  Strict:
  a candidate that duplicates the true caption ties with it and the row counts as a miss.
* ``draw_candidates(seed, n, c)``: per row c distinct indices != i.

Cosines: the float32 inputs are multiplied and added in float64; a zero row gives cosine 0.
"""
from __future__ import annotations

import math

import numpy as np

CLIP_SALT = 0x434C4950                 # "CLIP": the candidates of pass i come from SeedSequence([rng, i, CLIP_SALT])
CLIP_SCORE_WEIGHT = 2.5


# ------------------------------------------------------------------------------------------------------------- preprocessing
def keys_cubic(x, a=-0.5):
    """the Keys cubic convolution kernel (Pillow's ``bicubic_filter``)"""
    x = np.abs(np.asarray(x, np.float64))
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def cubic_coeffs(n_in: int, n_out: int):
    """Pillow's ``precompute_coeffs`` for ``BICUBIC``: -> (lo (n_out,), count (n_out,), weights (n_out, ksize) float64, zero past
    ``count``).  Output pixel o is centred at (o + 0.5) n_in / n_out; the support is 2 max(1, n_in / n_out) input pixels, the
    window is clipped to the image and the weights are normalised to sum to 1."""
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    lo, cnt, w = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, ksize), np.float64)
    for o in range(n_out):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        k = np.arange(xmax - xmin)
        ww = keys_cubic((k + xmin - center + 0.5) / fscale)
        lo[o], cnt[o] = xmin, xmax - xmin
        w[o, :xmax - xmin] = ww / ww.sum()
    return lo, cnt, w


def resize_matrix(n_in: int, n_out: int):
    """(n_out, n_in) float64: the resize along one axis as a matrix"""
    lo, cnt, w = cubic_coeffs(n_in, n_out)
    m = np.zeros((n_out, n_in), np.float64)
    for o in range(n_out):
        m[o, lo[o]:lo[o] + cnt[o]] = w[o, :cnt[o]]
    return m


def resize(images, size: int):
    """(n, H, W, 3) -> (n, size, size, 3) float64: the separable cubic resize"""
    x = np.asarray(images, np.float64)
    ry, rx = resize_matrix(x.shape[1], size), resize_matrix(x.shape[2], size)
    return np.einsum("yh,nhwc,xw->nyxc", ry, x, rx, optimize=True)


def patch_rows(x, patch: int):
    """(n, S, S, 3) -> (n (S / patch)^2, 3 patch^2): row = (image, patch row, patch column), column = (c, ky, kx) -- the order of
    the flattened patch-embedding weight (out, c, ky, kx)"""
    n, s, _, c = x.shape
    g = s // patch
    return x.reshape(n, g, patch, g, patch, c).transpose(0, 1, 3, 5, 2, 4).reshape(n * g * g, c * patch * patch)


def preprocess(images, size: int, patch: int, mean=None, std=None, ops=None):
    """(n, H, W, 3) in [0, 1], H = W -> the image tower's input: cubic resize to ``size``, ``(v - mean_c) / std_c``, patch rows.
    No uint8 round trip: OpenAI's preprocessing quantises the resized image to bytes, this one keeps the floats.  NumPy float64
    without ``ops``; with one, ``xmc_clip_preprocess`` (float32 device tensor)."""
    from . import clip_arch
    mean = clip_arch.IMAGE_MEAN if mean is None else mean
    std = clip_arch.IMAGE_STD if std is None else std
    if size % patch:
        raise ValueError(f"preprocess: size {size} is no multiple of the patch size {patch}")
    if ops is not None:
        import torch
        t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32))
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.float()
        return ops.clip_preprocess(t.to(ops.device).contiguous(), size, patch, mean, std)
    x = np.asarray(images, np.float64)
    if x.ndim != 4 or x.shape[1] != x.shape[2] or x.shape[3] != 3:
        raise ValueError(f"preprocess: images are (n, H, W, 3) with H = W, got {x.shape}")
    y = (resize(x, size) - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return patch_rows(y, patch)


# -------------------------------------------------------------------------------------------------------------------- scores
def _rows(a):
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"embeddings are (n, d), got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


def cosine_spec(a, b):
    """float64 cosines of paired rows (broadcasting over leading dims); 0 where a row is zero"""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    den = np.sqrt((a * a).sum(-1)) * np.sqrt((b * b).sum(-1))
    dot = (a * b).sum(-1)
    return np.where(den > 0.0, dot / np.where(den > 0.0, den, 1.0), 0.0)


def pair_cosine(a, b, ops=None):
    a, b = _rows(a), _rows(b)
    if a.shape != b.shape:
        raise ValueError(f"pair_cosine: {a.shape} against {b.shape}")
    return ops.pair_cosine(a, b) if ops is not None else cosine_spec(a, b)


def clip_score(img, txt, ops=None) -> float:
    """mean over the pairs of 2.5 max(cos, 0)"""
    return float(np.mean(CLIP_SCORE_WEIGHT * np.maximum(pair_cosine(img, txt, ops), 0.0)))


def check_indices(truth, cand, n, m):
    truth, cand = np.asarray(truth), np.asarray(cand)
    if truth.shape != (n,) or cand.ndim != 2 or cand.shape[0] != n or cand.shape[1] < 1:
        raise ValueError(f"r_precision: truth is (n,) and cand (n, c >= 1) for n = {n}, got {truth.shape} and {cand.shape}")
    if truth.dtype.kind not in "iu" or cand.dtype.kind not in "iu":
        raise ValueError("r_precision: integer indices")
    for what, idx in (("truth", truth), ("cand", cand)):
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= m):
            raise ValueError(f"r_precision: {what} holds an index outside [0, {m})")


def rprecision_margins(img, txt, truth, cand):
    """(n,) float64: cosine with the true caption minus the largest cosine with a candidate"""
    img, txt = _rows(img), _rows(txt)
    own = cosine_spec(img, txt[np.asarray(truth)])
    other = cosine_spec(img[:, None, :], txt[np.asarray(cand)])
    return own - other.max(axis=1)


def rprecision_hits(img, txt, truth, cand, ops=None):
    """(n,) bool: is image i's cosine with ``txt[truth[i]]`` strictly above its cosine with every ``txt[cand[i, j]]``"""
    img, txt = _rows(img), _rows(txt)
    check_indices(truth, cand, img.shape[0], txt.shape[0])
    if ops is not None:
        return ops.rprecision_hits(img, txt, truth, cand)
    return rprecision_margins(img, txt, truth, cand) > 0.0


def r_precision(img, txt, cand, ops=None) -> float:
    """the share of rows i whose caption ``txt[i]`` beats the candidates ``txt[cand[i]]`` (``img`` and ``txt`` are paired)"""
    img = _rows(img)
    return float(np.mean(rprecision_hits(img, txt, np.arange(img.shape[0], dtype=np.int64), cand, ops)))


def draw_candidates(seed, n: int, c: int = 99):
    """(n, min(c, n - 1)) int32: per row i, distinct indices != i from ``np.random.default_rng(SeedSequence(seed))`` (``seed``: a
    ``SeedSequence`` or what one is built from); every other row when n - 1 < c"""
    if n < 2 or c < 1:
        raise ValueError(f"draw_candidates: n = {n} rows leave no candidate (c = {c})")
    seq = seed if isinstance(seed, np.random.SeedSequence) else np.random.SeedSequence(seed)
    rng = np.random.default_rng(seq)
    if n - 1 <= c:
        other = np.arange(n - 1, dtype=np.int64)[None, :].repeat(n, 0)
    else:
        other = np.stack([rng.choice(n - 1, size=c, replace=False) for _ in range(n)])
    return (other + (other >= np.arange(n)[:, None])).astype(np.int32)          # skip the row's own index
