"""Data gradient of the CLIP image tower: the NumPy float64 SPECIFICATION of the four kernels of ``csrc/clip_grad.hip``
(``xmc_mha_attention_bwd``, ``xmc_ln_bwd_add``, ``xmc_bias_quick_gelu_bwd``, ``xmc_clip_preprocess_bwd``) and the fallback of
``clip_utils.ClipEncoder.image_backward`` on an operator table without them.  Each function is the pullback of its forward
twin's statement (``tests/clip_ref.py`` spells those out in torch; ``tests/test_clip_guidance.py`` compares the two through
autograd).  Nothing here is on the training hot path.
"""
from __future__ import annotations

import numpy as np

from . import alignment_metrics, clip_arch

HEAD_DIM = 64
GELU_ALPHA = 1.702


def _f64(a):
    return np.asarray(a, np.float64)


def attention_bwd(qkv, bias_qkv, lens, dctx, t, causal=False):
    """qkv (n t, 3h) WITHOUT its bias, dctx (n t, h) -> dqkv (n t, 3h): the pullback of ``softmax_j(q k^T / 8) v`` per (sequence,
    head) over the keys j < lens[i] (and j <= query row when ``causal``).  P is recomputed; dP = dctx v^T, dS = P o (dP -
    rowsum(P o dP)) / 8, dq = dS k, dk = dS^T q, dv = P^T dctx.  Masked keys get exactly 0."""
    qkv, dctx = _f64(qkv), _f64(dctx)
    rows, h3 = qkv.shape
    h, n = h3 // 3, rows // t
    heads = h // HEAD_DIM
    z = (qkv + _f64(bias_qkv)).reshape(n, t, 3, heads, HEAD_DIM)
    q, k, v = (z[:, :, i].transpose(0, 2, 1, 3) for i in range(3))                # (n, heads, t, 64)
    do = dctx.reshape(n, t, heads, HEAD_DIM).transpose(0, 2, 1, 3)
    live = (np.arange(t)[None, :] < np.asarray(lens).reshape(n, 1))[:, None, None, :]
    if causal:
        live = live & (np.arange(t)[None, :] <= np.arange(t)[:, None])[None, None]
    s = np.where(live, q @ k.transpose(0, 1, 3, 2) / 8.0, -np.inf)
    e = np.where(live, np.exp(s - s.max(-1, keepdims=True)), 0.0)
    p = e / e.sum(-1, keepdims=True)
    dp = do @ v.transpose(0, 1, 3, 2)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True)) / 8.0
    dq, dk, dv = ds @ k, ds.transpose(0, 1, 3, 2) @ q, p.transpose(0, 1, 3, 2) @ do
    out = np.stack([g.transpose(0, 2, 1, 3) for g in (dq, dk, dv)], axis=2)       # (n, t, 3, heads, 64)
    return out.reshape(rows, h3)


def ln_bwd(x, gamma, dy, eps=clip_arch.LN_EPS):
    """rows of y = LayerNorm(x) gamma + beta (biased variance): dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma"""
    x, g = _f64(x), _f64(dy) * _f64(gamma)
    d = x - x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    xhat = d * rstd
    return rstd * (g - g.mean(-1, keepdims=True) - xhat * (g * xhat).mean(-1, keepdims=True))


def ln_bwd_add(x, gamma, dy, dres=None, eps=clip_arch.LN_EPS, mode="rows", t=1, pos=None):
    """``xmc_ln_bwd_add`` with its three row maps.  "rows": x, dy, dres (rows, h).  "gather": x, dres (n t, h), dy (n, h) -- row 0
    of every sequence takes the pooled row's gradient, every other row 0 (+ dres).  "vision": x = the patch products
    (n (t - 1), h), pos (t, h), dy (n t, h) -> (n (t - 1), h): the class row's gradient is dropped."""
    x = _f64(x)
    rows, h = x.shape
    if mode == "rows":
        out = ln_bwd(x, gamma, dy, eps)
    elif mode == "gather":
        out = np.zeros((rows, h))
        out[::t] = ln_bwd(x[::t], gamma, dy, eps)
    elif mode == "vision":
        n = rows // (t - 1)
        full = x.reshape(n, t - 1, h) + _f64(pos)[1:]
        out = ln_bwd(full, gamma, _f64(dy).reshape(n, t, h)[:, 1:], eps).reshape(rows, h)
    else:
        raise ValueError(f"ln_bwd_add: unknown mode {mode!r}")
    return out + _f64(dres) if dres is not None else out


def bias_quick_gelu_bwd(x, bias, dy):
    """dv = dy (s + 1.702 v s (1 - s)), v = x + bias, s = sigmoid(1.702 v)"""
    v = _f64(x) + _f64(bias)
    s = 1.0 / (1.0 + np.exp(-GELU_ALPHA * v))
    return _f64(dy) * (s + GELU_ALPHA * v * s * (1.0 - s))


def patch_rows_adjoint(dpatches, n, size, patch):
    """(n g^2, 3 patch^2) -> (n, size, size, 3): ``alignment_metrics.patch_rows`` is a permutation; this is its inverse"""
    g = size // patch
    return _f64(dpatches).reshape(n, g, g, 3, patch, patch).transpose(0, 1, 4, 2, 5, 3).reshape(n, size, size, 3)


def preprocess_adjoint(dpatches, hw, size, patch, std=None):
    """the transpose of the linear part of ``alignment_metrics.preprocess`` (``xmc_clip_preprocess_bwd``): dpatches
    (n (size / patch)^2, 3 patch^2) -> (n, hw, hw, 3) float64, dX_c = R^T dY_c R / std_c with R = ``resize_matrix(hw, size)``"""
    if size % patch:
        raise ValueError(f"preprocess_adjoint: size {size} is no multiple of the patch size {patch}")
    std = clip_arch.IMAGE_STD if std is None else std
    g = size // patch
    d = _f64(dpatches)
    if d.ndim != 2 or d.shape[1] != 3 * patch * patch or d.shape[0] % (g * g):
        raise ValueError(f"preprocess_adjoint: patch rows are (n {g * g}, {3 * patch * patch}), got {d.shape}")
    dy = patch_rows_adjoint(d, d.shape[0] // (g * g), size, patch) / _f64(std)
    r = alignment_metrics.resize_matrix(hw, size)
    return np.einsum("yh,nyxc,xw->nhwc", r, dy, r, optimize=True)
