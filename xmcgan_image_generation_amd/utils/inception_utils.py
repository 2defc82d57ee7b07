"""Inception-v3 features, FID and Inception Score (the reference's ``xmcgan/utils/inception_utils.py`` and the NumPy metric
code of ``tf_inception_utils.py``).

``inception_model`` loads the network's ``{"params", "batch_stats"}`` -- the reference builds it from a Keras checkpoint
(``map_keras_variables_to_flax_dict``); this stack has no TensorFlow, so the converted Flax trees are read instead: the
``.npy`` pickle that ``pretrained_model_utils.get_pretrained_model`` reads, or a flax msgpack file.  Nothing is downloaded:
the user converts real weights once.  FID and IS computed with random weights (``checkpoint_path=None``) mean nothing.

``InceptionV3Features`` is ``get_inception`` (:102-130) on the HIP kernels: bilinear resize to 299 (``xmc_resize_bilinear``),
``clip(2x - 1, -1, 1)`` fused into the first convolution's gather, the 94 conv + folded-BatchNorm + ReLU blocks
(``xmc_inception_conv``, each branch written straight into its channel slice of the concatenation), the pools, the 8 x 8
mean (``xmc_mean_hw``), the 2048 -> 1000 head on ``ops.gemm`` and the softmax on the host.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import inception_arch as arch


def inception_model(checkpoint_path):
    """-> ``{"params", "batch_stats"}`` NumPy trees in the reference's flax layout.  ``checkpoint_path``: a ``.npy`` pickle of
    that dict or a flax msgpack file of it.  A path that does not exist raises ``FileNotFoundError``; ``None`` is the explicit
    opt-in to random weights (``inception_arch.init_inception``: tests and benchmarks -- FID from them means nothing)."""
    if checkpoint_path is None:
        params, stats = arch.init_inception(0)
        return {"params": params, "batch_stats": stats}
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"{checkpoint_path}: Inception-v3 checkpoint not found (convert the Keras InceptionV3 weights "
                                f"to {{'params', 'batch_stats'}} flax trees, .npy or msgpack; None = random weights)")
    with open(checkpoint_path, "rb") as f:
        data = f.read()
    if data[:6] == b"\x93NUMPY":
        tree = np.load(checkpoint_path, allow_pickle=True).item()
    else:
        from .checkpoint import msgpack_restore
        tree = msgpack_restore(data)
    return {"params": tree["params"], "batch_stats": tree["batch_stats"]}


def fold_block(params, batch_stats, spec):
    """eval-mode BatchNorm folded into the convolution, in float64: (x - mean) * rsqrt(var + 1e-3) + bias (no scale: the
    reference's ``use_scale=False``; a ``scale`` leaf added by its Keras mapping is ignored).
    -> (w (cout, kh * kw, cin) float64, bias (cout,) float64)"""
    p, s = params[spec.name], batch_stats[spec.name]["BatchNorm_0"]
    k = np.asarray(p["Conv_0"]["kernel"], np.float64)
    assert k.shape == (spec.kh, spec.kw, spec.cin, spec.cout), (spec.name, k.shape)
    a = 1.0 / np.sqrt(np.asarray(s["var"], np.float64) + arch.BN_EPS)
    w = np.transpose(k, (3, 0, 1, 2)).reshape(spec.cout, spec.kh * spec.kw, spec.cin) * a[:, None, None]
    b = np.asarray(p["BatchNorm_0"]["bias"], np.float64) - np.asarray(s["mean"], np.float64) * a
    return w, b


def softmax(logits):
    z = np.asarray(logits, np.float64)
    z = np.exp(z - z.max(axis=1, keepdims=True))
    return z / z.sum(axis=1, keepdims=True)


class InceptionV3Features:
    """``images (N, H, W, 3)`` in [0, 1] -> ``(pool (N, 2048) float32, preds (N, 1000) float32)`` (NumPy).

    The network follows ``ops.dtype``: float32 (the reference's precision, the default of ``EvalMetric``) or bf16.
    Intermediate buffers are allocated once per (chunk size, input size) and reused by every later call of that shape; the
    forward issues 94 conv launches, 4 max pools, 9 average pools, no concatenation and no copy kernel."""

    def __init__(self, ops, params, batch_stats):
        self.ops = ops
        dev, dt = ops.device, ops.dtype
        self.convs = []
        for spec in arch.CONVS:
            w, b = fold_block(params, batch_stats, spec)
            self.convs.append((spec, torch.as_tensor(w, dtype=torch.float32).to(dt).to(dev).contiguous(),
                               torch.as_tensor(b, dtype=torch.float32).to(dev).contiguous()))
        self.head_w = torch.as_tensor(np.asarray(params["Dense_0"]["kernel"], np.float32)).to(dev).contiguous()
        self.head_b = np.asarray(params["Dense_0"]["bias"], np.float64)
        self._bufs = {}

    def buffers(self, n, hs, ws):
        key = (n, hs, ws)
        bufs = self._bufs.get(key)
        if bufs is None:
            ops = self.ops
            bufs = {name: ops.empty((n,) + shape) for name, shape in arch.BUFFERS.items()}
            bufs["input"] = ops.empty((n, hs, ws, 3))
            bufs["pool"] = ops.empty((n, arch.POOL_DIM), torch.float32)
            bufs["logits"] = ops.empty((n, arch.NUM_CLASSES), torch.float32)
            self._bufs[key] = bufs
        return bufs

    def forward_device(self, images):
        """-> (pool, logits without the head's bias): float32 device tensors owned by this object (valid until the next call
        of the same shape)"""
        ops = self.ops
        n, hs, ws, c = images.shape
        assert c == 3
        bufs = self.buffers(n, hs, ws)
        x = images
        if not (isinstance(x, torch.Tensor) and x.device == bufs["input"].device and x.dtype == ops.dtype and x.is_contiguous()):
            x = bufs["input"]
            if isinstance(images, torch.Tensor) and images.device == x.device:
                x.copy_(images)                                               # (a cast of the caller's device images)
            else:                                                             # host -> device upload
                x.copy_(torch.as_tensor(np.asarray(images, np.float32)).to(ops.dtype))
        ops.inception_resize(x, bufs["image"])
        for step in arch.STEPS:
            if isinstance(step, arch.ConvSpec):
                spec, w, b = self.convs[step.index]
                ops.inception_conv(bufs[step.src], w, b, bufs[step.dst], kh=spec.kh, kw=spec.kw, stride=spec.stride, pad=spec.pad,
                                   y_off=step.dst_off, first=step.index == 0)
            elif step.kind == "max":
                ops.maxpool3x3s2_valid(bufs[step.src], bufs[step.dst], step.dst_off)
            else:
                ops.avgpool3x3_same(bufs[step.src], bufs[step.dst])
        ops.mean_hw(bufs[arch.OUTPUT], bufs["pool"])
        ops.gemm(bufs["pool"], self.head_w, out=bufs["logits"])
        return bufs["pool"], bufs["logits"]

    def __call__(self, images):
        pool, logits = self.forward_device(images)
        pool = pool.cpu().numpy().copy()
        preds = softmax(logits.cpu().numpy().astype(np.float64) + self.head_b[None, :]).astype(np.float32)
        return pool, preds


def calculate_fid(pool1, pool2):
    """The reference's FID (tf_inception_utils.py: means, ``np.cov(rowvar=False)``, Frechet distance) in float64.  The trace
    of sqrt(S1 S2) is the sum of sqrt(max(l, 0)) over the eigenvalues l of the symmetric S1^1/2 S2 S1^1/2 (``eigh``; no
    scipy): the same number as ``scipy.linalg.sqrtm``'s trace when S1 S2 is well conditioned.  Where the reference's sqrtm
    fails on a singular product it retries with 1e-6 added to both diagonals; here tiny negative eigenvalues (rounding of a
    singular product) are clipped to zero instead, so no retry is needed and no complex part can appear."""
    p1, p2 = np.asarray(pool1, np.float64), np.asarray(pool2, np.float64)
    mu1, mu2 = p1.mean(axis=0), p2.mean(axis=0)
    s1 = np.atleast_2d(np.cov(p1, rowvar=False))
    s2 = np.atleast_2d(np.cov(p2, rowvar=False))
    if mu1.shape != mu2.shape or s1.shape != s2.shape:
        raise ValueError("pool1 and pool2 have different feature sizes")
    lam, v = np.linalg.eigh(s1)
    r1 = (v * np.sqrt(np.maximum(lam, 0.0))) @ v.T
    m = r1 @ s2 @ r1
    mu = np.linalg.eigvalsh(0.5 * (m + m.T))
    tr_covmean = np.sqrt(np.maximum(mu, 0.0)).sum()
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * tr_covmean)


def calculate_inception_score(pred, num_splits=10):
    """The reference's Inception Score: ``num_splits`` chunks of ``N // num_splits`` predictions (the remainder dropped),
    exp(mean KL(p(y|x) || p(y))) per chunk -> (mean, std) over the chunks (float64)."""
    pred = np.asarray(pred, np.float64)
    k = pred.shape[0] // num_splits
    scores = []
    for i in range(num_splits):
        chunk = pred[i * k:(i + 1) * k]
        kl = chunk * (np.log(chunk) - np.log(np.mean(chunk, axis=0, keepdims=True)))
        scores.append(np.exp(np.mean(np.sum(kl, axis=1))))
    return float(np.mean(scores)), float(np.std(scores))
