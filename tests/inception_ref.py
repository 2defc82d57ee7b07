"""CPU restatement of the Inception-v3 feature network (torch CPU, float32 / float64) and a CPU operator table for
``inception_utils.InceptionV3Features``.

``forward`` is written straight from the reference's module structure (xmcgan/utils/inception_arch.py: the blocks in call
order, ``jnp.concatenate`` as ``torch.cat``, flax SAME / VALID padding, ``tensorflow_style_avg_pooling`` as
``avg_pool2d(count_include_pad=False)``) and reads the flax parameter trees directly, with the eval-mode BatchNorm
unfolded -- it shares nothing with the plan of ``inception_arch`` but the block names.  ``CpuInceptionOps`` implements the
operator methods the plan is run on (``inception_resize``, ``inception_conv``, ``maxpool3x3s2_valid``, ``avgpool3x3_same``,
``mean_hw``, ``gemm``), so the host logic of ``InceptionV3Features`` runs without a GPU; ``CountingOps`` counts its
launches.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def resize299(images, dtype=torch.float64):
    """jax.image.resize(..., (299, 299), "bilinear") for upsampling (or the identity): half-pixel centres, edge taps
    renormalised -- torch's align_corners=False bilinear"""
    x = torch.as_tensor(np.asarray(images) if not isinstance(images, torch.Tensor) else images).to(dtype).permute(0, 3, 1, 2)
    if x.shape[2] != 299 or x.shape[3] != 299:
        assert x.shape[2] <= 299 and x.shape[3] <= 299, "the restatement covers upsampling only"
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    return x                                                                       # NCHW


class _Net:
    def __init__(self, params, stats, dtype):
        self.p, self.s, self.dtype, self.i = params, stats, dtype, 0

    def block(self, x, cout, k, stride=1, padding="SAME"):
        name = f"ConvBatchNormReluBlock_{self.i}"
        self.i += 1
        p, s = self.p[name], self.s[name]["BatchNorm_0"]
        w = torch.as_tensor(np.asarray(p["Conv_0"]["kernel"])).to(self.dtype).permute(3, 2, 0, 1)     # OIHW
        assert tuple(w.shape) == (cout, x.shape[1]) + tuple(k), (name, tuple(w.shape))
        pad = ((k[0] - 1) // 2, (k[1] - 1) // 2) if padding == "SAME" else (0, 0)
        y = F.conv2d(x, w, stride=stride, padding=pad)
        t = lambda a: torch.as_tensor(np.asarray(a)).to(self.dtype)[None, :, None, None]     # noqa: E731
        y = (y - t(s["mean"])) * torch.rsqrt(t(s["var"]) + EPS) + t(p["BatchNorm_0"]["bias"])
        return torch.relu(y)


def _avg(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def _max(x):
    return F.max_pool2d(x, 3, 2)


def forward(params, stats, images, dtype=torch.float64, return_mixed=False):
    """images (N, H, W, 3) in [0, 1] -> (pool (N, 2048), logits (N, 1000)) in ``dtype``; ``return_mixed``: also the 11
    mixed-block outputs (NCHW)"""
    net, mixed = _Net(params, stats, dtype), []
    b = net.block
    x = torch.clamp(resize299(images, dtype) * 2 - 1, -1, 1)
    x = b(x, 32, (3, 3), 2, "VALID")
    x = b(x, 32, (3, 3), 1, "VALID")
    x = b(x, 64, (3, 3))
    x = _max(x)
    x = b(x, 80, (1, 1), 1, "VALID")
    x = b(x, 192, (3, 3), 1, "VALID")
    x = _max(x)
    for pool_features in (32, 64, 64):
        b1 = b(x, 64, (1, 1))
        b5 = b(b(x, 48, (1, 1)), 64, (5, 5))
        b3 = b(b(b(x, 64, (1, 1)), 96, (3, 3)), 96, (3, 3))
        bp = b(_avg(x), pool_features, (1, 1))
        x = torch.cat((b1, b5, b3, bp), 1)
        mixed.append(x)
    b3 = b(x, 384, (3, 3), 2, "VALID")
    bd = b(b(b(x, 64, (1, 1)), 96, (3, 3)), 96, (3, 3), 2, "VALID")
    x = torch.cat((b3, bd, _max(x)), 1)
    mixed.append(x)
    for c7 in (128, 160, 160, 192):
        b1 = b(x, 192, (1, 1))
        b7 = b(b(b(x, c7, (1, 1)), c7, (1, 7)), 192, (7, 1))
        bd = b(x, c7, (1, 1))
        bd = b(b(b(b(bd, c7, (7, 1)), c7, (1, 7)), c7, (7, 1)), 192, (1, 7))
        bp = b(_avg(x), 192, (1, 1))
        x = torch.cat((b1, b7, bd, bp), 1)
        mixed.append(x)
    b3 = b(b(x, 192, (1, 1)), 320, (3, 3), 2, "VALID")
    b7 = b(b(b(b(x, 192, (1, 1)), 192, (1, 7)), 192, (7, 1)), 192, (3, 3), 2, "VALID")
    x = torch.cat((b3, b7, _max(x)), 1)
    mixed.append(x)
    for _ in range(2):
        b1 = b(x, 320, (1, 1))
        t = b(x, 384, (1, 1))
        b3 = torch.cat((b(t, 384, (1, 3)), b(t, 384, (3, 1))), 1)
        t = b(b(x, 448, (1, 1)), 384, (3, 3))
        bd = torch.cat((b(t, 384, (1, 3)), b(t, 384, (3, 1))), 1)
        bp = b(_avg(x), 192, (1, 1))
        x = torch.cat((b1, b3, bd, bp), 1)
        mixed.append(x)
    assert net.i == 94
    pool = x.mean(dim=(2, 3))
    d = params["Dense_0"]
    logits = pool @ torch.as_tensor(np.asarray(d["kernel"])).to(dtype) + torch.as_tensor(np.asarray(d["bias"])).to(dtype)
    return (pool, logits, mixed) if return_mixed else (pool, logits)


def conv_ref(x, w, bias, *, kh, kw, stride=1, pad=(0, 0), relu=True, first=False, dtype=torch.float64):
    """xmc_inception_conv's math: x NHWC (its cin channels), w (cout, kh * kw, cin) -> NHWC in ``dtype``"""
    xc = x.to(dtype).permute(0, 3, 1, 2)
    if first:
        xc = torch.clamp(2 * xc - 1, -1, 1)
    cout, _, cin = w.shape
    wc = w.to(dtype).reshape(cout, kh, kw, cin).permute(0, 3, 1, 2)
    hi, wi = xc.shape[2], xc.shape[3]
    # explicit top / left padding; the bottom / right rows a window reaches past the input are zero as well
    y = F.conv2d(F.pad(xc, (pad[1], kw, pad[0], kh)), wc, stride=stride)
    ho = (hi + 2 * pad[0] - kh) // stride + 1
    wo = (wi + 2 * pad[1] - kw) // stride + 1
    y = y[:, :, :ho, :wo]
    if bias is not None:
        y = y + bias.to(dtype)[None, :, None, None]
    if relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1)


class CpuInceptionOps:
    """The operator methods of ``HipOps`` that ``InceptionV3Features`` uses, in torch on the CPU (float32 / float64)."""

    name = "cpu-inception"

    def __init__(self, dtype=torch.float32):
        self.dtype, self.device = dtype, torch.device("cpu")

    def empty(self, shape, dtype=None):
        return torch.full(tuple(shape), float("nan"), dtype=dtype or self.dtype)

    def inception_resize(self, x, out):
        out.copy_(resize299(x, torch.float64).permute(0, 2, 3, 1).to(out.dtype))
        return out

    def inception_conv(self, x, w, bias, out, *, kh, kw, stride=1, pad=(0, 0), x_off=0, y_off=0, relu=True, first=False):
        cout, _, cin = w.shape
        y = conv_ref(x[..., x_off:x_off + cin], w, bias, kh=kh, kw=kw, stride=stride, pad=pad, relu=relu, first=first,
                     dtype=self.dtype)
        assert y.shape[1:3] == out.shape[1:3], (y.shape, out.shape)
        out[..., y_off:y_off + cout] = y.to(out.dtype)
        return out

    def maxpool3x3s2_valid(self, x, out, y_off=0):
        c = x.shape[3]
        out[..., y_off:y_off + c] = _max(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        return out

    def avgpool3x3_same(self, x, out):
        out.copy_(_avg(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))
        return out

    def mean_hw(self, x, out):
        out.copy_(x.to(torch.float64).mean(dim=(1, 2)).to(out.dtype))
        return out

    def gemm(self, a, b, *, out=None, beta=0.0, **kw):
        r = (a.to(torch.float64) @ b.to(torch.float64)).to(torch.float32)
        if out is None:
            return r
        out.copy_(r if beta == 0.0 else r + beta * out)
        return out


class CountingOps(CpuInceptionOps):
    """counts every operator call by name"""

    def __init__(self, dtype=torch.float32):
        super().__init__(dtype)
        self.calls = {}

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name in ("inception_resize", "inception_conv", "maxpool3x3s2_valid", "avgpool3x3_same", "mean_hw", "gemm"):
            calls = object.__getattribute__(self, "calls")

            def counted(*a, **k):
                calls[name] = calls.get(name, 0) + 1
                return attr(*a, **k)
            return counted
        return attr
