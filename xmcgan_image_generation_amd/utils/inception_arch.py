"""Inception-v3 layer table of the FID / Inception Score network (the reference's ``xmcgan/utils/inception_arch.py``).

The reference is a flax module: 94 ``ConvBatchNormReluBlock_{i}`` (conv without bias, BatchNorm with ``use_scale=False`` and
eps 1e-3, ReLU) named in call order, max pools, TF-style average pools, channel concatenations, the 8 x 8 spatial mean and
``Dense_0`` (2048 -> 1000).  Here the same network is a static PLAN: a list of steps over named NHWC buffers, in which every
branch of a concatenation writes straight into its channel slice of the block's output buffer (``ConvSpec.dst_off``).
``inception_utils.InceptionV3Features`` runs the plan on the HIP kernels; ``tests/inception_ref.py`` restates the network
with ``torch.cat`` and checks the plan against it.

Flax conventions held to: kernels HWIO ``(kh, kw, cin, cout)``; SAME at stride 1 pads ``(k - 1) // 2`` before (all kernels
are odd); every stride-2 layer and pool is VALID except the stride-1 SAME average pools.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np

IMAGE_SIZE = 299
BN_EPS = 1e-3
POOL_DIM = 2048
NUM_CLASSES = 1000
NUM_BLOCKS = 94


class ConvSpec(NamedTuple):
    index: int              # ConvBatchNormReluBlock_{index}
    src: str                # input buffer (all channels of it are read)
    dst: str                # output buffer
    dst_off: int            # first output channel inside dst
    cin: int
    cout: int
    kh: int
    kw: int
    stride: int
    padding: str            # "SAME" | "VALID"
    hi: int
    wi: int
    ho: int
    wo: int

    @property
    def name(self):
        return f"ConvBatchNormReluBlock_{self.index}"

    @property
    def pad(self) -> Tuple[int, int]:
        """(top, left) zero padding"""
        return ((self.kh - 1) // 2, (self.kw - 1) // 2) if self.padding == "SAME" else (0, 0)

    @property
    def macs(self) -> int:
        """multiply-adds per image"""
        return self.ho * self.wo * self.cout * self.kh * self.kw * self.cin

    @property
    def geometry(self) -> Tuple[int, int, int, int, int, int]:
        return (self.cin, self.cout, self.kh, self.kw, self.ho, self.wo)


class PoolSpec(NamedTuple):
    kind: str               # "max" (3x3 stride 2 VALID) | "avg" (3x3 stride 1 SAME, in-bounds divisor)
    src: str
    dst: str
    dst_off: int


class _Builder:
    def __init__(self):
        self.buffers: Dict[str, Tuple[int, int, int]] = {"image": (IMAGE_SIZE, IMAGE_SIZE, 3)}
        self.steps: List = []
        self.convs: List[ConvSpec] = []

    def new(self, name, h, w, c):
        assert name not in self.buffers, name
        self.buffers[name] = (h, w, c)
        return name

    def conv(self, src, cout, k, stride=1, padding="SAME", into=None):
        """-> the output buffer; ``into`` = (buffer, channel offset) writes into a concatenation"""
        hi, wi, cin = self.buffers[src]
        kh, kw = k
        if padding == "SAME":
            assert stride == 1 and kh % 2 == 1 and kw % 2 == 1
            ho, wo = hi, wi
        else:
            ho, wo = (hi - kh) // stride + 1, (wi - kw) // stride + 1
        i = len(self.convs)
        if into is None:
            dst, off = self.new(f"c{i}", ho, wo, cout), 0
        else:
            dst, off = into
            assert self.buffers[dst][:2] == (ho, wo) and off + cout <= self.buffers[dst][2], (dst, off, cout)
        spec = ConvSpec(i, src, dst, off, cin, cout, kh, kw, stride, padding, hi, wi, ho, wo)
        self.convs.append(spec)
        self.steps.append(spec)
        return dst

    def maxpool(self, src, into=None):
        hi, wi, c = self.buffers[src]
        ho, wo = (hi - 3) // 2 + 1, (wi - 3) // 2 + 1
        if into is None:
            dst, off = self.new(f"max_{src}", ho, wo, c), 0
        else:
            dst, off = into
            assert self.buffers[dst][:2] == (ho, wo)
        self.steps.append(PoolSpec("max", src, dst, off))
        return dst

    def avgpool(self, src):
        h, w, c = self.buffers[src]
        dst = self.new(f"avg_{src}", h, w, c)
        self.steps.append(PoolSpec("avg", src, dst, 0))
        return dst


def _build():
    b = _Builder()
    x = b.conv("image", 32, (3, 3), 2, "VALID")                 # 149
    x = b.conv(x, 32, (3, 3), 1, "VALID")                       # 147
    x = b.conv(x, 64, (3, 3))                                   # 147
    x = b.maxpool(x)                                            # 73
    x = b.conv(x, 80, (1, 1), 1, "VALID")
    x = b.conv(x, 192, (3, 3), 1, "VALID")                      # 71
    x = b.maxpool(x)                                            # 35

    def block_a(x, name, pool_features):                       # mixed0 .. mixed2: 64 + 64 + 96 + pool_features
        h, w, _ = b.buffers[x]
        out = b.new(name, h, w, 224 + pool_features)
        b.conv(x, 64, (1, 1), into=(out, 0))
        t = b.conv(x, 48, (1, 1))
        b.conv(t, 64, (5, 5), into=(out, 64))
        t = b.conv(x, 64, (1, 1))
        t = b.conv(t, 96, (3, 3))
        b.conv(t, 96, (3, 3), into=(out, 128))
        b.conv(b.avgpool(x), pool_features, (1, 1), into=(out, 224))
        return out

    x = block_a(x, "mixed0", 32)
    x = block_a(x, "mixed1", 64)
    x = block_a(x, "mixed2", 64)

    out = b.new("mixed3", 17, 17, 768)                          # 384 + 96 + 288
    b.conv(x, 384, (3, 3), 2, "VALID", into=(out, 0))
    t = b.conv(x, 64, (1, 1))
    t = b.conv(t, 96, (3, 3))
    b.conv(t, 96, (3, 3), 2, "VALID", into=(out, 384))
    b.maxpool(x, into=(out, 480))
    x = out

    def block_c(x, name, c7):                                   # mixed4 .. mixed7: 4 x 192
        out = b.new(name, 17, 17, 768)
        b.conv(x, 192, (1, 1), into=(out, 0))
        t = b.conv(x, c7, (1, 1))
        t = b.conv(t, c7, (1, 7))
        b.conv(t, 192, (7, 1), into=(out, 192))
        t = b.conv(x, c7, (1, 1))
        t = b.conv(t, c7, (7, 1))
        t = b.conv(t, c7, (1, 7))
        t = b.conv(t, c7, (7, 1))
        b.conv(t, 192, (1, 7), into=(out, 384))
        b.conv(b.avgpool(x), 192, (1, 1), into=(out, 576))
        return out

    x = block_c(x, "mixed4", 128)
    x = block_c(x, "mixed5", 160)
    x = block_c(x, "mixed6", 160)
    x = block_c(x, "mixed7", 192)

    out = b.new("mixed8", 8, 8, 1280)                           # 320 + 192 + 768
    t = b.conv(x, 192, (1, 1))
    b.conv(t, 320, (3, 3), 2, "VALID", into=(out, 0))
    t = b.conv(x, 192, (1, 1))
    t = b.conv(t, 192, (1, 7))
    t = b.conv(t, 192, (7, 1))
    b.conv(t, 192, (3, 3), 2, "VALID", into=(out, 320))
    b.maxpool(x, into=(out, 512))
    x = out

    def block_e(x, name):                                       # mixed9, mixed10: 320 + 2 x 384 + 2 x 384 + 192
        out = b.new(name, 8, 8, 2048)
        b.conv(x, 320, (1, 1), into=(out, 0))
        t = b.conv(x, 384, (1, 1))
        b.conv(t, 384, (1, 3), into=(out, 320))
        b.conv(t, 384, (3, 1), into=(out, 704))
        t = b.conv(x, 448, (1, 1))
        t = b.conv(t, 384, (3, 3))
        b.conv(t, 384, (1, 3), into=(out, 1088))
        b.conv(t, 384, (3, 1), into=(out, 1472))
        b.conv(b.avgpool(x), 192, (1, 1), into=(out, 1856))
        return out

    x = block_e(x, "mixed9")
    x = block_e(x, "mixed10")
    assert len(b.convs) == NUM_BLOCKS and b.buffers[x] == (8, 8, POOL_DIM)
    return b


_PLAN = _build()
CONVS: List[ConvSpec] = _PLAN.convs
STEPS: List = _PLAN.steps
BUFFERS: Dict[str, Tuple[int, int, int]] = _PLAN.buffers
OUTPUT = "mixed10"
MIXED = [f"mixed{i}" for i in range(11)]


def param_shapes():
    """-> (params, batch_stats) trees of shapes, in the reference's flax layout"""
    params, stats = {}, {}
    for c in CONVS:
        params[c.name] = {"Conv_0": {"kernel": (c.kh, c.kw, c.cin, c.cout)}, "BatchNorm_0": {"bias": (c.cout,)}}
        stats[c.name] = {"BatchNorm_0": {"mean": (c.cout,), "var": (c.cout,)}}
    params["Dense_0"] = {"kernel": (POOL_DIM, NUM_CLASSES), "bias": (NUM_CLASSES,)}
    return params, stats


def param_counts():
    """-> (trainable, bn_channels, total with the moving statistics)"""
    trainable = sum(c.kh * c.kw * c.cin * c.cout + c.cout for c in CONVS) + POOL_DIM * NUM_CLASSES + NUM_CLASSES
    bn = sum(c.cout for c in CONVS)
    return trainable, bn, trainable + 2 * bn


def macs_per_image(include_head=True):
    """algorithmic multiply-adds of one 299 x 299 image (convolutions + the dense head)"""
    return sum(c.macs for c in CONVS) + (POOL_DIM * NUM_CLASSES if include_head else 0)


def flops_per_image(include_head=True):
    return 2 * macs_per_image(include_head)


def geometries():
    """distinct conv geometries (cin, cout, kh, kw, ho, wo), first-use order"""
    return list(dict.fromkeys(c.geometry for c in CONVS))


def init_inception(seed=0):
    """Seeded random weights in the reference's layout.  He-normal kernels and BatchNorm statistics near the identity keep the
    activations O(1) through all 11 mixed blocks (no dead feature maps); a head of std 2 / sqrt(2048) spreads the logits
    enough that the softmax is far from uniform.  Meaningless as a FID network: tests and benchmarks only."""
    rng = np.random.default_rng(seed)
    params, stats = {}, {}
    for c in CONVS:
        fan_in = c.kh * c.kw * c.cin
        k = rng.standard_normal((c.kh, c.kw, c.cin, c.cout)).astype(np.float32) * np.float32(np.sqrt(2.0 / fan_in))
        params[c.name] = {"Conv_0": {"kernel": k},
                          "BatchNorm_0": {"bias": (0.1 * rng.standard_normal(c.cout)).astype(np.float32)}}
        stats[c.name] = {"BatchNorm_0": {"mean": (0.1 * rng.standard_normal(c.cout)).astype(np.float32),
                                         "var": rng.uniform(0.6, 1.4, c.cout).astype(np.float32)}}
    params["Dense_0"] = {"kernel": (rng.standard_normal((POOL_DIM, NUM_CLASSES)) * (2.0 / np.sqrt(POOL_DIM))).astype(np.float32),
                         "bias": (0.1 * rng.standard_normal(NUM_CLASSES)).astype(np.float32)}
    return params, stats
