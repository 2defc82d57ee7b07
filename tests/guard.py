"""Guard-band allocator for the kernel tests: every tensor a test (or ops.py on its behalf) allocates sits in the middle of its own
uint8 buffer whose every other byte is 0xFF -- NaN in float32 / bf16 / e4m3 / e8m0, -1 in the integer types.

* a store past either end of a buffer (an overhanging tile, a split-K slice at the wrong index, a workspace-size function that
  returns too little) changes a band byte: ``Guard.check()`` names the allocation and the distance of the damage from the tensor;
* a result that depends on the bytes next to an operand turns NaN and fails the float64 comparison the test already makes;
* ``skew`` moves every tensor to an address == skew (mod 512): 16 is the weakest pointer include/xmcgan_hip.h admits.

What it cannot see: a store that jumps further than the band, a read whose value is selected away (``cond ? x : 0``), and tensors
made by any other route than the patched functions (``torch.tensor(..., device=)``, ``clone``, arithmetic results).

A helper module, imported by tests; nothing is patched outside ``with guarded(g):``."""
import contextlib
import math
import os
import sys
from collections import namedtuple

import torch

_EMPTY = torch.empty                       # the real one, whatever is patched later
_HERE = os.path.abspath(__file__)
MIN_BAND = 64 << 10
MAX_BAND = 4 << 20

Damage = namedtuple("Damage", "shape dtype where side distance last count value")
Damage.__doc__ = """one damaged band.  ``side``: "after" / "before".  ``distance``: of the damaged byte NEAREST the tensor -- after: 0 is
the first byte past the tensor's end; before: -1 is the byte in front of its first.  ``last``: the same measure for the farthest
damaged byte, ``count``: damaged bytes in the band, ``value``: the nearest one's new value."""


class GuardError(AssertionError):
    def __init__(self, damage):
        self.damage = damage
        lines = [f"{d.side} {tuple(d.shape)} {d.dtype} allocated at {d.where}: {d.count} band byte(s) changed, nearest at distance "
                 f"{d.distance} (value 0x{d.value:02x}), farthest at {d.last}" for d in damage]
        super().__init__("guard band damaged:\n  " + "\n  ".join(lines))


def _caller():
    """file:line of the nearest frame outside this module"""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return f"{f.f_code.co_filename}:{f.f_lineno}" if f is not None else "?"


class Guard:
    def __init__(self, device, band=MIN_BAND, skew=0):
        assert band >= MIN_BAND and 0 <= skew < 512 and skew % 16 == 0
        self.device = torch.device(device)
        self.band, self.skew = band, skew
        self.recs = []                      # (base, off, nbytes, shape, dtype, where): strong references until check()
        self.fallthrough = []               # "function at file:line: why" of every request handed to the original function
        self.served = 0

    def mine(self, dev):
        if dev is None:
            return False
        dev = torch.device(dev)
        return dev.type == self.device.type and (dev.index is None or self.device.index is None or dev.index == self.device.index)

    def alloc(self, shape, dtype=None, fill=None):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        dtype = dtype or torch.get_default_dtype()
        n = math.prod(shape) * _EMPTY((), dtype=dtype).element_size()
        band = (max(self.band, min(n, MAX_BAND)) + 511) & ~511
        base = _EMPTY(n + 2 * band + 1024, dtype=torch.uint8, device=self.device)
        base.fill_(0xFF)
        off = band + (-(base.data_ptr() + band)) % 512 + self.skew
        t = base[off:off + n].view(dtype).view(shape)
        if fill is not None:
            t.fill_(fill)
        self.recs.append((base, off, n, shape, dtype, _caller()))
        self.served += 1
        return t

    def place(self, t):
        """guarded copy of an existing tensor (contiguous layout)"""
        g = self.alloc(tuple(t.shape), t.dtype)
        g.copy_(t)
        return g

    def damage(self):
        """list of Damage; releases the buffers"""
        recs, self.recs = self.recs, []
        if not recs:
            return []
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        # 0xFF is the largest uint8: a band is intact iff its minimum is 255 -- one transfer for all of them
        mins = torch.stack([torch.stack((base[:off].min(), base[off + n:].min())) for base, off, n, *_ in recs]).cpu()
        out = []
        for (base, off, n, shape, dtype, where), (lo_min, hi_min) in zip(recs, mins.tolist()):
            for side, band, bad in (("before", base[:off], lo_min != 0xFF), ("after", base[off + n:], hi_min != 0xFF)):
                if not bad:
                    continue
                idx = (band != 0xFF).nonzero().view(-1).cpu()
                near, far = (int(idx[0]), int(idx[-1])) if side == "after" else (int(idx[-1]) - off, int(idx[0]) - off)
                val = int(band[near if side == "after" else near + off])
                out.append(Damage(shape, dtype, where, side, near, far, int(idx.numel()), val))
        return out

    def check(self):
        """after a device synchronise every band byte must still be 0xFF"""
        bad = self.damage()
        if bad:
            raise GuardError(bad)


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        return tuple(size[0])
    return tuple(size)


@contextlib.contextmanager
def guarded(g):
    """inside: torch.empty / empty_like / zeros / zeros_like / full on the guard's device, and Tensor.cuda() / Tensor.to(device)
    of a CPU tensor, allocate through ``g.alloc``.  A request that cannot be served that way (keyword arguments beyond dtype /
    device, a non-contiguous model tensor) goes to the original function and is listed in ``g.fallthrough``."""
    T = torch.Tensor
    orig = dict(empty=torch.empty, empty_like=torch.empty_like, zeros=torch.zeros, zeros_like=torch.zeros_like, full=torch.full,
                cuda=T.cuda, to=T.to)
    own = {m: m in T.__dict__ for m in ("cuda", "to")}          # (inherited from the C base class: restored by deleting the override)

    def plain(k):
        k = dict(k)
        k.pop("dtype", None), k.pop("device", None)
        if k.get("requires_grad") is False:
            k.pop("requires_grad")
        return not k

    def miss(name, why):
        g.fallthrough.append(f"{name} at {_caller()}: {why}")

    def creator(name, fill):
        def f(*size, **k):
            if not g.mine(k.get("device")):
                return orig[name](*size, **k)
            if not plain(k):
                miss(name, f"keywords {sorted(k)}")
                return orig[name](*size, **k)
            return g.alloc(_shape_of(size), k.get("dtype"), fill)
        return f

    def like(name, fill):
        def f(t, **k):
            if not g.mine(k.get("device", t.device)):
                return orig[name](t, **k)
            if not plain(k) or not t.is_contiguous():
                miss(name, f"keywords {sorted(k)}" if not plain(k) else f"model tensor with strides {tuple(t.stride())}")
                return orig[name](t, **k)
            return g.alloc(tuple(t.shape), k.get("dtype") or t.dtype, fill)
        return f

    def full(size, fill_value, **k):
        if not g.mine(k.get("device")):
            return orig["full"](size, fill_value, **k)
        if not plain(k) or isinstance(fill_value, torch.Tensor):
            miss("full", f"keywords {sorted(k)}")
            return orig["full"](size, fill_value, **k)
        dtype = k.get("dtype")
        if dtype is None:
            dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else torch.get_default_dtype()
        return g.alloc(_shape_of((size,)), dtype, fill_value)

    def move(name, t, dtype=None):
        if not t.is_contiguous():
            miss(name, f"source with strides {tuple(t.stride())}")
            return None
        if t.requires_grad:
            miss(name, "source that requires grad")
            return None
        if dtype is not None and dtype != t.dtype:
            t = orig["to"](t, dtype)
        return g.place(t)

    def cuda(t, *a, **k):
        if t.device.type != "cpu" or g.device.type != "cuda" or a or k:
            if t.device.type == "cpu" and g.device.type == "cuda":
                miss("Tensor.cuda", "arguments")
            return orig["cuda"](t, *a, **k)
        out = move("Tensor.cuda", t)
        return out if out is not None else orig["cuda"](t)

    def to(t, *a, **k):
        dev, dtype, rest = k.get("device"), k.get("dtype"), [x for x in k if x not in ("device", "dtype")]
        pos = list(a)
        if pos and isinstance(pos[0], (str, torch.device)):
            dev = pos.pop(0)
        if pos and isinstance(pos[0], torch.dtype):
            dtype = pos.pop(0)
        if dev is None or t.device.type != "cpu" or not g.mine(dev) or g.device.type == "cpu":
            return orig["to"](t, *a, **k)
        if pos or rest:
            miss("Tensor.to", f"arguments {pos} {rest}")
            return orig["to"](t, *a, **k)
        out = move("Tensor.to", t, dtype)
        return out if out is not None else orig["to"](t, *a, **k)

    torch.empty, torch.zeros = creator("empty", None), creator("zeros", 0)
    torch.empty_like, torch.zeros_like = like("empty_like", None), like("zeros_like", 0)
    torch.full, T.cuda, T.to = full, cuda, to
    try:
        yield g
    finally:
        torch.empty, torch.empty_like, torch.zeros, torch.zeros_like = orig["empty"], orig["empty_like"], orig["zeros"], orig["zeros_like"]
        torch.full = orig["full"]
        for m in ("cuda", "to"):
            setattr(T, m, orig[m]) if own[m] else delattr(T, m)
