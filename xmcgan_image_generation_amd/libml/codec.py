"""Batches of images for the codec kernels (``include/xmc_codec.h``, ``libxmc_codec.so``): the arena layout both sides agree on
(``BatchLayout``), the device calls (``DeviceCodec``) and the same work in NumPy (``HostCodec``: the specifications of
``libml/jpeg.py`` and ``libml/png.py``), so that a caller picks one object and the bytes are the same either way.

There is no quiet fall-back: ``DeviceCodec`` raises when the library or the GPU is missing; ``HostCodec`` is asked for by name."""
from __future__ import annotations

import numpy as np

from . import jpeg, png

DESC_WORDS = 16
D_COEF, D_QT, D_PLANE, D_OUT, D_W, D_H, D_NCOMP, D_HS, D_VS, D_FILT, D_ROW = range(11)


def _up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


class BatchLayout:
    """Where each image of a batch lives in the arenas.  ``items``: per image ``(width, height, ncomp, hs, vs)`` (or
    ``jpeg.Info``).  ``desc``: int64 (n, 16), the table of include/xmc_codec.h.  Sizes: ``coef_elems`` (int16), ``qt_elems``
    (uint16), ``plane_bytes``, ``out_bytes`` (pixels), ``filt_bytes`` (filtered scanlines), ``rows``."""

    def __init__(self, items):
        items = [(i.width, i.height, i.ncomp, i.hs, i.vs) if isinstance(i, jpeg.Info) else tuple(int(v) for v in i) for i in items]
        if not items:
            raise ValueError("empty batch")
        self.items = items
        desc = np.zeros((len(items), DESC_WORDS), np.int64)
        coef = qt = plane = out = filt = rows = 0
        for k, (w, h, nc, hs, vs) in enumerate(items):
            if not (1 <= w <= jpeg.MAX_SIDE and 1 <= h <= jpeg.MAX_SIDE and w * h <= jpeg.MAX_PIXELS):
                raise ValueError(f"image {k}: size {w} x {h}")
            if (nc, hs, vs) not in ((1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)):
                raise ValueError(f"image {k}: {nc} components with luma sampling {hs} x {vs}")
            blocks = sum(bh * bw for bh, bw in jpeg.plane_blocks(nc, hs, vs, -(-w // (8 * hs)), -(-h // (8 * vs))))
            desc[k, :11] = (coef, qt, plane, out, w, h, nc, hs, vs, filt, rows)
            coef += blocks * 64
            qt += nc * 64
            plane += blocks * 64
            out = _up(out + 3 * w * h, 64)
            filt = _up(filt + h * (1 + 3 * w), 64)
            rows += h
        self.desc = desc
        self.coef_elems, self.qt_elems, self.plane_bytes, self.out_bytes, self.filt_bytes, self.rows = coef, qt, plane, out, filt, rows

    def __len__(self):
        return len(self.items)

    def coef_view(self, arena: np.ndarray, k: int) -> np.ndarray:
        end = self.desc[k + 1, D_COEF] if k + 1 < len(self) else self.coef_elems
        return arena[self.desc[k, D_COEF]:end]

    def qt_view(self, arena: np.ndarray, k: int) -> np.ndarray:
        return arena[self.desc[k, D_QT]:self.desc[k, D_QT] + 64 * self.items[k][2]]

    def image(self, out_arena: np.ndarray, k: int) -> np.ndarray:
        w, h = self.items[k][:2]
        o = int(self.desc[k, D_OUT])
        return out_arena[o:o + 3 * w * h].reshape(h, w, 3)

    def stream(self, filt_arena: np.ndarray, k: int) -> np.ndarray:
        w, h = self.items[k][:2]
        o = int(self.desc[k, D_FILT])
        return filt_arena[o:o + h * (1 + 3 * w)]


class HostCodec:
    """the specifications, batch by batch: what ``--no-device`` runs"""
    name = "host (NumPy specification)"

    def decode(self, coef: np.ndarray, qt: np.ndarray, layout: BatchLayout) -> np.ndarray:
        out = np.zeros(layout.out_bytes, np.uint8)
        for k, (w, h, nc, hs, vs) in enumerate(layout.items):
            layout.image(out, k)[...] = jpeg.decode_coefficients_np(layout.coef_view(coef, k), layout.qt_view(qt, k), w, h, nc, hs, vs)
        return out

    def filter(self, pixels: np.ndarray, layout: BatchLayout) -> np.ndarray:
        out = np.zeros(layout.filt_bytes, np.uint8)
        for k in range(len(layout)):
            layout.stream(out, k)[...] = png.filter_rows_np(layout.image(pixels, k))[0]
        return out

    def scanlines(self, coef, qt, layout):
        """host arenas -> the filtered-scanline arena, NumPy"""
        return self.filter(self.decode(coef, qt, layout), layout)


class DeviceCodec:
    """``xmc_jpeg_decode_batch`` / ``xmc_png_filter_batch`` on the current device and stream.  Arenas in and out are torch
    tensors on the device; ``scanlines`` takes and returns NumPy."""
    name = "device (libxmc_codec.so)"

    def __init__(self, device="cuda"):
        import torch
        from .. import _lib
        if not torch.cuda.is_available():
            raise _lib.XmcError("DeviceCodec needs a GPU; the NumPy specification is HostCodec (preprocess_data --no-device)")
        self.torch, self._lib, self.lib = torch, _lib, _lib.load_codec()
        self.device = torch.device(device)
        self._keep = []                     # (host table, event) of the calls in flight: the copy of the table is stream-ordered

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _hold(self, desc):
        """keep ``desc`` alive until the stream has passed the call just enqueued; forget the tables it has passed"""
        ev = self.torch.cuda.Event()
        ev.record(self.torch.cuda.current_stream(self.device))
        self._keep = [(d, e) for d, e in self._keep if not e.query()] + [(desc, ev)]

    def decode(self, coef, qt, layout: BatchLayout):
        """coef int16 (>= coef_elems,), qt uint16-as-int16 (>= qt_elems,): device tensors -> uint8 pixel arena (out_bytes,)"""
        torch, lib = self.torch, self.lib
        desc = np.ascontiguousarray(layout.desc)
        need = int(lib.xmc_jpeg_decode_workspace_bytes(desc.ctypes.data, len(layout)))
        if need <= 0:
            raise self._lib.XmcError(f"xmc_jpeg_decode_workspace_bytes: invalid table (rc={need})")
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(max(layout.out_bytes, 16), dtype=torch.uint8, device=self.device)
        self._lib.check(lib.xmc_jpeg_decode_batch(coef.data_ptr(), coef.numel(), qt.data_ptr(), qt.numel(), desc.ctypes.data,
                                                  len(layout), out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(),
                                                  self._stream()), "xmc_jpeg_decode_batch")
        self._hold(desc)
        return out

    def filter(self, pixels, layout: BatchLayout):
        """uint8 pixel arena (device) -> uint8 filtered-scanline arena (filt_bytes,)"""
        torch, lib = self.torch, self.lib
        desc = np.ascontiguousarray(layout.desc)
        need = int(lib.xmc_png_filter_workspace_bytes(desc.ctypes.data, len(layout)))
        if need <= 0:
            raise self._lib.XmcError(f"xmc_png_filter_workspace_bytes: invalid table (rc={need})")
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(max(layout.filt_bytes, 16), dtype=torch.uint8, device=self.device)
        self._lib.check(lib.xmc_png_filter_batch(pixels.data_ptr(), pixels.numel(), desc.ctypes.data, len(layout), out.data_ptr(),
                                                 out.numel(), ws.data_ptr(), ws.numel(), self._stream()), "xmc_png_filter_batch")
        self._hold(desc)
        return out

    def upload(self, coef: np.ndarray, qt: np.ndarray, layout: BatchLayout):
        torch = self.torch
        c = torch.from_numpy(np.ascontiguousarray(coef[:layout.coef_elems], np.int16)).to(self.device)
        q = torch.from_numpy(np.ascontiguousarray(qt[:layout.qt_elems]).view(np.int16)).to(self.device)
        return c, q

    def scanlines(self, coef: np.ndarray, qt: np.ndarray, layout: BatchLayout):
        """host arenas -> the filtered-scanline arena, NumPy: one decode call, one filter call, one copy back (the pixels
        stay on the device)"""
        c, q = self.upload(coef, qt, layout)
        st = self.filter(self.decode(c, q, layout), layout)
        return st.cpu().numpy()[:layout.filt_bytes]
