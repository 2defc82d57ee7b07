"""Device-resident dataset cache (``config.device_dataset_cache``): decode and resize every record ONCE, keep the result in HBM and
build each batch with one HIP launch (``xmc_cache_gather``, csrc/dataset_cache.hip) from a plan of integers drawn on the host.

Per example only the resize is costly, and it is deterministic: ``xmc_resize_bilinear_rgb`` applies the left-right flip by
mirroring the output index, so everything random in ``COCODataset.preprocess`` -- the flip, the caption choice, the reflect-shift
and the flip of ``augmentation.augment`` -- is an index or a reflection of the unflipped resize.  ``plan_example`` draws those
integers (and ``z``) from the example's generator exactly as ``preprocess`` does, ``execute_plan`` applies them in NumPy (the
written specification of the kernel, and the host fallback), the kernel applies them on the device.  The batches are bit for bit
those of the host pipeline with ``procs=0`` for the same ``(config, data_rng, rank, world)``: the record order comes from the
same ``input_pipeline._records``, walking cache slots instead of record bytes.

Sizes (float32): COCO-2014 train at 128 px is 16.3 GB of images + 22.9 GB of captions; nothing is cached on disk, the cache is
refilled at process start.  ``DeviceDatasetCache`` refuses (``ValueError``) a cache above half of the device's memory or above what
is free; it never falls back to the host pipeline by itself.
"""
from __future__ import annotations

import collections
import time
from typing import Dict, Iterator

import numpy as np

from . import _io, augmentation, input_pipeline, tfrecord

PLAN_STRIDE = 8          # int32 per example: slot, caption, flip, aug_dy, aug_dx, aug_flip, 0, 0 (XMC_CACHE_PLAN_STRIDE)
AUG_PAD = 4              # augmentation.augment_shift's default padding, the one preprocess uses


def plan_example(rng, sentence_num: int, z_dim: int, image_hw: int, caption_max_len=None, return_text: bool = False):
    """-> ((caption, flip, aug_dy, aug_dx, aug_flip), z) of one example: the draws of ``COCODataset.preprocess(features, rng)``
    without the image.  Consumes ``rng`` exactly as ``preprocess`` does: four child generators (flip, sentence index, z, aug) from
    ``integers(0, 2**63-1, size=4)``, the aug one consumed as ``augmentation.augment`` does.  ``return_text``: the SHORTEST
    caption (``caption_max_len``: the record's integer lengths) replaces the drawn index, as in ``preprocess``."""
    if image_hw <= AUG_PAD:
        raise ValueError(f"image size {image_hw} must exceed the augmentation's reflect padding {AUG_PAD}")
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    s_flip, s_idx, s_z, s_aug = rng.integers(0, 2 ** 63 - 1, size=4).tolist()
    child = lambda s: np.random.Generator(np.random.PCG64(s))                  # noqa: E731  (= default_rng(s), minus its dispatch)
    flip = int(child(s_flip).random() < 0.5)
    dy, dx, aug_flip = augmentation.augment_shift_draws(child(s_aug), AUG_PAD)
    if return_text:                                  # the children are independent: the index draw need not happen
        idx = int(np.argsort(-np.asarray(caption_max_len), kind="stable")[-1])
    else:
        idx = int(child(s_idx).integers(0, sentence_num)) if sentence_num > 1 else 0
    z = child(s_z).standard_normal((z_dim,)).astype(np.float32)
    return (idx, flip, dy, dx, int(aug_flip)), z


def check_plan(plan: np.ndarray, slots: int, s: int, h: int, w: int, pad: int = AUG_PAD) -> None:
    """the checks of ``xmc_cache_plan_check``: raises ValueError on a plan that would index outside the cache"""
    plan = np.asarray(plan)
    if plan.ndim != 2 or plan.shape[1] != PLAN_STRIDE or plan.shape[0] < 1:
        raise ValueError(f"plan must be (n >= 1, {PLAN_STRIDE}) integers, got shape {plan.shape}")
    if not (h > pad and w > pad and pad >= 0):
        raise ValueError(f"image {h} x {w} must exceed the reflect padding {pad}")
    slot, cap, dy, dx = plan[:, 0], plan[:, 1], plan[:, 3], plan[:, 4]
    if slot.min() < 0 or slot.max() >= slots:
        raise ValueError(f"plan slot outside [0, {slots})")
    if cap.min() < 0 or cap.max() >= s:
        raise ValueError(f"plan caption outside [0, {s})")
    if min(dy.min(), dx.min()) < 0 or max(dy.max(), dx.max()) > 2 * pad:
        raise ValueError(f"plan shift outside [0, {2 * pad}]")


def _reflect(i, n):
    """np.pad(mode="reflect") index: r(i, L) = -i below 0, 2 (L - 1) - i from L on"""
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def execute_plan(img, emb, sent, mlen, plan, pad: int = AUG_PAD, with_aug: bool = True) -> Dict[str, np.ndarray]:
    """NumPy executor of a plan -- the specification of ``xmc_cache_gather``.  img (slots, H, W, 3) the resized UNFLIPPED images,
    emb (slots, S, T, E), sent (slots, S, E), mlen (slots, S); plan (N, 8) int: slot, caption, flip, aug_dy, aug_dx, aug_flip.
      image[n, y, x]     = img[slot, y, W-1-x if flip else x]
      image_aug[n, y, x] = image[n, r(y + aug_dy - pad, H), r((W-1-x if aug_flip else x) + aug_dx - pad, W)]
      embedding[n] = emb[slot, caption]; sentence_embedding[n] = sent[slot, caption]; max_len[n, 0] = mlen[slot, caption]"""
    plan = np.asarray(plan).astype(np.int64)
    slots, h, w = img.shape[:3]
    check_plan(plan, slots, emb.shape[1], h, w, pad)
    slot, cap, flip, dy, dx, aflip = (plan[:, k] for k in range(6))
    ys, xs = np.arange(h), np.arange(w)
    mirror = lambda on, x: np.where(on[:, None] != 0, w - 1 - x, x)                # noqa: E731
    out = {"image": img[slot[:, None, None], ys[None, :, None], mirror(flip, xs[None, :])[:, None, :]]}
    if with_aug:
        sy = _reflect(ys[None, :] + dy[:, None] - pad, h)                           # row of `image`
        sx = _reflect(mirror(aflip, xs[None, :]) + dx[:, None] - pad, w)            # column of `image`
        out["image_aug"] = img[slot[:, None, None], sy[:, :, None], mirror(flip, sx)[:, None, :]]
    out["embedding"] = emb[slot, cap]
    out["max_len"] = mlen[slot, cap][:, None]
    out["sentence_embedding"] = sent[slot, cap]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------- fill
def fill_examples(ds, files, starts, workers: int = 1):
    """the records of ``files`` in file order, decoded for the cache: ``slot`` (``starts[f]`` + position in file f), the resized
    UNFLIPPED image, the caption tables and the host-side fields.  ``parse_example`` + the C resize run on ``workers`` threads,
    ``2 * workers`` records ahead, results kept in order (the layout of ``input_pipeline._examples``)."""
    def decode(item):
        slot, rec = item
        f = ds.parse_example(rec)
        emb = f["caption/embedding"]
        max_len = f["caption/max_len"].astype(np.float32)[:, None]
        return dict(slot=slot, image=_io.resize_bilinear_rgb(f["image"], ds.image_size, False), emb=emb,
                    sent=emb.sum(axis=-2) / max_len,                 # preprocess's own expression on the whole (S, T, E) array
                    mlen=max_len[:, 0], max_len=f["caption/max_len"], text=f["caption/text"], filename=f["image/filename"])

    def items():
        for path, start in zip(files, starts):
            for k, rec in enumerate(tfrecord.read_records(path)):
                yield start + k, rec

    if workers <= 1:
        for item in items():
            yield decode(item)
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="xmc-fill") as pool:
        pending = collections.deque()
        for item in items():
            pending.append(pool.submit(decode, item))
            if len(pending) >= 2 * workers:
                yield pending.popleft().result()
        while pending:
            yield pending.popleft().result()


def fill_chunks(ds, files, starts, workers: int, chunk: int) -> Iterator[dict]:
    """``fill_examples`` in runs of up to ``chunk`` records: arrays of leading dimension ``chunk`` (``count`` rows valid) plus the
    host-side lists.  The arrays are REUSED from one chunk to the next: the consumer copies them out before it asks for more."""
    s, t, e = ds.embedding_shape
    size = ds.image_size
    buf = dict(slot=np.zeros((chunk,), np.int64), image=np.empty((chunk, size, size, 3), np.float32),
               emb=np.empty((chunk, s, t, e), np.float32), sent=np.empty((chunk, s, e), np.float32),
               mlen=np.empty((chunk, s), np.float32), max_len=np.zeros((chunk, s), np.int64))
    count, texts, names = 0, [], []
    for ex in fill_examples(ds, files, starts, workers):
        for k in buf:
            buf[k][count] = ex[k]
        texts.append(ex["text"])
        names.append(ex["filename"])
        count += 1
        if count == chunk:
            yield dict(buf, count=count, text=texts, filename=names)
            count, texts, names = 0, [], []
    if count:
        yield dict(buf, count=count, text=texts, filename=names)


# ------------------------------------------------------------------------------------------------------------- planner
# (one thread: building the seven NumPy generators of an example holds the GIL, so a thread pool does not scale -- measured)
def plan_batches(files, counts, seed, shuffle, shuffle_buffer, repeat, batch, s, z_dim, size, max_len=None, drop_remainder=True):
    """(plan (n, 8) int32, z (n, z_dim) float32) per batch of the stream.  ``counts``: path -> (first slot, records); ``max_len``
    (slots, S) integers: given for ``return_text`` (the shortest caption is taken)."""
    def read(path):
        start, count = counts[path]
        return iter(range(start, start + count))
    recs = input_pipeline._records(files, input_pipeline._record_seed(seed), shuffle, shuffle_buffer, repeat, read=read)

    def new():
        return np.zeros((batch, PLAN_STRIDE), np.int32), np.empty((batch, z_dim), np.float32)
    (plan, z), n = new(), 0
    for i, slot in recs:
        fields, z[n] = plan_example(np.random.default_rng(seed + [i]), s, z_dim, size, None if max_len is None else max_len[slot],
                                    max_len is not None)
        plan[n, 0] = slot
        plan[n, 1:6] = fields
        n += 1
        if n == batch:
            yield plan, z
            (plan, z), n = new(), 0
    if n and not drop_remainder:
        yield plan[:n], z[:n]


def _device_memory(device):
    """(free, total) bytes of the device the cache would live on; None for the host cache (no budget)"""
    if device is None:
        return None
    import torch
    return torch.cuda.mem_get_info(torch.device(device))


def check_budget(need: int, free: int, total: int, what: str = "device dataset cache") -> None:
    """the cache may take at most half of the device's memory, and no more than is free: ValueError with both numbers otherwise"""
    if need > total // 2 or need > free:
        raise ValueError(f"{what} needs {need} bytes ({need / 2 ** 30:.2f} GiB): more than half of the device's {total} bytes "
                         f"({total / 2 ** 30:.2f} GiB) or than the {free} bytes ({free / 2 ** 30:.2f} GiB) free; "
                         "lower the image size, shard over more ranks or set config.device_dataset_cache = False")


_ARRAYS = ("image", "emb", "sent", "mlen")


class DeviceDatasetCache:
    """Every record of ``files`` (this rank's shards of one split, sorted) decoded once and kept as four float32 arrays -- in
    device memory (``device`` set: torch tensors, batches by ``xmc_cache_gather``) or in host NumPy arrays (``device=None``:
    batches by ``execute_plan``).  Slot = position of the record in the concatenation of the files.  Integer ``max_len``, texts
    and file names stay in host lists.  ``workers`` / ``procs``: the fill's decode threads per process / worker processes
    (0: threads of this process), the layout of the host pipeline; ``chunk``: records per pinned staging upload (32 = 15 MB at
    128 px: a worker's four-slot shared-memory ring stays at 60 MB and is warm after its first pass)."""

    def __init__(self, ds, files, device=None, workers: int = 4, procs: int = 0, chunk: int = 32, reserved_bytes: int = 0):
        self.ds, self.files, self.device = ds, list(files), device
        self.s, self.t, self.e = ds.embedding_shape
        self.size = int(ds.image_size)
        if self.e % 4 != 0:
            raise ValueError(f"embedding dimension {self.e} must be a multiple of 4 (caption rows move as 16-byte vectors)")
        if self.size <= AUG_PAD:
            raise ValueError(f"image size {self.size} must exceed the augmentation's reflect padding {AUG_PAD}")
        counts = [tfrecord.count_records(f) for f in self.files]
        self.starts = [int(v) for v in np.concatenate([[0], np.cumsum(counts)[:-1]])]
        self.counts = dict(zip(self.files, zip(self.starts, counts)))
        self.slots = int(sum(counts))
        if self.slots < 1:
            raise ValueError(f"no records in {self.files[:3]}...")
        self.shapes = dict(image=(self.size, self.size, 3), emb=(self.s, self.t, self.e), sent=(self.s, self.e), mlen=(self.s,))
        self.nbytes = 4 * self.slots * sum(int(np.prod(v)) for v in self.shapes.values())
        mem = _device_memory(device)
        if mem is not None:                          # BEFORE anything is allocated
            check_budget(self.nbytes + int(reserved_bytes), int(mem[0]), int(mem[1]))
        self.max_len = np.zeros((self.slots, self.s), np.int64)
        self.texts, self.filenames = [None] * self.slots, [None] * self.slots
        self.fill_seconds = self.fill_first_seconds = self.first_chunk = None
        self._fill(max(1, int(workers)), int(procs), max(1, min(int(chunk), self.slots)))

    # ------------------------------------------------------------------------------------------------------------ fill
    def _chunks(self, workers, procs, chunk):
        if procs > 0:
            ds = self.ds
            ds_kw = dict(image_size=ds.image_size, z_dim=ds.z_dim, data_dtype=ds.data_dtype, data_dir=ds.data_dir,
                         coco_version=ds.coco_version, return_text=ds.return_text, return_filename=ds.return_filename)
            return input_pipeline._batches_mp(ds_kw, self.files, [0], False, 1, False, False, chunk, procs, workers,
                                              fill_starts=self.starts)
        return fill_chunks(self.ds, self.files, self.starts, workers, chunk)

    def _fill(self, workers, procs, chunk):
        t0 = time.perf_counter()
        seen = np.zeros((self.slots,), bool)
        if self.device is None:
            self.arrays = {k: np.empty((self.slots,) + self.shapes[k], np.float32) for k in _ARRAYS}
            stage = None
        else:
            import torch
            dev = torch.device(self.device)
            self.arrays = {k: torch.empty((self.slots,) + self.shapes[k], dtype=torch.float32, device=dev) for k in _ARRAYS}
            # two pinned staging sets: chunk c + 1 is copied in while chunk c's uploads are still queued
            stage = [{k: torch.empty((chunk,) + self.shapes[k], dtype=torch.float32).pin_memory() for k in _ARRAYS} for _ in range(2)]
            busy = [None, None]
            stream = torch.cuda.Stream(device=dev)
            stream.wait_stream(torch.cuda.current_stream(dev))
        chunks = self._chunks(workers, procs, chunk)
        try:
            for ci, ch in enumerate(chunks):
                n = int(ch["count"])
                if ci == 0:                                  # (threads or worker processes are up: what follows is the steady rate)
                    self.fill_first_seconds, self.first_chunk = time.perf_counter() - t0, n
                slots = np.array(ch["slot"][:n])
                if seen[slots].any():
                    raise RuntimeError("device dataset cache: a record was delivered twice during the fill")
                seen[slots] = True
                self.max_len[slots] = ch["max_len"][:n]
                for j, sl in enumerate(slots):
                    self.texts[sl], self.filenames[sl] = ch["text"][j], ch["filename"][j]
                # runs of consecutive slots: (first row of the chunk, rows, first slot)
                cut = [0] + [j for j in range(1, n) if slots[j] != slots[j - 1] + 1] + [n]
                runs = [(a, b - a, int(slots[a])) for a, b in zip(cut[:-1], cut[1:])]
                if stage is None:
                    for a, m, s0 in runs:
                        for k in _ARRAYS:
                            self.arrays[k][s0:s0 + m] = ch[k][a:a + m]
                else:
                    st = stage[ci % 2]
                    if busy[ci % 2] is not None:
                        busy[ci % 2].synchronize()           # the uploads that read this staging set are complete
                    for k in _ARRAYS:
                        st[k][:n].copy_(torch.from_numpy(ch[k][:n]))
                    with torch.cuda.stream(stream):
                        for a, m, s0 in runs:
                            for k in _ARRAYS:
                                self.arrays[k][s0:s0 + m].copy_(st[k][a:a + m], non_blocking=True)
                        busy[ci % 2] = torch.cuda.Event()
                        busy[ci % 2].record(stream)
                if isinstance(ch, input_pipeline.SlotBatch):
                    ch.release()                             # copied out: the worker may refill its slot
        finally:
            if hasattr(chunks, "close"):
                chunks.close()
        if stage is not None:
            stream.synchronize()
            torch.cuda.current_stream(dev).wait_stream(stream)
        if not seen.all():
            raise RuntimeError(f"device dataset cache: {int((~seen).sum())} of {self.slots} records never arrived during the fill")
        self.fill_seconds = time.perf_counter() - t0

    # ---------------------------------------------------------------------------------------------------------- batches
    def read_ids(self, path):
        """``read`` of ``input_pipeline._records``: the cache slots of a file's records, in file order"""
        start, count = self.counts[path]
        return iter(range(start, start + count))

    def plans(self, seed, shuffle: bool, shuffle_buffer: int, repeat: bool, batch: int, drop_remainder: bool = True):
        """host side of the stream: per batch ``dict(plan=(n, 8) int32, z=(n, z_dim) float32[, text][, filename])``, example i of
        the stream drawn from ``default_rng([*seed, i])`` -- the generator ``input_pipeline._examples`` gives ``preprocess``."""
        ds = self.ds
        for plan, z in plan_batches(self.files, self.counts, [int(v) for v in np.atleast_1d(seed)], shuffle, shuffle_buffer, repeat,
                                    batch, self.s, ds.z_dim, self.size, self.max_len if ds.return_text else None, drop_remainder):
            out = dict(plan=plan, z=z)
            if ds.return_text:
                out["text"] = [self.texts[slot][cap] for slot, cap in plan[:, :2].tolist()]
            if ds.return_filename:
                out["filename"] = [self.filenames[slot] for slot in plan[:, 0].tolist()]
            yield out

    def _assemble(self, arrays, p):
        """the batch dict in ``preprocess``'s key order"""
        out = {k: arrays[k] for k in ("image", "image_aug", "embedding", "max_len", "sentence_embedding")}
        for k in ("text", "filename"):
            if k in p:
                out[k] = p[k]
        out["z"] = arrays["z"]
        return out

    def gather_host(self, p) -> dict:
        """one batch of the host cache (``device=None``) from a ``plans`` item: the NumPy executor"""
        a = self.arrays
        out = execute_plan(a["image"], a["emb"], a["sent"], a["mlen"], p["plan"])
        out["z"] = np.array(p["z"])
        return self._assemble(out, p)

    def gather_device(self, plan_dev, plan_host: np.ndarray, with_aug: bool = True) -> dict:
        """one ``xmc_cache_gather`` launch on the current stream; ``plan_dev``: the device copy of ``plan_host`` ((n, 8) int32)"""
        from .. import ops
        a = self.arrays
        return ops.cache_gather(a["image"], a["emb"], a["sent"], a["mlen"], plan_dev, plan_host, AUG_PAD, with_aug)

    def batches(self, seed, shuffle: bool, shuffle_buffer: int, repeat: bool, batch: int, prefetch: int = 2):
        """the stream's iterator: device tensors produced ``prefetch`` batches ahead on a stream of their own when the cache is on
        a device, NumPy batches otherwise"""
        plans = self.plans(seed, shuffle, shuffle_buffer, repeat, batch)
        if self.device is None:
            return input_pipeline.Prefetcher((self.gather_host(p) for p in plans), prefetch, None)
        return CachePrefetcher(self, plans, prefetch, self.device, batch)


class CachePrefetcher(input_pipeline.Prefetcher):
    """``Prefetcher`` whose upload step is the gather: the background thread draws the plans, sends each (plan, z) through a ring
    of pinned buffers on a side stream, launches ``xmc_cache_gather`` there and records an event; ``Prefetcher.__next__`` hands the
    batch over with that event plus ``record_stream``.  A ring entry is rewritten only after the event of the batch that last used
    it has completed, so no queued copy ever reads a buffer that is being refilled."""

    def __init__(self, cache: DeviceDatasetCache, plans, depth: int, device, batch: int):
        import torch
        self._cache = cache
        self._ring = [dict(plan=torch.empty((batch, PLAN_STRIDE), dtype=torch.int32).pin_memory(),
                           z=torch.empty((batch, cache.ds.z_dim), dtype=torch.float32).pin_memory(), ev=None)
                      for _ in range(max(1, depth) + 2)]
        self._turn = 0
        self._stream = torch.cuda.Stream(device=torch.device(device))
        super().__init__(plans, depth, device)

    def _upload(self, p):
        import torch
        slot = self._ring[self._turn % len(self._ring)]
        self._turn += 1
        if slot["ev"] is not None:
            slot["ev"].synchronize()
        n = p["plan"].shape[0]
        plan_host = np.ascontiguousarray(p["plan"], dtype=np.int32)
        slot["plan"][:n].copy_(torch.from_numpy(plan_host))
        slot["z"][:n].copy_(torch.from_numpy(p["z"]))
        with torch.cuda.stream(self._stream):
            plan_dev = slot["plan"][:n].to(self._device, non_blocking=True)
            out = self._cache.gather_device(plan_dev, plan_host)
            out["z"] = slot["z"][:n].to(self._device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        slot["ev"] = ev
        return self._cache._assemble(out, p), ev
