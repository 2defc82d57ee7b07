"""Times every stage of the dataset builder (xmcgan_image_generation_amd/preprocess_data.py) on synthetic JPEG files it
makes itself: 640 x 480, 4:2:0, quality 90, Huffman tables fitted to the data (what ``optimize=True`` writes).

    python tools/bench_jpeg.py [--images 1000] [--batch 64] [--out profiles/r19_preprocess.txt]

Stages, in images/s: entropy decode on one core and on the CPU budget (at most 16 processes), the two codec kernels (device
events, median of five after two warm-ups, with the bytes they move over the copy rate of profiles/r02_hbm_bw_probe.txt),
deflate + PNG wrapping, BERT, then the whole tool.  Pillow's full decode on the same files is timed for comparison when Pillow
is installed.  The encoder below is a plain baseline JPEG writer (float64 forward DCT, Annex K quantisation tables scaled as
libjpeg scales them); it exists so that the tool needs nothing but NumPy to make its input."""
import argparse
import heapq
import multiprocessing as mp
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_RATE = 5.2e12          # bytes/s, profiles/r02_hbm_bw_probe.txt

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                   100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] +
                    [99] * 32)
_C = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16) for u in range(8)] for x in range(8)])


def synth_image(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 37 + seed) * np.cos(y / 23), 255 * y / h, 128 + 90 * np.sin((x + y) / 51 + seed)], axis=-1)
    for _ in range(40):                                       # rectangles: edges off the block grid
        x0, y0 = rng.integers(0, w - 8), rng.integers(0, h - 8)
        img[y0:y0 + rng.integers(8, h // 3), x0:x0 + rng.integers(8, w // 3)] += rng.normal(0, 60, 3)
    img += rng.normal(0, 6, img.shape)                        # sensor-like noise keeps the high bands alive at quality 90
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _huffman_lengths(freq):
    """code lengths (<= 16) of the symbols with non-zero frequency; one code point stays free for the all-ones pattern"""
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freq.items()))] + [(0, len(freq), (-1,))]     # -1: the reserved point
    heapq.heapify(heap)
    depth = {s: 0 for s in list(freq) + [-1]}
    n = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        n += 1
        heapq.heappush(heap, (a[0] + b[0], n, a[2] + b[2]))
    counts = [0] * 64
    for s, d in depth.items():
        counts[max(d, 1)] += 1
    for i in range(63, 16, -1):                               # Annex K.3: move over-long codes up
        while counts[i] > 0:
            j = i - 2
            while counts[j] == 0:
                j -= 1
            counts[i] -= 2
            counts[i - 1] += 1
            counts[j + 1] += 2
            counts[j] -= 1
    i = 16
    while counts[i] == 0:
        i -= 1
    counts[i] -= 1                                            # the reserved point is the longest code
    order = sorted((s for s in depth if s != -1), key=lambda s: (depth[s], -freq[s], s))
    return counts[1:17], order


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for ln, c in enumerate(bits, 1):
        for _ in range(c):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def _size(v):
    return int(abs(int(v))).bit_length()


def encode_jpeg(img):
    """uint8 (H, W, 3) -> baseline JPEG bytes, 4:2:0, quality 90, fitted Huffman tables"""
    h, w, _ = img.shape
    f = img.astype(np.float64)
    yy = 0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]
    cb = 128 - 0.168736 * f[..., 0] - 0.331264 * f[..., 1] + 0.5 * f[..., 2]
    cr = 128 + 0.5 * f[..., 0] - 0.418688 * f[..., 1] - 0.081312 * f[..., 2]
    mx, my = -(-w // 16), -(-h // 16)

    def pad(p, ph, pw):
        return np.pad(p, ((0, ph - p.shape[0]), (0, pw - p.shape[1])), mode="edge")
    yy = pad(yy, my * 16, mx * 16)
    sub = [pad(p, my * 16, mx * 16).reshape(my * 8, 2, mx * 8, 2).mean(axis=(1, 3)) for p in (cb, cr)]
    scale = 200 - 2 * 90
    qts = [np.clip((q * scale + 50) // 100, 1, 255) for q in (Q_LUMA, Q_CHROMA)]
    planes = []
    for p, q in ((yy, qts[0]), (sub[0], qts[1]), (sub[1], qts[1])):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = (p - 128.0).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        coef = np.einsum("yv,abyx,xu->abvu", _C, blocks, _C)
        planes.append(np.rint(coef.reshape(bh, bw, 64) / q).astype(np.int64)[..., ZIGZAG])
    # the MCU-ordered block list: (table class, zigzagged block)
    seq = []
    for j in range(my):
        for i in range(mx):
            seq += [(0, 0, planes[0][2 * j + a, 2 * i + b]) for a in (0, 1) for b in (0, 1)]
            seq += [(1, 1, planes[1][j, i]), (1, 2, planes[2][j, i])]
    tokens, pred = [], [0, 0, 0]                              # (table id: 0/1 DC, 2/3 AC; symbol; extra bits; extra length)
    for cls, comp, blk in seq:
        d = int(blk[0]) - pred[comp]
        pred[comp] = int(blk[0])
        s = _size(d)
        tokens.append((cls, s, d if d >= 0 else d + (1 << s) - 1, s))
        nz = np.nonzero(blk[1:])[0] + 1
        last = 0
        for k in nz:
            run = int(k) - last - 1
            while run > 15:
                tokens.append((2 + cls, 0xF0, 0, 0))
                run -= 16
            v = int(blk[k])
            s = _size(v)
            tokens.append((2 + cls, (run << 4) | s, v if v >= 0 else v + (1 << s) - 1, s))
            last = int(k)
        if last < 63:
            tokens.append((2 + cls, 0, 0, 0))
    tables = []
    for t in range(4):
        freq = {}
        for tid, sym, _, _ in tokens:
            if tid == t:
                freq[sym] = freq.get(sym, 0) + 1
        bits, vals = _huffman_lengths(freq)
        tables.append((bits, vals, _codes(bits, vals)))
    parts = []
    for tid, sym, extra, n in tokens:
        code, ln = tables[tid][2][sym]
        parts.append(format(code, f"0{ln}b"))
        if n:
            parts.append(format(extra, f"0{n}b"))
    bitstr = "".join(parts)
    bitstr += "1" * (-len(bitstr) % 8)
    scan = int(bitstr, 2).to_bytes(len(bitstr) // 8, "big").replace(b"\xff", b"\xff\x00")

    def seg(marker, body):
        return b"\xff" + bytes([marker]) + struct.pack(">H", len(body) + 2) + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate(qts):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in q[ZIGZAG]))
    out += seg(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t, (bits, vals, _) in enumerate(tables):
        out += seg(0xC4, bytes([(t >> 1) << 4 | (t & 1)]) + bytes(bits) + bytes(vals))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out + scan + b"\xff\xd9"


# ----------------------------------------------------------------------------------------------------------- stages
def _entropy_worker(args):
    paths, reps = args
    from xmcgan_image_generation_amd.libml import jpeg
    datas = [open(p, "rb").read() for p in paths]
    t0 = time.perf_counter()
    for _ in range(reps):
        for d in datas:
            jpeg.coefficients(d)
    return time.perf_counter() - t0


def _pillow_worker(args):
    paths, reps = args
    import io
    from PIL import Image
    datas = [open(p, "rb").read() for p in paths]
    t0 = time.perf_counter()
    for _ in range(reps):
        for d in datas:
            np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))
    return time.perf_counter() - t0


def _parallel(worker, paths, reps, procs):
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(worker, [(paths[:1], 1)] * procs)                        # start-up and imports outside the clock
        t0 = time.perf_counter()
        pool.map(worker, [(paths, reps)] * procs)
        return procs * reps * len(paths) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=1000, help="images of the whole-tool run")
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic images (each takes about a second to encode)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from xmcgan_image_generation_amd import preprocess_data as P
    from xmcgan_image_generation_amd.libml import codec, input_pipeline, jpeg, png
    from xmcgan_image_generation_amd.utils import bert_arch, bert_utils
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    procs = max(1, min(16, int(input_pipeline.cpu_budget())))
    tmp = tempfile.mkdtemp(prefix="bench_jpeg_")
    images_dir = os.path.join(tmp, "images")
    os.makedirs(images_dir)
    base = [encode_jpeg(synth_image(a.width, a.height, s)) for s in range(a.distinct)]
    say(f"# bench_jpeg: {a.width} x {a.height}, 4:2:0, quality 90, fitted Huffman tables; {a.distinct} distinct images, "
        f"{sum(map(len, base)) / len(base) / 1024:.1f} KiB each; CPU budget {procs} processes")
    names = []
    for i in range(a.images):
        names.append(f"img_{i:06d}.jpg")
        with open(os.path.join(images_dir, names[-1]), "wb") as f:
            f.write(base[i % len(base)])
    paths = [os.path.join(images_dir, n) for n in names[:len(base)]]
    one = len(paths) * 3 / _entropy_worker((paths, 3))
    say(f"entropy decode, 1 core        {one:10.1f} images/s")
    say(f"entropy decode, {procs:2d} processes  {_parallel(_entropy_worker, paths, 6, procs):10.1f} images/s")
    try:
        import PIL                                                         # noqa: F401
        say(f"Pillow full decode, 1 core    {len(paths) * 3 / _pillow_worker((paths, 3)):10.1f} images/s")
        say(f"Pillow full decode, {procs:2d} procs  {_parallel(_pillow_worker, paths, 6, procs):10.1f} images/s")
    except ImportError:
        say("Pillow full decode            not installed here")
    # the kernels
    infos = [jpeg.coefficients(base[i % len(base)]) for i in range(a.batch)]
    layout = codec.BatchLayout([i[0] for i in infos])
    coef, qt = np.zeros(layout.coef_elems, np.int16), np.zeros(layout.qt_elems, np.uint16)
    for k, (_, c, q) in enumerate(infos):
        layout.coef_view(coef, k)[...] = c
        layout.qt_view(qt, k)[...] = q.reshape(-1)
    if torch.cuda.is_available():
        cod = codec.DeviceCodec()
        c, q = cod.upload(coef, qt, layout)

        def timed(fn):
            ts = []
            for i in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3)
            return float(np.median(ts[2:])), out
        t, px = timed(lambda: cod.decode(c, q, layout))
        pixels = a.batch * a.width * a.height
        moved = layout.coef_elems * 2 + 2 * layout.plane_bytes + 3 * pixels           # coefficients in, planes out and in, pixels out
        say(f"xmc_jpeg_decode_batch         {a.batch / t:10.1f} images/s  ({t * 1e6:.0f} us per batch of {a.batch}; {moved / pixels:.1f} B/pixel moved, "
            f"{moved / t / 1e12:.2f} TB/s = {100 * moved / t / HBM_COPY_RATE:.0f} % of the 5.2 TB/s copy rate)")
        t, st = timed(lambda: cod.filter(px, layout))
        moved = 2 * 3 * pixels + 3 * pixels + a.batch * a.height * 5                  # pixels read by both launches, stream out, ids
        say(f"xmc_png_filter_batch          {a.batch / t:10.1f} images/s  ({t * 1e6:.0f} us per batch of {a.batch}; {moved / pixels:.1f} B/pixel moved, "
            f"{moved / t / 1e12:.2f} TB/s = {100 * moved / t / HBM_COPY_RATE:.0f} % of the 5.2 TB/s copy rate)")
        st_host = st.cpu().numpy()
    else:
        say("xmc_jpeg_decode_batch         no GPU here")
        say("xmc_png_filter_batch          no GPU here")
        st_host = codec.HostCodec().scanlines(coef, qt, layout)
    streams = [layout.stream(st_host, k).tobytes() for k in range(min(8, a.batch))]
    t0 = time.perf_counter()
    sizes = [len(png.encode_filtered(s, a.height, a.width)) for s in streams]
    dt = (time.perf_counter() - t0) / len(streams)
    say(f"deflate + PNG chunks, 1 core  {1 / dt:10.1f} images/s  ({np.mean(sizes) / 1024:.0f} KiB per PNG; x {procs} processes = {procs / dt:.1f} if it scales)")
    vocab = os.path.join(ROOT, "tests", "golden", "bert_vocab_small.txt")
    if torch.cuda.is_available():
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            enc = bert_utils.TextEncoder(vocab, None)                       # BERT-base, random weights: the speed is the same
        caps = ["a man riding a horse on the beach with two dogs"] * (5 * a.batch)
        enc.get_bert_for_captions(caps, 17)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.get_bert_for_captions(caps, 17)
        torch.cuda.synchronize()
        say(f"BERT-base, 5 captions / image {a.batch / (time.perf_counter() - t0):10.1f} images/s  (embeddings copied back included)")
        records = [(n, ["a man riding a horse on the beach with two dogs"] * 5) for n in names]
        t0 = time.perf_counter()
        s = P.run(images_dir, records, os.path.join(tmp, "out"), enc, num_shards=10, batch=a.batch, procs=procs, log=lambda *_: None)
        dt = time.perf_counter() - t0
        say(f"whole tool, {a.images} images      {s['records'] / dt:10.1f} images/s  ({dt:.1f} s, {procs} worker processes, worker start-up included)")
    else:
        say("BERT-base / whole tool        no GPU here")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
