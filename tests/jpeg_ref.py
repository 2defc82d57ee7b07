"""Helpers of the JPEG tests: the recorded fixtures (tests/golden/jpeg_fixtures.npz, made by make_jpeg_fixture.py with
Pillow) and the IDEAL decoder every integer decoder is measured against -- the same quantised coefficients, float64
throughout, no intermediate rounding or clamping, the same interpolation weights and the JFIF matrix."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_PATH = os.path.join(HERE, "golden", "jpeg_fixtures.npz")
REFUSED = ("cmyk_8x8",)


@functools.lru_cache(maxsize=None)
def _npz():
    z = np.load(FIXTURE_PATH)
    return {k: z[k] for k in z.files}


def names(decodable_only=True):
    return [str(n) for n in _npz()["names"] if not (decodable_only and str(n) in REFUSED)]


def groups():
    """sets of fixtures made from one image with one mode, quality and subsampling: they differ only in their entropy coding"""
    import json
    return json.loads(str(_npz()["groups"]))


def jpeg_bytes(name) -> bytes:
    return _npz()[name + ".jpg"].tobytes()


def pillow_pixels(name) -> np.ndarray:
    return _npz()[name + ".rgb"]


@functools.lru_cache(maxsize=None)
def decoded(name):
    """(Info, coefficients, tables, the specification's pixels): computed once, shared, never written to"""
    from xmcgan_image_generation_amd.libml import jpeg
    nfo, coef, qt = jpeg.coefficients(jpeg_bytes(name))
    px = jpeg.decode_coefficients_np(coef, qt, nfo.width, nfo.height, nfo.ncomp, nfo.hs, nfo.vs)
    for a in (coef, qt, px):
        a.setflags(write=False)
    return nfo, coef, qt, px


_C = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16) for u in range(8)] for x in range(8)])


def idct_f64(blocks) -> np.ndarray:
    """(..., 8, 8) [v][u] -> (..., 8, 8) [y][x], float64, no level shift"""
    return np.einsum("yv,...vu,xu->...yx", _C, np.asarray(blocks, np.float64), _C)


def _taps(n_out, factor, n_samples):
    i = np.arange(n_out)
    if factor == 1:
        return i, i, 1.0, 0.0
    near = i >> 1
    return near, np.clip(near + np.where(i & 1, 1, -1), 0, n_samples - 1), 0.75, 0.25


def ideal_decode(nfo, coef, qt) -> np.ndarray:
    """float64 (H, W, 3), clipped to [0, 255] only at the very end"""
    from xmcgan_image_generation_amd.libml import jpeg
    w, h = nfo.width, nfo.height
    planes, off = [], 0
    for c, (bh, bw) in enumerate(jpeg.plane_blocks(nfo.ncomp, nfo.hs, nfo.vs, nfo.mcus_x, nfo.mcus_y)):
        blocks = coef[off:off + bh * bw * 64].reshape(bh, bw, 8, 8).astype(np.float64) * qt[c].reshape(8, 8).astype(np.float64)
        off += bh * bw * 64
        planes.append(idct_f64(blocks).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8) + 128.0)
    y = planes[0][:h, :w]
    if nfo.ncomp == 1:
        return np.clip(np.repeat(y[..., None], 3, axis=2), 0, 255)
    cw, ch = -(-w // nfo.hs), -(-h // nfo.vs)
    x0, x1, wx0, wx1 = _taps(w, nfo.hs, cw)
    y0, y1, wy0, wy1 = _taps(h, nfo.vs, ch)

    def up(p):
        return wy0 * (wx0 * p[y0][:, x0] + wx1 * p[y0][:, x1]) + wy1 * (wx0 * p[y1][:, x0] + wx1 * p[y1][:, x1])
    cb, cr = up(planes[1]) - 128.0, up(planes[2]) - 128.0
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(rgb, 0, 255)


def rows_for_each_filter():
    """a (6, 24, 3) image whose rows are built so that filters 0, 2, 1, 3, 4 win in turn (row 0 has no row above it)"""
    rng = np.random.default_rng(3)
    w = 24
    img = np.zeros((6, w, 3), np.uint8)
    img[0] = np.where(rng.integers(0, 2, (w, 3)), 1, 255)                         # small as signed bytes: None wins
    img[1] = img[0]                                                               # equal to the row above: Up gives zeros
    img[2] = (np.arange(w)[:, None] * 9 + np.array([0, 80, 160])) % 256           # a ramp: Sub gives constants
    up, row, left = img[2].reshape(-1).astype(int), np.zeros(w * 3, int), np.zeros(3, int)
    for i in range(w * 3):                                                        # exactly the Average prediction
        a = row[i - 3] if i >= 3 else 0
        row[i] = ((a + up[i]) >> 1) & 0xff
    img[3] = row.reshape(w, 3)
    # Paeth: a plane a + b - c continues exactly: rows 4 = row 3 shifted pattern + gradient in both axes
    base = rng.integers(60, 120, 3)
    yy, xx = np.mgrid[0:2, 0:w]
    plane = (base[None, None, :] + 40 * yy[..., None] * np.array([1, 0, 1]) + 5 * xx[..., None] * np.array([0, 1, 1])) % 256
    img[4:6] = plane
    return img


# ------------------------------------------------------------------------------------------- the dataset builder's tree
TREE = (("COCO_train2014_000000000009.jpg", "q90_420"), ("COCO_train2014_000000000025.jpg", "prog_444"),
        ("COCO_train2014_000000000030.jpg", "q90_grey"))
WORDS = ("a man riding a horse", "two dogs on the beach", "a red bus on the street", "a cat sitting on a table with pizza",
         "the horse and the dog", "a man with a red table", "two cats riding a bus")


def make_tree(root, captions_per_image=5):
    """three fixture files under ``root/images`` and a COCO annotation file that lists their captions INTERLEAVED (annotation
    k belongs to image k mod 3) and the images in an order that is not alphabetical.  -> (images dir, annotation path,
    [(file name, [captions in annotation order])])"""
    import json
    images = os.path.join(str(root), "images")
    os.makedirs(images, exist_ok=True)
    order = [TREE[2], TREE[0], TREE[1]]
    for fname, fixture in TREE:
        with open(os.path.join(images, fname), "wb") as f:
            f.write(jpeg_bytes(fixture))
    ann = {"images": [{"id": 100 + k, "file_name": fname} for k, (fname, _) in enumerate(order)], "annotations": []}
    caps = {fname: [] for fname, _ in order}
    for a in range(3 * captions_per_image):
        k = a % 3
        text = f"{WORDS[a % len(WORDS)]} {WORDS[(a * 3 + 1) % len(WORDS)]}"[:60] if a % 4 else WORDS[a % len(WORDS)]
        ann["annotations"].append({"id": 9000 + a, "image_id": 100 + k, "caption": text})
        caps[order[k][0]].append(text)
    path = os.path.join(str(root), "captions_train2014.json")
    with open(path, "w") as f:
        json.dump(ann, f)
    return images, path, [(fname, caps[fname]) for fname, _ in order]


def stub_encoder(ids, max_len):
    """(ids, max_len) -> (N, T, 768) float32, a fixed function of the token ids: stands in for BERT on a CPU"""
    ids = np.asarray(ids, np.float32)
    return (ids[:, :, None] * 0.01 + np.arange(768, dtype=np.float32)[None, None, :] * 1e-3).astype(np.float32)


def read_shards(out_dir, version, split, n):
    """[(shard index, [serialized examples])] of a finished run"""
    from xmcgan_image_generation_amd import preprocess_data as P
    from xmcgan_image_generation_amd.libml import tfrecord
    return [(i, list(tfrecord.read_records(os.path.join(str(out_dir), P.shard_name(version, split, i, n))))) for i in range(n)]
