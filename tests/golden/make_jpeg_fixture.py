"""Writes tests/golden/jpeg_fixtures.npz: small JPEG files made with Pillow (libjpeg) from images synthesised in NumPy, and
Pillow's own decode of each, recorded so that no test needs Pillow to compare against it.

    python tests/golden/make_jpeg_fixture.py

Per fixture ``NAME``: ``NAME.jpg`` (the file's bytes, uint8) and ``NAME.rgb`` (Pillow's pixels, uint8 (H, W, 3)); the CMYK
file, which the decoder refuses, has no pixels.  ``names`` lists them in order.  ``groups`` (JSON) lists the sets of fixtures
that were made from one image with one mode, quality and subsampling and differ only in their entropy coding."""
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def synth(w, h, seed):
    """gradients, a hard edge and noise: smooth areas, a discontinuity across block borders, and full-band energy"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 255 * (x + y) / max(w + h - 2, 1)], axis=-1)
    img[:, w // 3:, 0] = 255 - img[:, w // 3:, 0]                      # vertical edge off the block grid
    img[h // 2:, :, 2] = 40                                            # horizontal edge
    img += rng.normal(0, 12, img.shape)
    img[:h // 4, :w // 4] = rng.integers(0, 256, (h // 4, w // 4, 3))  # a patch of pure noise
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# name, (w, h), mode, save options
FIXTURES = [
    ("q90_444", (37, 29), "RGB", dict(quality=90, subsampling=0)),
    ("q90_422", (37, 29), "RGB", dict(quality=90, subsampling=1)),
    ("q90_420", (37, 29), "RGB", dict(quality=90, subsampling=2)),
    ("q90_grey", (37, 29), "L", dict(quality=90)),
    ("q50_420", (37, 29), "RGB", dict(quality=50, subsampling=2)),
    ("q50_444", (17, 9), "RGB", dict(quality=50, subsampling=0)),
    ("q100_422", (37, 29), "RGB", dict(quality=100, subsampling=1)),
    ("q100_444", (17, 9), "RGB", dict(quality=100, subsampling=0)),
    ("q100_420", (17, 9), "RGB", dict(quality=100, subsampling=2)),
    ("opt_420", (37, 29), "RGB", dict(quality=90, subsampling=2, optimize=True)),
    ("opt_grey", (17, 9), "L", dict(quality=50, optimize=True)),
    ("prog_420", (37, 29), "RGB", dict(quality=90, subsampling=2, progressive=True)),
    ("prog_444", (17, 9), "RGB", dict(quality=50, subsampling=0, progressive=True)),
    ("prog_422", (37, 29), "RGB", dict(quality=100, subsampling=1, progressive=True)),
    ("prog_grey", (37, 29), "L", dict(quality=90, progressive=True)),
    ("rstb2_420", (37, 29), "RGB", dict(quality=90, subsampling=2, restart_marker_blocks=2)),
    ("rstr1_422", (37, 29), "RGB", dict(quality=90, subsampling=1, restart_marker_rows=1)),
    ("rstb2_prog_420", (37, 29), "RGB", dict(quality=90, subsampling=2, progressive=True, restart_marker_blocks=2)),
    ("one_1x1", (1, 1), "RGB", dict(quality=90, subsampling=2)),
    ("one_8x8", (8, 8), "RGB", dict(quality=90, subsampling=0)),
    ("mcu_8x8_420", (8, 8), "RGB", dict(quality=90, subsampling=2)),
    ("cmyk_8x8", (8, 8), "CMYK", dict(quality=90)),
]


def main():
    out, names = {}, []
    for name, (w, h), mode, opts in FIXTURES:
        # one source image per size: fixtures that differ only in their entropy coding (optimised tables, progressive scans,
        # restart markers) then hold the same quantised coefficients, which tests/test_jpeg.py asserts
        px = synth(w, h, 100 + 31 * w + h)
        im = Image.fromarray(px).convert(mode) if mode != "CMYK" else Image.fromarray(np.concatenate([px, px[..., :1]], -1), "CMYK")
        buf = io.BytesIO()
        im.save(buf, "JPEG", **opts)
        data = buf.getvalue()
        out[name + ".jpg"] = np.frombuffer(data, np.uint8)
        if mode != "CMYK":
            out[name + ".rgb"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        names.append(name)
        print(f"{name:16s} {w:3d} x {h:3d} {len(data):6d} bytes")
    out["names"] = np.array(names)
    groups = {}
    for name, size, mode, opts in FIXTURES:
        if mode != "CMYK":
            groups.setdefault((size, mode, opts.get("quality"), opts.get("subsampling")), []).append(name)
    out["groups"] = np.array(json.dumps([g for g in groups.values() if len(g) > 1]))
    path = os.path.join(HERE, "jpeg_fixtures.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
