"""JPEG on the host: the entropy decoder (csrc_host/xmc_jpeg.c), the integer specification of the pixel stage
(libml/jpeg.py) and the PNG filter specification (libml/png.py: filter_rows_np).  No GPU.

Measured on the fixtures (profiles/r19_jpeg_accuracy.txt has the table): mean |specification - ideal| is at most 1.044 times
Pillow's mean |Pillow - ideal|, the maximum exceeds Pillow's by at most 0.20 level; |specification - Pillow| is at most 3 levels
(grey: 1) and 0.23 on average.  IEEE 1180-1990 on the specification's
IDCT: peak error 1, worst mean square error 0.0187 at a position and 0.0153 overall, worst mean error 0.0029 / 0.0002."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_ref as R
from xmcgan_image_generation_amd.libml import jpeg, png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# how far the specification's mean error may exceed Pillow's: both are integer approximations of one ideal; the largest ratio
# measured on the fixtures is 1.044 (a 17 x 9 image, 459 values), so 1.15 leaves room for that noise and little else
MEAN_MARGIN = 1.15


# ------------------------------------------------------------------------------------------------ IEEE 1180-1990
@pytest.mark.parametrize("lo,hi", [(-256, 255), (-5, 5), (-300, 300)])
@pytest.mark.parametrize("sign", [1, -1])
def test_idct_meets_ieee_1180(lo, hi, sign):
    rng = np.random.default_rng(1180 + hi)
    data = sign * rng.integers(lo, hi + 1, (10000, 8, 8))
    coef = np.clip(np.rint(np.einsum("yv,nyx,xu->nvu", R._C, data.astype(np.float64), R._C)), -2048, 2047)   # float64 forward DCT
    want = np.clip(np.rint(R.idct_f64(coef)), -256, 255)
    got = np.clip(jpeg.idct_signed_np(coef.astype(np.int64), np.ones(64, np.int64)), -256, 255)
    e = (got - want).astype(np.float64)
    figures = dict(peak=np.abs(e).max(), pmse=(e ** 2).mean(axis=0).max(), omse=(e ** 2).mean(), pme=np.abs(e.mean(axis=0)).max(),
                   ome=abs(e.mean()))
    print(f"1180 [{lo}, {hi}] sign {sign}: {figures}")
    assert figures["peak"] <= 1
    assert figures["pmse"] <= 0.06 and figures["omse"] <= 0.02
    assert figures["pme"] <= 0.015 and figures["ome"] <= 0.0015


def test_idct_of_zeros_is_zero():
    assert not jpeg.idct_signed_np(np.zeros((3, 8, 8), np.int64), np.full(64, 255)).any()
    assert (jpeg.idct_blocks_np(np.zeros((8, 8), np.int16), np.ones(64)) == 128).all()


def test_int32_bounds_of_the_specification():
    """the derivation in libml/jpeg.py, evaluated: extreme inputs stay inside int32 at every step"""
    m = np.abs(jpeg.IDCT_MATRIX).sum(axis=1).max()
    assert m * jpeg.DEQUANT_CLAMP + (1 << (jpeg.PASS1_SHIFT - 1)) < 2 ** 31
    assert m * jpeg.PASS1_CLAMP + (1 << (jpeg.PASS2_SHIFT - 1)) < 2 ** 31
    assert 32768 * 65535 < 2 ** 31                     # any int16 times any uint16
    for c, q in ((32767, 65535), (-32768, 65535), (2047, 255), (-2047, 65535)):
        blk = np.full((8, 8), c, np.int64) * np.where(np.indices((8, 8)).sum(0) % 2, 1, -1)
        out = jpeg.idct_blocks_np(blk, np.full(64, q))
        assert out.dtype == np.uint8


# ---------------------------------------------------------------------------------- the fixtures against Pillow
def _errors(name):
    nfo, coef, qt, px = R.decoded(name)
    ideal = R.ideal_decode(nfo, coef, qt)
    ep, es = np.abs(R.pillow_pixels(name) - ideal), np.abs(px - ideal)
    return ep.mean(), ep.max(), es.mean(), es.max()


@pytest.mark.parametrize("name", R.names())
def test_specification_is_as_close_to_the_ideal_as_pillow(name):
    nfo, _, _, px = R.decoded(name)
    assert px.shape == R.pillow_pixels(name).shape == (nfo.height, nfo.width, 3)
    pm, px_max, sm, sx = _errors(name)
    print(f"{name}: Pillow mean {pm:.4f} max {px_max:.3f}; specification mean {sm:.4f} max {sx:.3f}")
    assert sm <= MEAN_MARGIN * pm
    assert sx <= px_max + 1.0


# What holds the ENTROPY decoder to something it did not produce itself.  The ideal above is built from xmc_jpeg.c's own
# coefficients, so a wrongly decoded scan would move it along; these two tests compare with Pillow's recorded pixels directly.
# Bounds: both decoders round at the same three places (sample, upsampled chroma, output), so they differ by a level at many
# pixels, by 2 or 3 where the chroma roundings add up through the 1.772 and 1.402 gains, and by half a level on average at the
# very most; a grey image has one rounding place (IEEE 1180 allows each IDCT a peak error of 1).  A wrong coefficient of any
# band moves a whole 8 x 8 block by its quantisation step over 8 per unit, a lost DC difference or a mis-indexed block by
# tens of levels.
@pytest.mark.parametrize("name", R.names())
def test_specification_against_the_recorded_pillow_pixels(name):
    nfo, _, _, px = R.decoded(name)
    d = np.abs(px.astype(np.int64) - R.pillow_pixels(name).astype(np.int64))
    print(f"{name}: |specification - Pillow| max {d.max()} mean {d.mean():.4f}")
    assert d.max() <= (2 if nfo.ncomp == 1 else 3)
    assert d.mean() <= 0.5


@pytest.mark.parametrize("group", R.groups(), ids=lambda g: g[0])
def test_files_that_differ_only_in_entropy_coding_hold_the_same_coefficients(group):
    """one image, one quality, one subsampling, written baseline, with fitted Huffman tables, with restart intervals and as
    progressive scans (spectral selection and successive approximation): libjpeg quantises before it chooses the coding, so
    the decoder must return the baseline file's coefficients and tables for every one of them, exactly"""
    base = R.decoded(group[0])
    assert base[0].process == 0
    for other in group[1:]:
        nfo, coef, qt, _ = R.decoded(other)
        assert (nfo.width, nfo.height, nfo.ncomp, nfo.hs, nfo.vs) == (base[0].width, base[0].height, base[0].ncomp, base[0].hs, base[0].vs)
        assert np.array_equal(qt, base[2]), other
        bad = np.flatnonzero(coef != base[1])
        assert bad.size == 0, f"{other}: {bad.size} coefficients differ from {group[0]}, first at {bad[:5]}"


def test_groups_cover_every_coding_and_sampling():
    groups = R.groups()
    members = {n for g in groups for n in g}
    assert {"opt_420", "prog_420", "rstb2_420", "rstb2_prog_420", "rstr1_422", "prog_422", "prog_444", "prog_grey"} <= members
    assert {jpeg.info(R.jpeg_bytes(n)).process for n in members} == {0, 2}


def test_fixture_set_covers_what_the_issue_lists():
    got = {n: jpeg.info(R.jpeg_bytes(n)) for n in R.names()}
    assert {(i.ncomp, i.hs, i.vs) for i in got.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {i.process for i in got.values()} == {0, 2}
    assert {(i.width, i.height) for i in got.values()} >= {(1, 1), (8, 8), (17, 9), (37, 29)}
    assert b"\xff\xdd" in R.jpeg_bytes("rstb2_420") and b"\xff\xd0" in R.jpeg_bytes("rstr1_422")
    assert os.path.getsize(R.FIXTURE_PATH) < 100_000


def test_progressive_and_sequential_files_of_one_image_give_the_same_coefficients():
    """Pillow writes the same quantised coefficients whatever the scan script: q90 4:2:0 sequential, optimised, with restart
    markers and progressive differ only in their entropy coding"""
    # (each fixture has its own noise seed, so encode one image here both ways when Pillow is present)
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(5)
    img = Image.fromarray(rng.integers(0, 256, (29, 37, 3), dtype=np.uint8))
    outs = []
    for opts in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_marker_blocks=3),
                 dict(progressive=True, restart_marker_rows=1)):
        buf = io.BytesIO()
        img.save(buf, "JPEG", quality=85, subsampling=2, **opts)
        nfo, coef, qt = jpeg.coefficients(buf.getvalue())
        outs.append((coef, qt))
        live = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).astype(int)
        assert np.abs(jpeg.decode_np(buf.getvalue()).astype(int) - live).max() <= 4
    for coef, qt in outs[1:]:
        assert np.array_equal(coef, outs[0][0]) and np.array_equal(qt, outs[0][1])


# -------------------------------------------------------------------------------------------------- refusals
def _patch_sof(data: bytes, marker=None, precision=None) -> bytes:
    b = bytearray(data)
    i = b.index(b"\xff\xc0")
    if marker is not None:
        b[i + 1] = marker
    if precision is not None:
        b[i + 4] = precision
    return bytes(b)


def test_refusals_have_their_own_codes():
    base = R.jpeg_bytes("q90_420")
    cases = [(R.jpeg_bytes("cmyk_8x8"), jpeg.E_COMPONENTS), (_patch_sof(base, marker=0xC9), jpeg.E_ARITHMETIC),
             (_patch_sof(base, marker=0xCA), jpeg.E_ARITHMETIC), (_patch_sof(base, precision=12), jpeg.E_PRECISION),
             (_patch_sof(base, marker=0xC3), jpeg.E_PROCESS)]
    b = bytearray(base)
    i = b.index(b"\xff\xc0")
    b[i + 11] = 0x41                                   # luma sampling 4 x 1
    cases.append((bytes(b), jpeg.E_SAMPLING))
    b = bytearray(base)
    b[i + 5:i + 9] = (20000).to_bytes(2, "big") + (16).to_bytes(2, "big")
    cases.append((bytes(b), jpeg.E_SIZE))
    for data, code in cases:
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.info(data)
        assert e.value.code == code and e.value.unsupported
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.coefficients(data)
        assert e.value.code == code
    assert len({c for _, c in cases}) == 6


def test_damaged_input_returns_codes():
    data = R.jpeg_bytes("rstb2_420")
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.coefficients(data[:len(data) // 2])
    assert e.value.code == jpeg.E_TRUNCATED and not e.value.unsupported
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.coefficients(data[:-2])                   # no EOI
    assert e.value.code == jpeg.E_TRUNCATED
    b = bytearray(data)
    k = b.index(b"\xff\xd1")
    b[k + 1] = 0xD5                                    # the second restart marker is the wrong one
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.coefficients(bytes(b))
    assert e.value.code == jpeg.E_RESTART
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.info(b"\x89PNG\r\n\x1a\n" + bytes(32))
    assert e.value.code == jpeg.E_MALFORMED
    nfo = jpeg.info(data)
    rc = jpeg.coefficients_into(data, np.empty(nfo.coef_bytes // 2 - 64, np.int16), np.empty((3, 64), np.uint16))
    assert rc == jpeg.E_BUFFER


def test_scan_count_is_capped():
    """a progressive file may repeat a scan: 256 are decoded, the 257th is refused with its own code, before it is walked"""
    data = R.jpeg_bytes("prog_grey")
    first = data.index(b"\xff\xda")
    second = data.index(b"\xff\xda", first + 2)
    scan = data[first:second]                                     # the DC scan (and what follows it up to the next scan)
    assert jpeg.coefficients(data[:first] + scan * 200 + data[first:])[1] is not None
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.coefficients(data[:first] + scan * 300 + data[first:])
    assert e.value.code == jpeg.E_SCANS and not e.value.unsupported


def test_entropy_decoder_under_sanitizers(tmp_path):
    """every fixture truncated at each offset and 2,000 seeded corruptions of each, through a stand-alone program built with
    -fsanitize=address,undefined (runtime linked statically): every call returns and nothing is reported"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler (the build needs one too)"
    flags = ["-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run([cc] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link an empty program with -fsanitize=address,undefined")
    exe = tmp_path / "jpeg_fuzz"
    src = [os.path.join(ROOT, "tests", "c", "jpeg_fuzz.c"), os.path.join(ROOT, "xmcgan_image_generation_amd", "csrc_host", "xmc_jpeg.c")]
    build = subprocess.run([cc] + flags + ["-o", str(exe)] + src, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    files = []
    for n in R.names(decodable_only=False):
        p = tmp_path / (n + ".jpg")
        p.write_bytes(R.jpeg_bytes(n))
        files.append(str(p))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    calls = int(run.stdout.split()[0])
    assert calls >= sum(len(R.jpeg_bytes(n)) + 2001 for n in R.names(decodable_only=False))


# ---------------------------------------------------------------------------------------------- PNG filter rows
def test_filter_rows_each_filter_wins_where_built_to():
    img = R.rows_for_each_filter()
    stream, ids = png.filter_rows_np(img)
    assert list(ids[:4]) == [0, 2, 1, 3] and ids[5] == 4, ids
    assert stream.dtype == np.uint8 and stream.size == 6 * (1 + 24 * 3)
    assert np.array_equal(stream.reshape(6, -1)[:, 0], ids)
    assert np.array_equal(png.decode_rgb(png.encode_filtered(stream, 6, 24)), img)
    # the filtered bytes are what encode_rgb computes for the same ids
    assert png.encode_rgb(img, filter_types=ids) == png.encode_filtered(stream, 6, 24)


def test_filter_rows_ties_go_to_the_lowest_id():
    img = np.zeros((3, 5, 3), np.uint8)                                            # every filter gives zeros: None
    assert list(png.filter_rows_np(img)[1]) == [0, 0, 0]
    img[:] = 7                                                                     # row 0: Sub = Paeth (7 then zeros), Up = None
    ids = png.filter_rows_np(img)[1]
    assert ids[0] == 1 and ids[1] == 2 and ids[2] == 2                             # Sub before Paeth; Up before Average / Paeth
    img = np.zeros((2, 2, 3), np.uint8)
    img[1] = 255                                                                   # -1 as signed: None costs 6; Sub and Paeth 3
    assert list(png.filter_rows_np(img)[1]) == [0, 1]


@pytest.mark.parametrize("name", ["q90_420", "prog_grey", "one_1x1", "q100_444"])
def test_filter_rows_round_trip_on_decoded_fixtures(name):
    px = R.decoded(name)[3]
    h, w, _ = px.shape
    stream, _ = png.filter_rows_np(px)
    data = png.encode_filtered(stream, h, w)
    assert np.array_equal(png.decode_rgb(data), px) and np.array_equal(png._decode_rgb_py(data), px)
    with pytest.raises(ValueError):
        png.encode_filtered(stream[:-1], h, w)
