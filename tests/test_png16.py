"""The 16-bit greyscale PNG codec (glf_read_png16 / glf_write_png16) against Pillow, and the rejections on both sides: read_png16
takes colour type 0 at bit depth 16 only, read_png still rejects 16-bit input. CPU only."""
import os
import zlib
import struct

import numpy as np
import pytest

import glf

Image = pytest.importorskip("PIL.Image")


def _ramp(h, w, seed=0):
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w]
    img = (r * 997 + c * 263) % 65536 + rng.integers(0, 64, (h, w))
    return np.clip(img, 0, 65535).astype(np.uint16)


def _pillow_write16(path, img, **kw):
    Image.fromarray(img).save(path, **kw)   # numpy uint16 -> mode "I;16": colour type 0, bit depth 16


@pytest.mark.parametrize("h,w", [(64, 80), (37, 53), (1, 29), (17, 1), (1, 1)])
@pytest.mark.parametrize("optimize", [False, True])
def test_pillow_written_files_read_back_identical(tmp_path, h, w, optimize):
    img = _ramp(h, w, seed=h * 1000 + w)
    p = str(tmp_path / "g16.png")
    _pillow_write16(p, img, optimize=optimize)
    with Image.open(p) as im:
        assert im.mode.startswith("I;16")
    np.testing.assert_array_equal(glf.read_png16(p), img)


def _png(path, w, h, bit_depth, color_type, raw_rows, filters, interlace=0):
    """A PNG written by hand: each row of bytes after its filter-type byte (the filter already applied by the caller)."""
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    raw = b"".join(bytes([f]) + r for f, r in zip(filters, raw_rows))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth, color_type, 0, 0, interlace)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _filter_rows(img16, ftype):
    """Big-endian rows of a uint16 image, each filtered with its scanline filter (bpp = 2)."""
    rows = [img16[r].astype(">u2").tobytes() for r in range(img16.shape[0])]
    out = []
    for y, row in enumerate(rows):
        prev = rows[y - 1] if y else bytes(len(row))
        f = ftype[y]
        enc = bytearray(len(row))
        for x in range(len(row)):
            a = row[x - 2] if x >= 2 else 0
            b = prev[x]
            c = prev[x - 2] if x >= 2 else 0
            if f == 0:
                pred = 0
            elif f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            enc[x] = (row[x] - pred) & 0xff
        out.append(bytes(enc))
    return out


def test_all_five_filters_with_two_byte_pixels(tmp_path):
    img = _ramp(10, 13, seed=5)
    ftype = [0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    p = str(tmp_path / "filters.png")
    _png(p, 13, 10, 16, 0, _filter_rows(img, ftype), ftype)
    np.testing.assert_array_equal(glf.read_png16(p), img)
    with Image.open(p) as im:   # (the hand-written file is a valid PNG: Pillow reads the same values)
        np.testing.assert_array_equal(np.array(im).astype(np.uint16), img)


@pytest.mark.parametrize("h,w", [(48, 61), (1, 7), (5, 1)])
def test_write_png16_read_back_by_pillow(tmp_path, h, w):
    img = _ramp(h, w, seed=w)
    img[0, 0], img[-1, -1] = 0, 65535
    p = str(tmp_path / "out16.png")
    glf.write_png16(p, img)
    with Image.open(p) as im:
        assert im.mode.startswith("I;16") and im.size == (w, h)
        np.testing.assert_array_equal(np.array(im).astype(np.uint16), img)
    np.testing.assert_array_equal(glf.read_png16(p), img)


def test_read_png16_rejects_other_formats(tmp_path):
    cases = {
        "g8.png": Image.fromarray(np.arange(64, dtype=np.uint8).reshape(8, 8)),
        "rgb.png": Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)),
        "rgba.png": Image.fromarray(np.zeros((8, 8, 4), dtype=np.uint8)),
        "pal.png": Image.fromarray(np.arange(64, dtype=np.uint8).reshape(8, 8)).convert("P"),
        "la.png": Image.fromarray(np.zeros((8, 8, 2), dtype=np.uint8), mode="LA"),
    }
    for name, im in cases.items():
        p = str(tmp_path / name)
        im.save(p)
        with pytest.raises(glf.GlfError):
            glf.read_png16(p)
    # interlaced 16-bit grey, a corrupt file (bad CRC), a truncated one, a file that is no PNG
    img = _ramp(4, 4)
    p = str(tmp_path / "interlaced.png")
    _png(p, 4, 4, 16, 0, _filter_rows(img, [0] * 4), [0] * 4, interlace=1)
    with pytest.raises(glf.GlfError):
        glf.read_png16(p)
    good = str(tmp_path / "good.png")
    _pillow_write16(good, img)
    data = bytearray(open(good, "rb").read())
    bad = str(tmp_path / "badcrc.png")
    data[40] ^= 0xff
    open(bad, "wb").write(bytes(data))
    with pytest.raises(glf.GlfError):
        glf.read_png16(bad)
    trunc = str(tmp_path / "trunc.png")
    open(trunc, "wb").write(open(good, "rb").read()[:-20])
    with pytest.raises(glf.GlfError):
        glf.read_png16(trunc)
    junk = str(tmp_path / "junk.png")
    open(junk, "wb").write(b"not a png at all" * 8)
    with pytest.raises(glf.GlfError):
        glf.read_png16(junk)
    with pytest.raises(glf.GlfError):
        glf.read_png16(str(tmp_path / "missing.png"))


def test_read_png_still_rejects_16_bit(tmp_path):
    p = str(tmp_path / "g16.png")
    _pillow_write16(p, _ramp(16, 16))
    with pytest.raises(glf.GlfError):
        glf.read_png(p)
    q = str(tmp_path / "w16.png")
    glf.write_png16(q, _ramp(9, 11))
    with pytest.raises(glf.GlfError):
        glf.read_png(q)
    with pytest.raises(glf.GlfError):
        glf.read_png_rgb(q)
