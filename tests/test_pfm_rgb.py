"""The colour Portable Float Map codec (glf_read_pfm_rgb / glf_write_pfm_rgb): "PF\\n<width> <height>\\n<scale>\\n", then 3 * width *
height raw floats, rows of 3 * width (R G B interleaved), bottom row first, little-endian for a negative scale and big-endian for a
positive one. CPU only."""
import struct

import numpy as np
import pytest

import glf

# top row first, 3 wide x 2 high, [row][pixel][channel]
VALUES = [[[1.5, -2.25, 3.0], [1e-3, -7.0, 65536.5], [0.0, 0.25, -0.5]],
          [[10.0, 20.0, 30.0], [-1.0, -2.0, -3.0], [7.5, 8.5, 9.5]]]


def _file(byte_order, header=None, rows=VALUES, magic="PF"):
    """A PFM built with struct.pack, independent of the codec: the bottom row first."""
    head = header if header is not None else ("%s\n3 2\n%s\n" % (magic, "-1.0" if byte_order == "<" else "1.0")).encode()
    flat = [[c for px in r for c in px] for r in rows]
    return head + b"".join(struct.pack(byte_order + "%df" % len(r), *r) for r in flat[::-1])


def _write(tmp_path, data, name="a.pfm"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@pytest.mark.parametrize("byte_order", ["<", ">"])
def test_reads_an_independently_built_file_rows_top_first(tmp_path, byte_order):
    """Both byte orders; the file's first row is the image's bottom row."""
    img = glf.read_pfm_rgb(_write(tmp_path, _file(byte_order)))
    assert img.dtype == np.float32 and img.shape == (2, 3, 3)
    np.testing.assert_array_equal(img, np.array(VALUES, dtype=np.float32))
    assert img[1, 0, 0] == 10.0 and img[0, 0, 0] == 1.5


def test_writer_is_little_endian_scale_minus_one_bottom_row_first(tmp_path):
    p = str(tmp_path / "w.pfm")
    glf.write_pfm_rgb(p, np.array(VALUES, dtype=np.float32))
    assert open(p, "rb").read() == _file("<")


def test_round_trip_bit_for_bit(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.normal(0.0, 50.0, (19, 37, 3)).astype(np.float32)       # 37 wide, 19 high: negative values throughout
    img[0, 0] = [1e-45, -1e-40, 3e-39]                                 # subnormal
    img[1, 0] = [3.4e38, -3.4e38, -0.0]                                # huge, and the negative zero
    img[18, 36] = [-123.456, 0.0, 1e30]
    assert (img < 0).any() and img.shape[0] != img.shape[1]
    p = str(tmp_path / "rt.pfm")
    glf.write_pfm_rgb(p, img)
    back = glf.read_pfm_rgb(p)
    assert back.shape == img.shape
    np.testing.assert_array_equal(back.view(np.int32), img.view(np.int32))


def test_each_reader_refuses_the_other_magic(tmp_path):
    colour = _write(tmp_path, _file("<"), "c.pfm")
    grey = _write(tmp_path, b"Pf\n3 2\n-1.0\n" + struct.pack("<18f", *range(18)), "g.pfm")   # (room for 3 x 2 x 3 floats)
    with pytest.raises(glf.GlfError):
        glf.read_pfm_rgb(grey)
    with pytest.raises(glf.GlfError):
        glf.read_pfm(colour)
    assert glf.read_pfm(grey).shape == (2, 3) and glf.read_pfm_rgb(colour).shape == (2, 3, 3)


REJECTED = {
    "grey Pf": _file("<", magic="Pf"),
    "truncated data": _file("<")[:-1],
    "a third of the data": _file("<")[:len(b"PF\n3 2\n-1.0\n") + 24],
    "zero width": _file("<", header=b"PF\n0 5\n-1.0\n"),
    "zero height": _file("<", header=b"PF\n5 0\n-1.0\n"),
    "width overflows int": _file("<", header=b"PF\n99999999999 5\n-1.0\n"),
    "size overflows": _file("<", header=b"PF\n2147483647 2147483647\n-1.0\n"),
    "3 x size overflows": _file("<", header=b"PF\n1431655766 2147483647\n-1.0\n"),
    "missing scale line": _file("<", header=b"PF\n3 2\n"),
    "zero scale": _file("<", header=b"PF\n3 2\n0.0\n"),
    "empty file": b"",
    "magic only": b"PF",
    "not a PFM": b"\x89PNG\r\n\x1a\n" + bytes(80),
}


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejections(tmp_path, case):
    with pytest.raises(glf.GlfError) as e:
        glf.read_pfm_rgb(_write(tmp_path, REJECTED[case]))
    assert e.value.status == glf.ERR_IO


def test_missing_file(tmp_path):
    with pytest.raises(glf.GlfError):
        glf.read_pfm_rgb(str(tmp_path / "nope.pfm"))
