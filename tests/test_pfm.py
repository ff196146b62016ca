"""The greyscale Portable Float Map codec (glf_read_pfm / glf_write_pfm): "Pf\\n<width> <height>\\n<scale>\\n", then raw floats,
bottom row first, little-endian for a negative scale and big-endian for a positive one. CPU only."""
import struct

import numpy as np
import pytest

import glf

VALUES = [[1.5, -2.25, 3.0], [1e-3, -7.0, 65536.5]]      # top row first, 3 x 2


def _file(byte_order, header=None, rows=VALUES):
    """A PFM built with struct.pack, independent of the codec: the bottom row first."""
    head = header if header is not None else ("Pf\n3 2\n%s\n" % ("-1.0" if byte_order == "<" else "1.0")).encode()
    return head + b"".join(struct.pack(byte_order + "%df" % len(r), *r) for r in rows[::-1])


def _write(tmp_path, data, name="a.pfm"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@pytest.mark.parametrize("byte_order", ["<", ">"])
def test_reads_an_independently_built_file_rows_top_first(tmp_path, byte_order):
    img = glf.read_pfm(_write(tmp_path, _file(byte_order)))
    assert img.dtype == np.float32 and img.shape == (2, 3)
    np.testing.assert_array_equal(img, np.array(VALUES, dtype=np.float32))


def test_any_whitespace_between_header_tokens(tmp_path):
    img = glf.read_pfm(_write(tmp_path, _file("<", header=b"Pf \t\r\n3\n\n2 \t-1.0\n")))
    np.testing.assert_array_equal(img, np.array(VALUES, dtype=np.float32))


def test_writer_is_little_endian_scale_minus_one_bottom_row_first(tmp_path):
    p = str(tmp_path / "w.pfm")
    glf.write_pfm(p, np.array(VALUES, dtype=np.float32))
    assert open(p, "rb").read() == _file("<")


def test_round_trip_bit_for_bit(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.normal(0.0, 50.0, (19, 37)).astype(np.float32)          # 37 wide, 19 high: negative values throughout
    img[0, :4] = [1e-45, -1e-40, 3e-39, 0.0]                           # subnormal
    img[1, :4] = [3.4e38, -3.4e38, 1e30, -0.0]                         # huge, and the negative zero
    img[18, 36] = -123.456
    p = str(tmp_path / "rt.pfm")
    glf.write_pfm(p, img)
    back = glf.read_pfm(p)
    assert back.shape == img.shape
    np.testing.assert_array_equal(back.view(np.int32), img.view(np.int32))


REJECTED = {
    "colour PF": _file("<", header=b"PF\n3 2\n-1.0\n", rows=[r * 3 for r in VALUES]),
    "truncated data": _file("<")[:-1],
    "half the data": _file("<")[:len(b"Pf\n3 2\n-1.0\n") + 12],
    "zero width": _file("<", header=b"Pf\n0 5\n-1.0\n"),
    "width overflows int": _file("<", header=b"Pf\n99999999999 5\n-1.0\n"),
    "size overflows": _file("<", header=b"Pf\n2147483647 2147483647\n-1.0\n"),
    "missing scale line": _file("<", header=b"Pf\n3 2\n"),
    "zero scale": _file("<", header=b"Pf\n3 2\n0.0\n"),
    "empty file": b"",
    "magic only": b"Pf",
    "not a PFM": b"\x89PNG\r\n\x1a\n" + bytes(40),
}


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejections(tmp_path, case):
    with pytest.raises(glf.GlfError) as e:
        glf.read_pfm(_write(tmp_path, REJECTED[case]))
    assert e.value.status == glf.ERR_IO


def test_missing_file(tmp_path):
    with pytest.raises(glf.GlfError):
        glf.read_pfm(str(tmp_path / "nope.pfm"))
