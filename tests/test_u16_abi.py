"""16-bit greyscale entry points (glf_image_processing_u16, its _capture variant, glf_multi_image_processing_u16, the 16-bit PNG
codec, GLF_KERNEL_BILATERAL_U16): exported by libglf.so, declared in include/glf.h, and their argument checks answer GLF_ERR_INVALID
before any device work. CPU only (the host program's flag checks run after it has opened a device: tests/test_host_u16.py)."""
import ctypes as C
import os
import re

import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_image_processing_u16", "glf_image_processing_u16_capture", "glf_multi_image_processing_u16", "glf_read_png16",
         "glf_write_png16")


def test_u16_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"GLF_KERNEL_BILATERAL_U16\s*=\s*5\b", header) and glf.KERNEL_BILATERAL_U16 == 5
    assert re.search(r"GLF_KERNEL_BILATERAL_RGB\s*=\s*4\b", header) and glf.KERNEL_BILATERAL_RGB == 4   # appended, no renumbering
    assert hasattr(glf.Context, "image_processing_u16") and hasattr(glf.Multi, "image_processing_u16")
    assert callable(glf.read_png16) and callable(glf.write_png16)


@pytest.mark.parametrize("img,out,w,h", [(None, 1, 8, 8), (1, None, 8, 8), (1, 1, 0, 8), (1, 1, 8, -1), (1, 1, 8, 8)])
def test_null_or_invalid_arguments_are_invalid_without_a_device(img, out, w, h):
    """Without a context / world, with a null image or output, or a non-positive size: GLF_ERR_INVALID before any device work."""
    lib = C.CDLL(glf.LIB_PATH)
    rc = lib.glf_image_processing_u16(None, None, C.c_void_p(img), C.c_int(w), C.c_int(h), C.c_void_p(out), None, None, None)
    assert rc == glf.ERR_INVALID
    rc = lib.glf_image_processing_u16_capture(None, None, C.c_void_p(img), C.c_int(w), C.c_int(h), C.c_void_p(out), None, None, None,
                                              None)
    assert rc == glf.ERR_INVALID
    rc = lib.glf_multi_image_processing_u16(None, None, C.c_void_p(img), C.c_int(w), C.c_int(h), C.c_void_p(out), None, None, None)
    assert rc == glf.ERR_INVALID


def test_stage_entry_rejects_null_image_for_the_u16_kernel():
    lib = C.CDLL(glf.LIB_PATH)
    K_B = glf.Mat()
    rc = lib.glf_ComputeAffinityMatrices(None, None, C.byref(K_B), None, C.c_int(8), C.c_int(8), C.c_uint(4), None,
                                         C.c_int(glf.KERNEL_BILATERAL_U16), C.c_float(40.0), C.c_float(30.0 * 257))
    assert rc == glf.ERR_INVALID


def test_png16_null_arguments():
    lib = C.CDLL(glf.LIB_PATH)
    rows = C.c_void_p()
    w, h = C.c_int(), C.c_int()
    assert lib.glf_read_png16(None, C.byref(rows), C.byref(w), C.byref(h)) == -1
    assert lib.glf_write_png16(None, None, C.c_uint(4), C.c_uint(4)) == -1
