"""Float colour entry points (glf_image_processing_rgbf32, its _capture and _signals variants, the glf_multi_ counterparts, the colour
PFM codec, GLF_KERNEL_BILATERAL_RGBF32): exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS, their argument
checks answer GLF_ERR_INVALID before any device work, and the public structures keep their sizes. CPU only."""
import ctypes as C
import os
import re

import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_image_processing_rgbf32", "glf_image_processing_rgbf32_capture", "glf_image_processing_rgbf32_signals",
         "glf_multi_image_processing_rgbf32", "glf_multi_image_processing_rgbf32_signals", "glf_read_pfm_rgb", "glf_write_pfm_rgb")


def test_rgbf32_entry_points_are_exported_declared_and_listed():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert hasattr(glf.Context, "image_processing_rgbf32") and hasattr(glf.Context, "image_processing_rgbf32_signals")
    assert hasattr(glf.Multi, "image_processing_rgbf32") and hasattr(glf.Multi, "image_processing_rgbf32_signals")
    assert callable(glf.read_pfm_rgb) and callable(glf.write_pfm_rgb)


def test_kernel_id_is_appended():
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    assert re.search(r"GLF_KERNEL_BILATERAL_RGBF32\s*=\s*7\b", header) and glf.KERNEL_BILATERAL_RGBF32 == 7
    for name, value in (("BILATERAL", 0), ("PHOTOMETRIC", 1), ("SPATIAL", 2), ("NLM", 3), ("BILATERAL_RGB", 4), ("BILATERAL_U16", 5),
                        ("BILATERAL_F32", 6)):
        assert re.search(r"GLF_KERNEL_%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(glf, "KERNEL_" + name) == value


ARGS = [(None, 1, 8, 8), (1, None, 8, 8), (1, 1, 0, 8), (1, 1, 8, -1), (1, 1, 8, 8)]


@pytest.mark.parametrize("img,out,w,h", ARGS)
def test_null_or_invalid_arguments_are_invalid_without_a_device(img, out, w, h):
    """Without a context / world, with a null image or output, or a non-positive size: GLF_ERR_INVALID before any device work."""
    lib = C.CDLL(glf.LIB_PATH)
    p = C.c_void_p
    rc = lib.glf_image_processing_rgbf32(None, None, p(img), C.c_int(w), C.c_int(h), p(out), None, None)
    assert rc == glf.ERR_INVALID
    rc = lib.glf_image_processing_rgbf32_capture(None, None, p(img), C.c_int(w), C.c_int(h), p(out), None, None, None)
    assert rc == glf.ERR_INVALID
    rc = lib.glf_multi_image_processing_rgbf32(None, None, p(img), C.c_int(w), C.c_int(h), p(out), None, None)
    assert rc == glf.ERR_INVALID
    rc = lib.glf_image_processing_rgbf32_signals(None, None, p(img), C.c_int(w), C.c_int(h), C.c_int(1), p(1), p(1), p(out), None, None)
    assert rc == glf.ERR_INVALID
    rc = lib.glf_multi_image_processing_rgbf32_signals(None, None, p(img), C.c_int(w), C.c_int(h), C.c_int(1), p(1), p(1), p(out), None, None)
    assert rc == glf.ERR_INVALID


@pytest.mark.parametrize("nsig,sig,sig_out", [(0, 1, 1), (5, 1, 1), (1, None, 1), (1, 1, None)])
def test_signals_plane_arguments_are_invalid_without_a_device(nsig, sig, sig_out):
    lib = C.CDLL(glf.LIB_PATH)
    p = C.c_void_p
    for name in ("glf_image_processing_rgbf32_signals", "glf_multi_image_processing_rgbf32_signals"):
        rc = getattr(lib, name)(None, None, p(1), C.c_int(8), C.c_int(8), C.c_int(nsig), p(sig), p(sig_out), p(1), None, None)
        assert rc == glf.ERR_INVALID, name


def test_stage_entry_rejects_null_image_for_the_rgbf32_kernel():
    lib = C.CDLL(glf.LIB_PATH)
    K_B = glf.Mat()
    rc = lib.glf_ComputeAffinityMatrices(None, None, C.byref(K_B), None, C.c_int(8), C.c_int(8), C.c_uint(4), None,
                                         C.c_int(glf.KERNEL_BILATERAL_RGBF32), C.c_float(40.0), C.c_float(7.71))
    assert rc == glf.ERR_INVALID


def test_pfm_rgb_null_arguments():
    lib = C.CDLL(glf.LIB_PATH)
    rows = C.c_void_p()
    w, h = C.c_int(), C.c_int()
    assert lib.glf_read_pfm_rgb(None, C.byref(rows), C.byref(w), C.byref(h)) == -1
    assert lib.glf_read_pfm_rgb(b"x.pfm", None, C.byref(w), C.byref(h)) == -1
    assert lib.glf_write_pfm_rgb(None, None, C.c_uint(4), C.c_uint(4)) == -1
    assert lib.glf_write_pfm_rgb(b"x.pfm", None, C.c_uint(4), C.c_uint(4)) == -1


def test_public_structures_keep_their_sizes():
    """The value block rides behind the records of glf_mat.samples: glf_mat, glf_options, glf_stats and glf_capture have the sizes
    they had before the format (through the Python mirrors; the library checks the two struct_size fields itself)."""
    assert hasattr(C.CDLL(glf.LIB_PATH), "glf_image_processing_rgbf32")
    assert (C.sizeof(glf.Mat), C.sizeof(glf.Options), C.sizeof(glf.Stats), C.sizeof(glf.Capture)) == (128, 104, 184, 72)
    assert glf.default_options().struct_size == C.sizeof(glf.Options)
