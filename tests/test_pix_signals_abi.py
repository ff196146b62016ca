"""Joint filtering under a colour or 16-bit guide (glf_image_processing_rgb_signals, glf_image_processing_u16_signals and their
glf_multi_ counterparts): exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS, and their argument checks answer
GLF_ERR_INVALID before any device work. CPU only."""
import ctypes as C
import os
import re

import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = ("glf_image_processing_rgb_signals", "glf_image_processing_u16_signals")
MULTI = ("glf_multi_image_processing_rgb_signals", "glf_multi_image_processing_u16_signals")


def test_pix_signal_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in SINGLE + MULTI:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+GLF_MAX_SIGNALS\s+4\b", header) and glf.MAX_SIGNALS == 4
    for cls in (glf.Context, glf.Multi):
        assert hasattr(cls, "image_processing_rgb_signals") and hasattr(cls, "image_processing_u16_signals")


def _call(lib, name, handle, nsig, sig, sig_out):
    return getattr(lib, name)(handle, None, C.c_void_p(1), C.c_int(8), C.c_int(8), C.c_int(nsig), C.c_void_p(sig), C.c_void_p(sig_out),
                              C.c_void_p(1), None, None, None)


@pytest.mark.parametrize("name", SINGLE + MULTI)
@pytest.mark.parametrize("nsig,sig,sig_out", [(1, 1, 1), (0, 1, 1), (5, 1, 1), (-1, 1, 1), (2, None, 1), (2, 1, None)])
def test_null_handle_is_invalid_without_a_device(name, nsig, sig, sig_out):
    """Without a context / world every call is GLF_ERR_INVALID before any device work, whatever the other arguments (the nsig and
    plane-pointer checks with a live context are in tests/test_gpu_pix_signals.py)."""
    lib = C.CDLL(glf.LIB_PATH)
    assert _call(lib, name, None, nsig, sig, sig_out) == glf.ERR_INVALID
