"""Joint filtering entry points (glf_image_processing_signals, glf_multi_image_processing_signals): exported by libglf.so,
declared in include/glf.h, and their argument checks answer GLF_ERR_INVALID before any device work. CPU only."""
import ctypes as C
import os
import re

import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_image_processing_signals", "glf_multi_image_processing_signals")


def test_signal_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+GLF_MAX_SIGNALS\s+4\b", header) and glf.MAX_SIGNALS == 4


def _single(lib, ctx, nsig, sig, sig_out, img=1, out=1):
    return lib.glf_image_processing_signals(ctx, None, C.c_void_p(img), C.c_int(8), C.c_int(8), C.c_int(nsig), C.c_void_p(sig),
                                            C.c_void_p(sig_out), C.c_void_p(out), None, None, None)


def _multi(lib, w, nsig, sig, sig_out):
    return lib.glf_multi_image_processing_signals(w, None, C.c_void_p(1), C.c_int(8), C.c_int(8), C.c_int(nsig), C.c_void_p(sig),
                                                  C.c_void_p(sig_out), C.c_void_p(1), None, None, None)


@pytest.mark.parametrize("nsig,sig,sig_out", [(1, 1, 1), (0, 1, 1), (5, 1, 1), (-1, 1, 1), (2, None, 1), (2, 1, None)])
def test_null_handle_is_invalid_without_a_device(nsig, sig, sig_out):
    """Without a context / world every call is GLF_ERR_INVALID before any device work, whatever the other arguments (the nsig and
    plane-pointer checks with a live context and world are in tests/test_gpu_signals.py and tests/test_gpu_signals_multi.py)."""
    lib = C.CDLL(glf.LIB_PATH)
    assert _single(lib, None, nsig, sig, sig_out) == glf.ERR_INVALID
    assert _multi(lib, None, nsig, sig, sig_out) == glf.ERR_INVALID
