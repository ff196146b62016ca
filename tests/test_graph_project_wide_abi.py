"""The wide projection's C-ABI (glf_graph_project_wide): exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS;
GLF_GRAPH_MAX_PLANES of the header against glf.GRAPH_MAX_PLANES; Graph.project_wide exists; and without a handle the call answers
GLF_ERR_INVALID before any device work, whatever nplanes is, and leaves h_c untouched. CPU only."""
import ctypes as C
import os
import re

import numpy as np

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "glf_graph_project_wide"


def test_project_wide_is_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    assert hasattr(lib, NAME)
    assert NAME in glf.EXPORTS
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    planes = re.search(r"#define\s+GLF_GRAPH_MAX_PLANES\s+(\d+)\b", header)
    assert planes and int(planes.group(1)) == glf.GRAPH_MAX_PLANES == 32
    assert hasattr(glf.Graph, "project_wide") and callable(glf.Graph.project_wide)


def test_project_wide_without_a_handle_is_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    fn = getattr(lib, NAME)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    one = C.c_void_p(1)
    fill = np.full(64, 12345.0)
    for nplanes in (-1, 0, 1, 32, 33):
        buf = fill.copy()
        assert fn(None, one, nplanes, one, glf._ptr(buf)) == glf.ERR_INVALID, nplanes
        assert fn(None, None, nplanes, one, glf._ptr(buf)) == glf.ERR_INVALID, nplanes
        assert fn(None, None, nplanes, None, None) == glf.ERR_INVALID, nplanes
        np.testing.assert_array_equal(buf, fill)
