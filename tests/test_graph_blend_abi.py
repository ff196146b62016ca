"""CPU-side checks of the blend read-out's boundary: glf_graph_blend is exported by libglf.so, declared in include/glf.h with the
argument list that glf.py gives ctypes, and listed in glf.EXPORTS; GLF_BLEND_MAX_SLOTS is the header's; Graph has the four methods;
a NULL handle is refused before anything is touched. No device compute."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration():
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.search(r"\bint\s+glf_graph_blend\s*\(([^)]*)\)\s*;", code)
    assert found
    return code, [" ".join(arg.split()) for arg in found.group(1).split(",")]


def test_symbol_is_exported_declared_and_listed():
    code, args = _declaration()
    assert re.search(r"#define\s+GLF_BLEND_MAX_SLOTS\s+32\b", code)
    assert hasattr(C.CDLL(glf.LIB_PATH), "glf_graph_blend")
    assert "glf_graph_blend" in glf.EXPORTS
    assert glf.BLEND_MAX_SLOTS == 32 == glf.GRAPH_MAX_OUTPUTS == glf.CLASSIFY_MAX == glf.SOFTMAX_MAX


def test_argument_types_are_the_headers():
    _, args = _declaration()
    assert args == ["glf_graph *g", "int nout", "int nlevels", "const double *h_a", "const float *ident", "const int *plane", "int nplanes",
                    "const float *d_planes", "const float *d_level", "float *d_out"]
    want = [C.c_int if arg.startswith("int ") else C.c_void_p for arg in args]
    assert list(glf._lib.glf_graph_blend.argtypes) == want


def test_graph_methods_exist():
    sig = inspect.signature(glf.Graph.blend)
    assert list(sig.parameters)[1:] == ["coeffs", "level", "ident", "plane", "planes", "out"]
    assert all(sig.parameters[key].default is None for key in ("ident", "plane", "planes", "out"))
    sig = inspect.signature(glf.Graph.apply_local)
    assert list(sig.parameters)[1:] == ["planes", "level", "weights", "ident"] and sig.parameters["ident"].default == 1.0
    sig = inspect.signature(glf.Graph.gather)
    assert list(sig.parameters)[1:3] == ["coeffs", "labels"]
    sig = inspect.signature(glf.Graph.fit_piecewise)
    assert list(sig.parameters)[1:] == ["planes", "labels", "k", "weight", "smooth", "ridge"]
    assert (sig.parameters["weight"].default, sig.parameters["smooth"].default, sig.parameters["ridge"].default) == (None, 0.0, 0.0)


def test_null_handle_is_refused():
    a = np.zeros((2, 8), dtype=np.float64)
    plane = np.full(2, -1, dtype=np.int32)
    rc = glf._lib.glf_graph_blend(None, C.c_int(1), C.c_int(2), glf._ptr(a), None, glf._ptr(plane), C.c_int(0), None, None, None)
    assert rc == glf.ERR_INVALID
