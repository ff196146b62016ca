"""CPU-side checks of the softmax read-out's boundary: glf_graph_softmax is exported by libglf.so, declared in include/glf.h and
listed in glf.EXPORTS, Graph has the three methods, and a NULL handle is refused before anything is touched. No device compute."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+glf_graph_softmax\s*\(", code)
    assert re.search(r"#define\s+GLF_SOFTMAX_MAX\s+32\b", code)
    assert hasattr(C.CDLL(glf.LIB_PATH), "glf_graph_softmax")
    assert "glf_graph_softmax" in glf.EXPORTS
    assert glf.SOFTMAX_MAX == 32 == glf.CLASSIFY_MAX == glf.GRAPH_MAX_OUTPUTS
    assert len(glf._lib.glf_graph_softmax.argtypes) == 12 and glf._lib.glf_graph_softmax.argtypes[8] is C.c_double


def test_graph_methods_exist():
    sig = inspect.signature(glf.Graph.softmax)
    assert list(sig.parameters)[1:] == ["coeffs", "ident", "plane", "planes", "bias", "beta", "want"]
    assert sig.parameters["beta"].default == 1.0 and sig.parameters["want"].default == ("prob",)
    sig = inspect.signature(glf.Graph.soft_assign)
    assert list(sig.parameters)[1:] == ["centres", "scale", "temperature", "want"]
    sig = inspect.signature(glf.Graph.mean_field)
    assert list(sig.parameters)[1:] == ["logits", "coupling", "compat", "response", "weight", "exclude_samples", "beta", "ident", "max_iter",
                                        "tol", "init", "want"]
    assert (sig.parameters["max_iter"].default, sig.parameters["tol"].default, sig.parameters["exclude_samples"].default) == (10, 1e-4, True)


def test_null_handle_is_refused():
    a = np.zeros((2, 8), dtype=np.float64)
    plane = np.full(2, -1, dtype=np.int32)
    rc = glf._lib.glf_graph_softmax(None, C.c_int(2), glf._ptr(a), None, glf._ptr(plane), C.c_int(0), None, None, C.c_double(1.0), None, None, None)
    assert rc == glf.ERR_INVALID
