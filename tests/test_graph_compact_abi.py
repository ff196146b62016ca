"""CPU-side checks of the compact graph handle's boundary (glf_graph_compact, glf_graph_storage, glf_graph_dequantize): the three
symbols are exported, declared in include/glf.h and listed in glf.EXPORTS, the enum values match, the Graph methods exist, and a
NULL handle is refused with GLF_ERR_INVALID before any device work. No device here."""
import ctypes as C
import os
import re

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("glf_graph_compact", "glf_graph_storage", "glf_graph_dequantize")


def _header():
    return open(os.path.join(ROOT, "include", "glf.h")).read()


def test_symbols_exported_declared_and_listed():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(glf.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in glf.EXPORTS, name
    assert re.search(r"int\s+glf_graph_compact\s*\(\s*glf_graph\s*\*\s*g\s*,\s*int\s+storage\s*\)", code)
    assert re.search(r"int\s+glf_graph_storage\s*\(\s*const\s+glf_graph\s*\*\s*g\s*,\s*int\s*\*\s*storage\s*,\s*int32_t\s*\*\s*h_exponent\s*\)", code)
    assert re.search(r"int\s+glf_graph_dequantize\s*\(\s*glf_graph\s*\*\s*g\s*,\s*float\s*\*\s*d_out\s*\)", code)


def test_enum_values_match():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"enum\s*\{\s*GLF_PHI_F32\s*=\s*(\d+)\s*,\s*GLF_PHI_F16\s*=\s*(\d+)\s*\}", code)
    assert m, "enum { GLF_PHI_F32, GLF_PHI_F16 } not declared"
    assert (int(m.group(1)), int(m.group(2))) == (glf.PHI_F32, glf.PHI_F16) == (0, 1)


def test_graph_methods_exist():
    for name in ("compact", "column_exponents", "dequantize"):
        assert callable(getattr(glf.Graph, name)), name
    assert isinstance(glf.Graph.storage, property)


def test_null_handle_is_refused():
    storage = C.c_int(-7)
    expo = (C.c_int32 * 4)(9, 9, 9, 9)
    out = (C.c_float * 4)()
    for st in (glf.PHI_F32, glf.PHI_F16, 5):
        assert glf._lib.glf_graph_compact(None, C.c_int(st)) == glf.ERR_INVALID
    assert glf._lib.glf_graph_storage(None, C.byref(storage), expo) == glf.ERR_INVALID
    assert storage.value == -7 and list(expo) == [9, 9, 9, 9]                    # nothing written
    assert glf._lib.glf_graph_storage(None, None, None) == glf.ERR_INVALID
    assert glf._lib.glf_graph_dequantize(None, out) == glf.ERR_INVALID
    assert glf._lib.glf_graph_dequantize(None, None) == glf.ERR_INVALID
