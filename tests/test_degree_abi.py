"""The testable degree stage's C-ABI (glf_Degree_ex): exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS;
glf_degree_info has the layout the header states; the argument types are the header's; and without a context, an image or an output the
call answers GLF_ERR_INVALID before any device work and leaves the outputs as they were. CPU only."""
import ctypes as C
import os
import re

import numpy as np

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def _header():
    return open(os.path.join(ROOT, "include", "glf.h")).read()


def test_entry_point_is_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    assert hasattr(lib, "glf_Degree_ex")
    assert "glf_Degree_ex" in glf.EXPORTS
    assert re.search(r"\bint\s+glf_Degree_ex\s*\(", _header())
    assert hasattr(glf.Context, "Degree_ex")


def test_info_layout_matches_the_header():
    body = re.search(r"typedef\s+struct\s+glf_degree_info\s*\{(.*?)\}\s*glf_degree_info\s*;", _header(), flags=re.S)
    assert body
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for decl in text.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    assert fields == list(glf.DegreeInfo._fields_)
    assert [n for n, _ in fields] == ["struct_size", "path", "shape", "skipping", "chunks", "mgroups", "row0", "row1", "entries_evaluated"]
    assert C.sizeof(glf.DegreeInfo) == 40
    assert [getattr(glf.DegreeInfo, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert (glf.DEG_DENSE, glf.DEG_GRID, glf.DEG_WINDOWED, glf.DEG_ENTRYWISE, glf.DEG_NLM) == (0, 1, 2, 5, 6)
    assert (glf.DEG_FIVES, glf.DEG_TEN, glf.DEG_WINDOW) == (0, 1, 2)


def test_argument_types_match_the_header():
    proto = re.search(r"\bint\s+glf_Degree_ex\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert proto
    args = [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]
    assert args == ["glf_ctx *ctx", "const void *d_img", "int width", "int height", "unsigned sample_size", "const unsigned *sample_indices",
                    "int kernel", "float h_loc", "float h_val", "int skip_exact_zeros", "unsigned row0", "unsigned row1",
                    "const float *d_plane", "double *h_degree", "double *h_ysum", "glf_degree_info *info"]
    want = [C.c_int if a.startswith("int ") else C.c_uint if a.startswith("unsigned ") else C.c_float if a.startswith("float ") else C.c_void_p
            for a in args]
    assert glf._lib.glf_Degree_ex.argtypes == want


def test_calls_without_a_context_image_or_output_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    lib.glf_Degree_ex.argtypes = glf._lib.glf_Degree_ex.argtypes
    idx = np.arange(4, dtype=np.uint32)
    deg = np.full(4, 77.0)
    info = glf.DegreeInfo(struct_size=C.sizeof(glf.DegreeInfo), path=77)
    args = (8, 8, 4, idx.ctypes.data_as(C.c_void_p), glf.KERNEL_BILATERAL, 40.0, 30.0, 0, 0, 0, None)
    assert lib.glf_Degree_ex(None, C.c_void_p(16), *args, deg.ctypes.data_as(C.c_void_p), None, C.byref(info)) == glf.ERR_INVALID
    assert lib.glf_Degree_ex(None, None, *args, None, None, None) == glf.ERR_INVALID
    assert info.path == 77 and (deg == 77.0).all()
