"""The testable Nystroem stage's C-ABI (glf_Nystroem_ex): exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS;
glf_nystroem_info has the layout the header states; the argument types are the header's; and without a context or its matrices
the call answers GLF_ERR_INVALID before any device work. CPU only."""
import ctypes as C
import os
import re

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def _header():
    return open(os.path.join(ROOT, "include", "glf.h")).read()


def test_entry_point_is_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    assert hasattr(lib, "glf_Nystroem_ex") and hasattr(lib, "glf_Nystroem")
    assert "glf_Nystroem_ex" in glf.EXPORTS
    assert re.search(r"\bint\s+glf_Nystroem_ex\s*\(", _header())
    assert hasattr(glf.Context, "Nystroem_ex")


def test_info_layout_matches_the_header():
    body = re.search(r"typedef\s+struct\s+glf_nystroem_info\s*\{(.*?)\}\s*glf_nystroem_info\s*;", _header(), flags=re.S)
    assert body
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for decl in text.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    assert fields == list(glf.NystroemInfo._fields_)
    assert [n for n, _ in fields] == ["path", "contraction", "skipping", "lut", "row0", "row1", "entries_evaluated"]
    assert C.sizeof(glf.NystroemInfo) == 32
    assert [getattr(glf.NystroemInfo, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20, 24]


def test_argument_types_match_the_header():
    proto = re.search(r"\bint\s+glf_Nystroem_ex\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert proto
    args = [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]
    assert args == ["glf_ctx *ctx", "const glf_mat *B", "const glf_mat *phi_A", "const glf_mat *Pi_A_Inv", "int skip_exact_zeros",
                    "unsigned row0", "unsigned row1", "glf_mat *phi", "glf_nystroem_info *info"]
    want = [C.c_int if a.startswith("int ") else C.c_uint if a.startswith("unsigned ") else C.c_void_p for a in args]
    assert glf._lib.glf_Nystroem_ex.argtypes == want


def test_calls_without_a_context_or_matrices_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    lib.glf_Nystroem_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    lib.glf_Nystroem.argtypes = [C.c_void_p] * 5
    B, phi_A, pinv, phi = glf.Mat(kind=glf.MAT_KERNEL_B), glf.Mat(), glf.Mat(), glf.Mat(rows=77)
    info = glf.NystroemInfo(path=77)
    assert lib.glf_Nystroem_ex(None, C.byref(B), C.byref(phi_A), C.byref(pinv), 0, 0, 0, C.byref(phi), C.byref(info)) == glf.ERR_INVALID
    assert lib.glf_Nystroem_ex(None, None, None, None, 1, 2, 3, None, None) == glf.ERR_INVALID
    assert lib.glf_Nystroem(None, C.byref(B), C.byref(phi_A), C.byref(pinv), C.byref(phi)) == glf.ERR_INVALID
    assert lib.glf_Nystroem(None, None, None, None, None) == glf.ERR_INVALID
    assert info.path == 77 and phi.rows == 77 and not phi.data
