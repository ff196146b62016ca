"""The operator sweep's C-ABI (glf_operator_create, glf_operator_apply, glf_operator_solve, glf_operator_stored, glf_operator_destroy):
exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS; glf_operator_info and glf_solve_info have the layout the
header states; and without a context or a handle the calls answer GLF_ERR_INVALID (destroy: GLF_OK) before any device work. CPU only."""
import ctypes as C
import os
import re

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_operator_create", "glf_operator_apply", "glf_operator_solve", "glf_operator_stored", "glf_operator_destroy")


def test_operator_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"typedef\s+struct\s+glf_operator\s+glf_operator\s*;", header)
    assert hasattr(glf.Context, "operator")
    for method in ("apply", "apply_numpy", "solve", "solve_numpy", "stored", "close"):
        assert hasattr(glf.Operator, method), method


def test_operator_info_layout_matches_the_header():
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    body = re.search(r"typedef\s+struct\s+glf_operator_info\s*\{(.*?)\}\s*glf_operator_info\s*;", header, flags=re.S)
    assert body
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for decl in text.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            assert ctype == "int32_t", decl
            fields += [n.strip() for n in names.split(",")]
    assert fields == [name for name, _ in glf.OperatorInfo._fields_] == ["path", "ksplit", "skipping", "row0", "row1"]
    assert all(t is C.c_int32 for _, t in glf.OperatorInfo._fields_)
    assert C.sizeof(glf.OperatorInfo) == 20
    assert [getattr(glf.OperatorInfo, n).offset for n in fields] == [0, 4, 8, 12, 16]


def test_solve_info_layout_matches_the_header():
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    body = re.search(r"typedef\s+struct\s+glf_solve_info\s*\{(.*?)\}\s*glf_solve_info\s*;", header, flags=re.S)
    assert body
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for decl in text.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            assert ctype == "int32_t", decl
            fields += [n.strip() for n in names.split(",")]
    assert fields == [name for name, _ in glf.SolveInfo._fields_] == ["iters", "unconverged", "matvecs", "narrow_sweeps", "path", "reserved"]
    assert all(t is C.c_int32 for _, t in glf.SolveInfo._fields_)
    assert C.sizeof(glf.SolveInfo) == 24
    assert [getattr(glf.SolveInfo, n).offset for n in fields] == [0, 4, 8, 12, 16, 20]
    assert re.search(r"\bint\s+glf_operator_solve\s*\(\s*glf_operator\s*\*op,\s*const\s+glf_mat\s*\*B,\s*glf_mat\s*\*X,\s*glf_mat\s*\*R", header)


def test_calls_without_a_context_or_a_handle_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    lib.glf_operator_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    lib.glf_operator_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.glf_operator_stored.argtypes = [C.c_void_p, C.c_void_p]
    lib.glf_operator_destroy.argtypes = [C.c_void_p]
    desc, x, y, info = glf.Mat(kind=glf.MAT_KERNEL_B), glf.Mat(), glf.Mat(), glf.OperatorInfo(path=77)
    handle = C.c_void_p(12345)
    assert lib.glf_operator_create(None, C.byref(desc), 0, 0, 9, 32, C.byref(handle)) == glf.ERR_INVALID
    assert handle.value == 12345                                  # (nothing to report through without a context)
    assert lib.glf_operator_create(None, None, 0, 0, 0, 0, None) == glf.ERR_INVALID
    assert lib.glf_operator_apply(None, C.byref(x), C.byref(y), C.byref(info)) == glf.ERR_INVALID
    assert lib.glf_operator_apply(None, None, None, None) == glf.ERR_INVALID
    assert info.path == 77
    lib.glf_operator_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_double, C.c_int, C.c_void_p]
    sinfo = glf.SolveInfo(iters=55)
    assert lib.glf_operator_solve(None, C.byref(x), C.byref(y), None, 1, 1e-5, 10, C.byref(sinfo)) == glf.ERR_INVALID
    assert lib.glf_operator_solve(None, None, None, None, 0, 0.0, 0, None) == glf.ERR_INVALID
    assert sinfo.iters == 55
    assert lib.glf_operator_stored(None, C.byref(x)) == glf.ERR_INVALID
    assert lib.glf_operator_destroy(None) == glf.OK
