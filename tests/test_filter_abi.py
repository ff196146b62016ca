"""The testable filter stage's C-ABI (glf_Filter_ex): exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS;
glf_filter_request and glf_filter_info have the layout the header states; the GLF_FK_* bits are the header's; and without a context or a
request the call answers GLF_ERR_INVALID before any device work and leaves the info as it was. CPU only."""
import ctypes as C
import os
import re

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}


def _header():
    return open(os.path.join(ROOT, "include", "glf.h")).read()


def _fields(name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _header(), flags=re.S)
    assert body
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for decl in text.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:                                            # every pointer travels as a void pointer
            fields.append((decl.split("*")[-1].strip(), C.c_void_p))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    return fields


def test_entry_point_is_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    assert hasattr(lib, "glf_Filter_ex")
    assert "glf_Filter_ex" in glf.EXPORTS
    assert re.search(r"\bint\s+glf_Filter_ex\s*\(\s*glf_ctx \*ctx,\s*const glf_filter_request \*rq,\s*glf_filter_info \*info\s*\)\s*;", _header())
    assert hasattr(glf.Context, "Filter_ex")
    assert glf._lib.glf_Filter_ex.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]


def test_request_layout_matches_the_header():
    fields = _fields("glf_filter_request")
    assert fields == list(glf.FilterRequest._fields_)
    assert [n for n, _ in fields] == ["struct_size", "pix", "d_img", "width", "height", "phi", "lam", "filter_mode", "filter_pow", "filter_beta",
                                      "gain", "row0", "row1", "nsig", "reserved_", "d_sig", "d_sig_out", "h_c_in", "h_c_out", "h_gram_out",
                                      "d_out", "d_zf", "d_corr"]
    assert C.sizeof(glf.FilterRequest) == 136
    assert [getattr(glf.FilterRequest, n).offset for n, _ in fields] == [0, 4, 8, 16, 20, 24, 32, 40, 44, 48, 52, 56, 60, 64, 68, 72, 80, 88, 96,
                                                                         104, 112, 120, 128]


def test_info_layout_and_kernel_bits_match_the_header():
    fields = _fields("glf_filter_info")
    assert fields == list(glf.FilterInfo._fields_)
    assert [n for n, _ in fields] == ["struct_size", "kernels", "ld", "panels", "proj_blocks", "apply_blocks", "grid_strided", "reserved_",
                                      "pix0", "pix1"]
    assert C.sizeof(glf.FilterInfo) == 48
    assert [getattr(glf.FilterInfo, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    bits = dict((k, int(v)) for k, v in re.findall(r"\b(GLF_FK_\w+)\s*=\s*(\d+)", _header()))
    assert bits == {"GLF_FK_" + k[3:]: getattr(glf, k) for k in dir(glf) if k.startswith("FK_")}
    assert sorted(bits.values()) == [1 << i for i in range(11)]


def test_calls_without_a_context_or_a_request_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    lib.glf_Filter_ex.argtypes = glf._lib.glf_Filter_ex.argtypes
    info = glf.FilterInfo(struct_size=C.sizeof(glf.FilterInfo), kernels=77)
    rq = glf.FilterRequest(struct_size=C.sizeof(glf.FilterRequest))
    assert lib.glf_Filter_ex(None, C.byref(rq), C.byref(info)) == glf.ERR_INVALID
    assert lib.glf_Filter_ex(None, None, None) == glf.ERR_INVALID
    assert info.kernels == 77
