"""The graph handle's C-ABI (glf_graph_build / _destroy / _get_info / _eigenvalues / _gram / _project / _synthesize and
glf_filter_coeffs): exported by libglf.so, declared in include/glf.h, listed in glf.EXPORTS; without a context or a handle every call
answers GLF_ERR_INVALID before any device work; and glf_filter_coeffs, which is host only, against the fp64 numpy restatement
tests/rgb_ref.weights. CPU only.

Tolerance of the coefficients: rel-L2 <= 1e-12. The sharpening weights are three chained m-term f64 products (L G L c, then L G of
that): gamma ~ 3 m 2^-53 = 1.2e-14 at m = 37, and the margin covers the cancellation in (1 + beta) u - beta v. That numpy itself
stays inside the bound is checked here too, by evaluating the same expression in extended precision."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glf
import rgb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_graph_build", "glf_graph_destroy", "glf_graph_get_info", "glf_graph_eigenvalues", "glf_graph_gram", "glf_graph_project",
         "glf_graph_synthesize", "glf_filter_coeffs")
MODES = {"reference": glf.FILTER_REFERENCE, "poc": glf.FILTER_POC, "smooth": glf.FILTER_SMOOTH, "sharpen": glf.FILTER_SHARPEN}
TOL = 1e-12


def test_graph_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+GLF_GRAPH_MAX_OUTPUTS\s+32\b", header) and glf.GRAPH_MAX_OUTPUTS == 32
    for k, name in enumerate(("U8", "RGB8", "U16", "F32", "RGBF32")):
        assert re.search(r"\bGLF_PIX_%s\s*=\s*%d\b" % (name, k), header) and getattr(glf, "PIX_" + name) == k
    assert re.search(r"typedef\s+struct\s+glf_graph\s+glf_graph\s*;", header)
    assert callable(glf.Context.graph) and callable(glf.filter_coeffs)
    for method in ("project", "synthesize", "apply", "gram", "close", "__enter__", "__exit__"):
        assert hasattr(glf.Graph, method), method


def test_null_context_or_handle_is_invalid_without_a_device():
    """Without a context / a handle every call is GLF_ERR_INVALID before any device work, whatever the other arguments (the
    checks with a live handle are in tests/test_gpu_graph.py); destroying no handle is not an error."""
    lib = C.CDLL(glf.LIB_PATH)
    one = C.c_void_p(1)
    for pix in (0, 4, 7):
        handle = C.c_void_p(0xdead)
        assert lib.glf_graph_build(None, None, C.c_int(pix), one, C.c_int(8), C.c_int(8), C.byref(handle), None) == glf.ERR_INVALID
        assert not handle.value                                                   # *graph = NULL
    assert lib.glf_graph_build(None, None, C.c_int(0), one, C.c_int(8), C.c_int(8), None, None) == glf.ERR_INVALID
    gi = glf.GraphInfo(struct_size=C.sizeof(glf.GraphInfo))
    buf = (C.c_double * 64)()
    idn, pl = (C.c_float * 32)(), (C.c_int * 32)()
    assert lib.glf_graph_get_info(None, C.byref(gi)) == glf.ERR_INVALID
    assert lib.glf_graph_get_info(None, None) == glf.ERR_INVALID
    assert lib.glf_graph_eigenvalues(None, buf) == glf.ERR_INVALID
    assert lib.glf_graph_gram(None, buf) == glf.ERR_INVALID
    for nplanes in (1, 0, 5):
        assert lib.glf_graph_project(None, C.c_int(nplanes), one, buf) == glf.ERR_INVALID
    for nout in (1, 0, 33):
        assert lib.glf_graph_synthesize(None, C.c_int(nout), buf, idn, pl, C.c_int(1), one, one) == glf.ERR_INVALID
    assert lib.glf_graph_synthesize(None, C.c_int(1), None, None, None, C.c_int(0), None, None) == glf.ERR_INVALID
    assert lib.glf_graph_destroy(None) == glf.OK


def _case(m, seed):
    rng = np.random.default_rng(seed)
    lam = rng.uniform(0.0, 1.0, m)
    lam = np.where(lam > 0.0, lam, 0.5)                                          # (0, 1), open at 0
    B = rng.normal(size=(m, m))
    G = np.eye(m) + 0.1 * (B @ B.T) / m
    R = np.linalg.cholesky(G).T                                                   # a "Phi" whose Gram matrix is G: rgb_ref.weights forms Phi^T Phi
    G = R.T @ R                                                                   # (the matrix both sides use, bit for bit)
    return lam, G, R, rng.normal(size=m) * 100.0


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("m", [1, 8, 37])
@pytest.mark.parametrize("filter_pow", [1, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_filter_coeffs_against_numpy(mode, filter_pow, m):
    lam, G, R, c = _case(m, 100 * m + filter_pow)
    opt = glf.default_options(filter_mode=MODES[mode], filter_pow=filter_pow, gain=2.5, filter_beta=1.5)
    a, ident = glf.filter_coeffs(opt, lam, c, gram=G)
    if mode == "reference":                                                       # rgb_ref.weights is f(Pi) c with f = Pi: times the gain, Pi^pow
        want = float(opt.gain) * rgb_ref.weights(R, lam ** filter_pow, MODES[mode], c)
    else:
        want = rgb_ref.weights(R, lam, MODES[mode], c, beta=1.5)
    err = _rel(a, want)
    print("%s pow %d m %d: rel-L2 %.2e" % (mode, filter_pow, m, err))
    assert a.shape == (m,) and err <= TOL, err
    assert ident == (1.0 if mode in ("reference", "poc") else 0.0)
    if mode == "sharpen":                                                         # numpy alone stays inside the bound
        ld = np.longdouble
        s, Gl, cl = (1.0 - lam).astype(ld), G.astype(ld), c.astype(ld)
        u = s * (Gl @ (s * cl))
        v = s * (Gl @ u)
        wide = ((ld(1.0) + ld(1.5)) * u - ld(1.5) * v).astype(np.float64)
        assert _rel(want, wide) <= TOL
    a2, _ = glf.filter_coeffs(opt, lam, np.stack([c, 2.0 * c]), gram=G)           # rows of c are independent planes
    np.testing.assert_array_equal(a2[0], a)


def test_filter_coeffs_refusals():
    lam, G, _, c = _case(8, 1)
    a, ident = np.zeros(8), C.c_float()

    def call(opt, gram=G, lam_=lam, c_=c, a_=a, ident_=ident):
        return glf._lib.glf_filter_coeffs(C.byref(opt) if opt is not None else None, C.c_uint(8), glf._ptr(lam_), glf._ptr(gram), glf._ptr(c_),
                                          glf._ptr(a_), C.byref(ident_) if ident_ is not None else None)

    assert call(glf.default_options(filter_mode=glf.FILTER_SHARPEN)) == glf.OK
    assert call(glf.default_options(filter_mode=glf.FILTER_SHARPEN), gram=None) == glf.ERR_INVALID
    assert call(glf.default_options(filter_mode=glf.FILTER_SMOOTH), gram=None) == glf.OK       # (the other modes do not read it)
    assert call(None) == glf.OK                                                                # the default options
    bad = glf.default_options()
    bad.struct_size += 4
    assert call(bad) == glf.ERR_INVALID
    for mode in (-1, 4, 99):
        assert call(glf.default_options(filter_mode=mode)) == glf.ERR_INVALID, mode
    for kw in (dict(lam_=None), dict(c_=None), dict(a_=None), dict(ident_=None)):
        assert call(glf.default_options(), **kw) == glf.ERR_INVALID, kw
    with pytest.raises(glf.GlfError):
        glf.filter_coeffs(glf.default_options(filter_mode=glf.FILTER_SHARPEN), lam, c)
