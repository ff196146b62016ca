"""The weighted fit's C-ABI (glf_graph_normal_equations, glf_fit_coeffs): exported by libglf.so, declared in include/glf.h, listed in
glf.EXPORTS; without a handle glf_graph_normal_equations answers GLF_ERR_INVALID before any device work; and glf_fit_coeffs, which is
host only, against numpy.linalg.solve. CPU only.

Tolerance of the coefficients: rel-L2 <= 1e-12, tests/test_graph_abi.py's TOL. The matrices are that file's G = I + 0.1 B B^T / m
(condition number below 2) plus a non-negative diagonal below 1, so the condition number stays below 3; a backward-stable solve of
an m x m system errs by about m 2^-53 cond ~ 7e-14 at m = 200, and the bound leaves a decade over that. That numpy itself stays
inside the bound is checked too, by the residual of its solution evaluated in extended precision."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glf
from test_graph_abi import TOL, _case, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_graph_normal_equations", "glf_fit_coeffs")


def test_fit_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    chain = re.search(r"#define\s+GLF_GRAPH_NORMAL_CHAIN\s+(\d+)\b", header)
    assert chain and int(chain.group(1)) == glf.GRAPH_NORMAL_CHAIN
    assert 1 <= glf.GRAPH_NORMAL_CHAIN <= 256
    assert callable(glf.fit_coeffs)
    for method in ("normal_equations", "fit"):
        assert hasattr(glf.Graph, method), method


def test_normal_equations_without_a_handle_is_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    one = C.c_void_p(1)
    buf = (C.c_double * 64)()
    for nplanes in (-1, 0, 1, 4, 5):
        assert lib.glf_graph_normal_equations(None, one, C.c_int(nplanes), one, buf, buf) == glf.ERR_INVALID, nplanes
        assert lib.glf_graph_normal_equations(None, None, C.c_int(nplanes), None, None, None) == glf.ERR_INVALID, nplanes


def _system(m, nrhs, seed):
    _, G, _, _ = _case(m, seed)
    rng = np.random.default_rng(seed + 7)
    return G, rng.uniform(0.0, 1.0, m), rng.normal(size=(nrhs, m)) * 100.0


@pytest.mark.parametrize("m", [1, 8, 37, 200])
@pytest.mark.parametrize("nrhs", [1, 4])
@pytest.mark.parametrize("with_penalty", [True, False])
def test_fit_coeffs_against_numpy(m, nrhs, with_penalty):
    G, pen, b = _system(m, nrhs, 100 * m + nrhs)
    penalty = pen if with_penalty else None
    A = G + (np.diag(pen) if with_penalty else 0.0)
    a = glf.fit_coeffs(G, b, penalty)
    want = np.linalg.solve(A, b.T).T
    assert a.shape == (nrhs, m)
    for k in range(nrhs):
        err = _rel(a[k], want[k])
        print("m %d nrhs %d penalty %s row %d: rel-L2 %.2e" % (m, nrhs, with_penalty, k, err))
        assert err <= TOL, err
        # numpy alone stays inside the bound: |x - x*| <= |A^-1| |b - A x|, the residual in extended precision, |A^-1|_2 <= 1
        # (A = I + a positive semi-definite matrix)
        ld = np.longdouble
        res = (b[k].astype(ld) - A.astype(ld) @ want[k].astype(ld)).astype(np.float64)
        assert float(np.linalg.norm(res) / np.linalg.norm(want[k])) <= TOL
        alone = glf.fit_coeffs(G, b[k], penalty)                                  # the rows of b are independent
        assert alone.shape == (m,)
        np.testing.assert_array_equal(alone, a[k])


def _raw(m, G, penalty, nrhs, b, a):
    return glf._lib.glf_fit_coeffs(C.c_uint(m), glf._ptr(G), glf._ptr(penalty), C.c_int(nrhs), glf._ptr(b), glf._ptr(a))


def test_fit_coeffs_refusals_leave_a_untouched():
    m = 8
    G, pen, b = _system(m, 2, 1)
    fill = np.full((2, m), 12345.0)
    a = fill.copy()
    assert _raw(m, G, pen, 2, b, a) == glf.OK and not np.array_equal(a, fill)
    indefinite = np.eye(m)
    indefinite[5, 5] = -1.0
    with_nan = G.copy()
    with_nan[2, 5] = np.nan
    nan_diag = G.copy()
    nan_diag[m - 1, m - 1] = np.nan
    cases = {"G NULL": (m, None, pen, 2, b), "b NULL": (m, G, pen, 2, None), "m = 0": (0, G, pen, 2, b), "nrhs = 0": (m, G, pen, 0, b),
             "nrhs < 0": (m, G, pen, -1, b), "indefinite": (m, indefinite, None, 2, b), "singular": (m, np.zeros((m, m)), None, 2, b),
             "NaN entry": (m, with_nan, pen, 2, b), "NaN on the diagonal": (m, nan_diag, None, 2, b)}
    for what, (mm, GG, pp, nr, bb) in cases.items():
        a = fill.copy()
        assert _raw(mm, GG, pp, nr, bb, a) == glf.ERR_INVALID, what
        np.testing.assert_array_equal(a, fill, err_msg=what)
    assert _raw(m, G, pen, 2, b, None) == glf.ERR_INVALID                        # a NULL
    assert _raw(m, np.zeros((m, m)), np.ones(m), 2, b, fill.copy()) == glf.OK    # (the penalty alone makes it definite)
    for bad in (indefinite, np.zeros((m, m)), with_nan):
        with pytest.raises(glf.GlfError) as e:
            glf.fit_coeffs(bad, b)
        assert e.value.status == glf.ERR_INVALID
    with pytest.raises(ValueError):
        glf.fit_coeffs(G, np.zeros((2, m + 1)))
    with pytest.raises(ValueError):
        glf.fit_coeffs(G, b, np.zeros(m + 1))
