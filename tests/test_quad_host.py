"""The host-only half of the per-pixel quadratic forms (glf_fit_factor, through ctypes) and the C-ABI of the section: exported by
libglf.so, declared in include/glf.h, listed in glf.EXPORTS; without a handle the device calls answer GLF_ERR_INVALID before any
device work. CPU only.

Tolerance of the factor: max |R^T (G + P) R - I| <= 1e-12 cond(G + P), for the Gram matrices G = B^T B of seeded random m x m
matrices B and a diagonal P in [0, 1). A backward-stable Cholesky factor has L L^T = M + E with |E| of the order m 2^-53 |M|, so
R^T M R - I = -R^T E R is of the order m 2^-53 cond(M) ~ 3e-14 cond at m = 256: the bound leaves a decade over that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_graph_quadform", "glf_fit_factor", "glf_graph_rows")


def test_quad_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    for macro, value in (("GLF_QUAD_MAX_COLS", glf.QUAD_MAX_COLS), ("GLF_QUAD_MAX_CENTRES", glf.QUAD_MAX_CENTRES)):
        found = re.search(r"#define\s+%s\s+(\d+)\b" % macro, header)
        assert found and int(found.group(1)) == value, macro
    assert (glf.QUAD_MAX_COLS, glf.QUAD_MAX_CENTRES) == (64, 32)
    assert callable(glf.fit_factor)
    for method in ("quadform", "leverage", "fit_loo", "distance", "rows"):
        assert hasattr(glf.Graph, method), method


def test_device_calls_without_a_handle_are_invalid():
    lib = glf._lib
    one = C.c_void_p(1)
    buf = (C.c_double * 64)()
    for r, ncent in ((1, 1), (64, 32), (0, 1), (65, 1), (1, 0), (1, 33)):
        assert lib.glf_graph_quadform(None, C.c_uint(r), buf, C.c_uint(ncent), buf, 0, one) == glf.ERR_INVALID, (r, ncent)
    assert lib.glf_graph_rows(None, C.c_uint(1), buf, buf) == glf.ERR_INVALID


def _system(m, seed):
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(m, m))
    return B.T @ B, rng.uniform(0.0, 1.0, m)


@pytest.mark.parametrize("m", [1, 4, 64, 256])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("with_penalty", [True, False])
def test_fit_factor_identity(m, seed, with_penalty):
    G, pen = _system(m, 1000 * m + seed)
    M = G + (np.diag(pen) if with_penalty else 0.0)
    R = glf.fit_factor(G, pen if with_penalty else None)
    assert R.shape == (m, m)
    assert np.all(np.tril(R, -1) == 0.0) and np.all(np.diag(R) > 0.0)            # L^-T: upper triangular
    ld = np.longdouble
    defect = float(np.abs((R.T.astype(ld) @ M.astype(ld) @ R.astype(ld)).astype(np.float64) - np.eye(m)).max())
    cond = float(np.linalg.cond(M))
    print("m %d seed %d penalty %s: max |R^T M R - I| %.3e, cond %.3e, fraction of the bound %.3e" % (m, seed, with_penalty, defect, cond,
                                                                                                  defect / (1e-12 * cond)))
    assert defect <= 1e-12 * cond
    np.testing.assert_array_equal(glf.fit_factor(G, pen if with_penalty else None), R)   # two calls, the same bits
    # phi^T M^-1 phi = |R^T phi|^2, the identity the leverage rests on, at the same tolerance relative to the value
    phi = np.random.default_rng(seed).normal(size=m)
    want = float(phi @ np.linalg.solve(M, phi))
    got = float(np.sum((R.T @ phi) ** 2))
    assert abs(got - want) <= 1e-12 * cond * want


def _raw(m, G, penalty, R):
    return glf._lib.glf_fit_factor(C.c_uint(m), glf._ptr(G), glf._ptr(penalty), glf._ptr(R))


def test_fit_factor_refusals_leave_R_untouched():
    m = 8
    G, pen = _system(m, 5)
    fill = np.full((m, m), 12345.0)
    R = fill.copy()
    assert _raw(m, G, pen, R) == glf.OK and not np.array_equal(R, fill)
    indefinite = np.eye(m)
    indefinite[5, 5] = -1.0
    with_nan = G.copy()
    with_nan[5, 2] = np.nan
    with_inf = G.copy()
    with_inf[m - 1, m - 1] = np.inf
    nan_pen, inf_pen = pen.copy(), pen.copy()
    nan_pen[3] = np.nan
    inf_pen[0] = np.inf
    cases = {"G NULL": (m, None, pen), "m = 0": (0, G, pen), "indefinite": (m, indefinite, None), "singular": (m, np.zeros((m, m)), None),
             "NaN entry": (m, with_nan, pen), "Inf on the diagonal": (m, with_inf, None), "NaN penalty": (m, G, nan_pen),
             "Inf penalty": (m, G, inf_pen), "a penalty that makes it indefinite": (m, G, np.full(m, -1e6))}
    for what, (mm, GG, pp) in cases.items():
        R = fill.copy()
        assert _raw(mm, GG, pp, R) == glf.ERR_INVALID, what
        np.testing.assert_array_equal(R, fill, err_msg=what)
    assert _raw(m, G, pen, None) == glf.ERR_INVALID                              # a NULL R
    assert _raw(m, np.zeros((m, m)), np.ones(m), fill.copy()) == glf.OK          # (the penalty alone makes it definite)
    for bad in (indefinite, np.zeros((m, m)), with_nan, with_inf):
        with pytest.raises(glf.GlfError) as e:
            glf.fit_factor(bad)
        assert e.value.status == glf.ERR_INVALID
    with pytest.raises(ValueError):
        glf.fit_factor(np.zeros((m, m + 1)))
    with pytest.raises(ValueError):
        glf.fit_factor(G, np.zeros(m + 1))
