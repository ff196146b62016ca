"""The change of basis' C-ABI (glf_graph_transform, glf_basis_orthonormal, glf_graph_orthonormalize): exported by libglf.so, declared
in include/glf.h, listed in glf.EXPORTS; without a handle the two handle calls answer GLF_ERR_INVALID before any device work; and
glf_basis_orthonormal, which is host only, against its defining identities and numpy. CPU only.

Matrices: G = Q diag(d) Q^T with a random orthogonal Q (QR of a normal matrix) and d spread geometrically over [cond^-1/2, cond^1/2],
cond = 1.3, 1e2, 1e4, at m = 4, 8, 40, 200; lam uniform in (0.6, 1.1), unsorted.
Bound of every identity and comparison: 64 m 2^-52 cond(G) times the largest entry involved (of T, G and the right-hand side). A
backward-stable Cholesky factorisation and triangular inverse err by about m 2^-53 cond(G) relative to those entries, and the Jacobi
rotations add m 2^-53 per sweep; the factor 64 leaves a decade and a half over that. numpy's own cholesky + eigh left 1.1e-15 at
m = 200, cond 1.3, against the 3.7e-12 this bound gives there. The products of the checks are formed in extended precision, so the
check's own rounding stays below the bound's last digit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glf_graph_transform", "glf_basis_orthonormal", "glf_graph_orthonormalize")
CONDS = (1.3, 1e2, 1e4)
SIZES = (4, 8, 40, 200)
LD = np.longdouble


def test_basis_entry_points_are_exported_and_declared():
    lib = C.CDLL(glf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "glf.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in glf.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"GLF_BASIS_CHOLESKY\s*=\s*0\b", header) and re.search(r"GLF_BASIS_RITZ\s*=\s*1\b", header)
    assert (glf.BASIS_CHOLESKY, glf.BASIS_RITZ) == (0, 1)
    assert C.sizeof(glf.BasisStats) == 24
    assert callable(glf.basis_orthonormal)
    for method in ("transform", "orthonormalize"):
        assert hasattr(glf.Graph, method), method


def test_handle_calls_without_a_handle_are_invalid():
    lib = C.CDLL(glf.LIB_PATH)
    lib.glf_graph_transform.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
    lib.glf_graph_orthonormalize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    buf = (C.c_double * 64)()
    st = glf.BasisStats(struct_size=C.sizeof(glf.BasisStats))
    for m_new in (0, 1, 8):
        assert lib.glf_graph_transform(None, m_new, buf, buf) == glf.ERR_INVALID, m_new
        assert lib.glf_graph_transform(None, m_new, None, None) == glf.ERR_INVALID, m_new
    for mode in (-1, 0, 1, 2):
        for passes in (0, 1, 2, 3):
            assert lib.glf_graph_orthonormalize(None, mode, passes, 1, C.byref(st)) == glf.ERR_INVALID, (mode, passes)
            assert lib.glf_graph_orthonormalize(None, mode, passes, 0, None) == glf.ERR_INVALID, (mode, passes)


def _case(m, cond, seed):
    """(G, lam): G = Q diag(d) Q^T, exactly symmetric, cond(G) = cond."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
    d = np.geomspace(cond ** -0.5, cond ** 0.5, m)
    rng.shuffle(d)
    G = (Q * d) @ Q.T
    return 0.5 * (G + G.T), rng.uniform(0.6, 1.1, m)


def _bound(m, cond, *mats):
    return 64.0 * m * 2.0 ** -52 * cond * max(float(np.abs(a).max()) for a in mats)


def _defect(T, A, want):
    """max |T^T A T - want| in extended precision."""
    Tl = T.astype(LD)
    return float(np.abs(Tl.T @ A.astype(LD) @ Tl - want.astype(LD)).max())


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("cond", CONDS)
def test_ritz_basis_identities_order_sign_and_determinism(m, cond):
    G, lam = _case(m, cond, 1000 * m + int(cond))
    T, lam_new = glf.basis_orthonormal(G, lam)
    assert T.shape == (m, m) and lam_new.shape == (m,) and np.isfinite(T).all()
    eye = np.eye(m)
    d1, b1 = _defect(T, G, eye), _bound(m, cond, T, G, eye)
    # T diag(1 - lam_new) T^T = diag(1 - lam): the congruence of T^T
    d2, b2 = _defect(T.T.copy(), np.diag(1.0 - lam_new), np.diag(1.0 - lam)), _bound(m, cond, T, 1.0 - lam_new, 1.0 - lam)
    print("m %d cond %g: |T^T G T - I| %.2e <= %.2e, |T diag(1 - lam') T^T - diag(1 - lam)| %.2e <= %.2e, max |T| %.2f"
          % (m, cond, d1, b1, d2, b2, float(np.abs(T).max())))
    assert d1 <= b1 and d2 <= b2
    assert np.all(np.diff(lam_new) >= 0.0)                                        # ascending
    # the eigenvalues of the operator: those of S = L^T diag(1 - lam) L, by numpy
    L = np.linalg.cholesky(G)
    theta = np.linalg.eigvalsh(L.T @ np.diag(1.0 - lam) @ L)[::-1]
    assert float(np.abs((1.0 - theta) - lam_new).max()) <= _bound(m, cond, L, 1.0 - lam)
    # the sign rule on U = L^T T: the entry of largest magnitude of every column is positive
    U = L.T @ T
    big = U[np.abs(U).argmax(axis=0), np.arange(m)]
    assert np.all(big > 0.0)
    T2, lam2 = glf.basis_orthonormal(G.copy(), lam.copy())                       # two calls, the same bits
    np.testing.assert_array_equal(T2.view(np.uint64), T.view(np.uint64))
    np.testing.assert_array_equal(lam2.view(np.uint64), lam_new.view(np.uint64))


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("cond", CONDS)
def test_cholesky_mode_against_numpy(m, cond):
    G, _ = _case(m, cond, 2000 * m + int(cond))
    T = glf.basis_orthonormal(G)
    assert T.shape == (m, m)
    np.testing.assert_array_equal(np.tril(T, -1), 0.0)                            # upper triangular,
    assert np.all(np.diag(T) > 0.0)                                               # positive diagonal
    eye = np.eye(m)
    d1, b1 = _defect(T, G, eye), _bound(m, cond, T, G, eye)
    want = np.linalg.inv(np.linalg.cholesky(G)).T
    d2, b2 = float(np.abs(T - want).max()), _bound(m, cond, T, want)
    print("m %d cond %g: |T^T G T - I| %.2e <= %.2e, |T - inv(cholesky(G))^T| %.2e <= %.2e" % (m, cond, d1, b1, d2, b2))
    assert d1 <= b1 and d2 <= b2
    # numpy's own factor stays inside the bound too
    assert _defect(want, G, eye) <= _bound(m, cond, want, G, eye)
    np.testing.assert_array_equal(glf.basis_orthonormal(G).view(np.uint64), T.view(np.uint64))
    # the lower triangle alone is read
    half = np.tril(G) + np.triu(np.full((m, m), 1e300), 1)
    np.testing.assert_array_equal(glf.basis_orthonormal(half).view(np.uint64), T.view(np.uint64))


def test_ties_keep_the_original_order():
    m = 5
    T, lam_new = glf.basis_orthonormal(np.eye(m), np.full(m, 0.75))
    np.testing.assert_array_equal(T, np.eye(m))
    np.testing.assert_array_equal(lam_new, np.full(m, 0.75))
    lam = np.array([0.9, 0.7, 1.05, 0.8, 0.7])                                   # orthonormal already: a stable sort
    T, lam_new = glf.basis_orthonormal(np.eye(m), lam)
    order = np.argsort(lam, kind="stable")
    np.testing.assert_array_equal(lam_new, 1.0 - (1.0 - lam[order]))
    np.testing.assert_array_equal(T, np.eye(m)[:, order])


def _raw(m, G, lam, T, lam_new):
    return glf._lib.glf_basis_orthonormal(C.c_uint(m), glf._ptr(G), glf._ptr(lam), glf._ptr(T), glf._ptr(lam_new))


def test_refusals_leave_the_outputs_untouched():
    m = 8
    G, lam = _case(m, 1.3, 5)
    fillT, filll = np.full((m, m), 12345.0), np.full(m, 54321.0)
    T, ln = fillT.copy(), filll.copy()
    assert _raw(m, G, lam, T, ln) == glf.OK and not np.array_equal(T, fillT) and not np.array_equal(ln, filll)
    indefinite = np.eye(m)
    indefinite[5, 5] = -1.0
    with_nan = G.copy()
    with_nan[2, 5] = np.nan
    with_inf = G.copy()
    with_inf[m - 1, m - 1] = np.inf
    nan_lam = lam.copy()
    nan_lam[3] = np.nan
    inf_lam = lam.copy()
    inf_lam[0] = -np.inf
    cases = {"G NULL": (m, None, lam, True, True), "T NULL": (m, G, lam, False, True), "lam without lam_new": (m, G, lam, True, False),
             "m = 0": (0, G, lam, True, True), "indefinite": (m, indefinite, lam, True, True), "singular": (m, np.zeros((m, m)), lam, True, True),
             "NaN in G": (m, with_nan, lam, True, True), "Inf on the diagonal": (m, with_inf, lam, True, True),
             "NaN in lam": (m, G, nan_lam, True, True), "Inf in lam": (m, G, inf_lam, True, True),
             "indefinite, Cholesky mode": (m, indefinite, None, True, True), "NaN in G, Cholesky mode": (m, with_nan, None, True, True),
             "singular, Cholesky mode": (m, np.zeros((m, m)), None, True, False)}
    for what, (mm, GG, ll, haveT, havel) in cases.items():
        T, ln = fillT.copy(), filll.copy()
        assert _raw(mm, GG, ll, T if haveT else None, ln if havel else None) == glf.ERR_INVALID, what
        np.testing.assert_array_equal(T, fillT, err_msg=what)
        np.testing.assert_array_equal(ln, filll, err_msg=what)
    T, ln = fillT.copy(), filll.copy()
    assert _raw(m, G, None, T, ln) == glf.OK                                      # Cholesky mode does not write lam_new
    np.testing.assert_array_equal(ln, filll)
    assert _raw(m, G, None, T, None) == glf.OK
    for bad in (indefinite, np.zeros((m, m)), with_nan):
        with pytest.raises(glf.GlfError) as e:
            glf.basis_orthonormal(bad, lam)
        assert e.value.status == glf.ERR_INVALID
    with pytest.raises(ValueError):
        glf.basis_orthonormal(np.zeros((m, m + 1)))
    with pytest.raises(ValueError):
        glf.basis_orthonormal(G, np.zeros(m + 1))


def test_make_basis_check_runs_clean(tmp_path):
    """The stand-alone driver of glf_basis_orthonormal under the address and undefined-behaviour sanitizers (CPU only)."""
    out = subprocess.run(["make", "-C", ROOT, "basis_check", "BASIS_CHECK_BIN=%s" % (tmp_path / "basis_host_check")], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "basis_host_check: ok" in out.stdout
