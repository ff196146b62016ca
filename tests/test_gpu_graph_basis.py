"""Change of basis on a graph handle: glf_graph_transform (k_graph_transform: Phi <- Phi T in place, v_mfma_f32_32x32x2_f32 with the
pixels as the M index, one wave per tile of 32 pixels, LD / 32 accumulator tiles per wave) and glf_graph_orthonormalize on top of
it (normal equations, the host solve glf_basis_orthonormal, the transform).

Shapes: those of tests/test_gpu_graph.py, epsilon = 0.1. 61 x 47 = 2867 = 89 * 32 + 19 pixels, so the last tile is partial, at
ld 32 / 64 / 128 / 256 (the whole of T in LDS up to ld 128; at ld 256 the workgroup stages 64 rows of T per chunk between barriers,
and 90 tiles are 22 groups of four and one of two: two waves of the last group have no tile and still reach the barriers); `tiny`
is 160 pixels, 5 tiles; 509 x 515 has 8192 tiles, more than the grid has waves at every ld, so every wave runs its tile loop more
than once: the prefetch of the next tile under the last chunk, fresh accumulators, the reuse of the wave's LDS image.

Bounds. The transform against fp64: |Phi' - Phi fl32(T)| <= (ld + 4) 2^-24 (|Phi| |fl32 T|) per element, the f32 bound of an
ld-term fma chain (the form of test_gpu_graph._synth_want); the operands are exact, so an identity, a permutation and powers of
two are reproduced exactly. After a transform: project, synthesize and gram against fp64 on the read-back Phi' under the bounds
of tests/test_gpu_graph.py and tests/test_gpu_graph_fit.py. The driver's orthonormality: with P = Phi fl32(T) in f64 and B the
bound above, max |Phi'^T Phi' - I| <= max |P^T P - I| + max_ij sum_px (|P_i| B_j + B_i |P_j| + B_i B_j).
The operator (test 8): |apply - z0| <= the apply test's bounds on Phi' + 4 times max |z1 - z0|, z1 the f64 pipeline on P.
Measured on an MI355X: max |z1 - z0| = 2.1e-8 .. 4.9e-8 of max |z0|, the whole error 1.3e-7 .. 6.9e-7 of it and at most 0.089 of the
bound (test_the_operator_is_unchanged's docstring has every shape); orthonormality after one Ritz pass 1.4e-7 .. 9.8e-7 from a
defect of 0.05 .. 0.41 before it, against a reference term of 1.1e-7 .. 1.6e-7 and a rounding term of 4.6e-6 .. 7.5e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _assert_synth, _bits, _dev, _grey_graph, _synth_want, shape_param  # noqa: E402
from test_gpu_graph_fit import EPS_G, EPS_GRAM  # noqa: E402

C = glf.C
EPS32 = 2.0 ** -24


def _fl32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _phi(g):
    """All ld columns of Phi as the float32 array [N, ld] it is."""
    return g.phi.cpu().numpy().copy()


def _want(phi, T, ld):
    """(Phi fl32(T), the elementwise bound) in fp64 from the float32 read-back phi [N, ld] and T [m, m_new]."""
    p64 = phi[:, :T.shape[0]].astype(np.float64)
    t32 = _fl32(T)
    return p64 @ t32, (ld + 4) * EPS32 * (np.abs(p64) @ np.abs(t32))


def _assert_transform(got, phi, T, ld, what):
    """got: the read-back Phi' [N, ld]."""
    m_new = T.shape[1]
    want, bound = _want(phi, T, ld)
    err = np.abs(got[:, :m_new].astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: max |Phi' - Phi fl32(T)| / bound %.3f (max err %.3e)" % (what, worst, float(err.max())))
    assert np.isfinite(got).all() and np.all(err <= bound), (what, worst)
    assert not got[:, m_new:].any(), what                                         # columns m_new .. ld: exact zeros
    return want, bound


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------

@shape_param
def test_identity_leaves_phi_unchanged(shape):
    m, ld = SHAPES[shape][4:]
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, shape)
        before, lam = _phi(g), g.eigenvalues.copy()
        assert before.shape[1] == ld and not before[:, m:].any() and before[:, :m].any()
        g.transform(np.eye(m), lam)
        after = _phi(g)
        assert g.info["m"] == m and g.info["ld"] == ld
        np.testing.assert_array_equal(g.eigenvalues, lam)
        g.close()
    np.testing.assert_array_equal(after, before)                                  # as float values, pad columns included


# ---- 2. permutation times powers of two ---------------------------------------------------------------------------------------------

@shape_param
def test_permutation_times_powers_of_two_is_exact(shape):
    m, ld = SHAPES[shape][4:]
    rng = np.random.default_rng(ld + m)
    perm = rng.permutation(m)
    scale = 2.0 ** rng.integers(-3, 4, m) * rng.choice([-1.0, 1.0], m)
    T = np.zeros((m, m))
    T[perm, np.arange(m)] = scale                                                  # column j = scale_j times the old column perm_j
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, shape)
        before, lam = _phi(g), g.eigenvalues.copy()
        g.transform(T, lam[perm])
        after = _phi(g)
        np.testing.assert_array_equal(g.eigenvalues, lam[perm])
        g.close()
    np.testing.assert_array_equal(after[:, :m], before[:, perm] * scale.astype(np.float32))
    assert not after[:, m:].any()


# ---- 3. dense random T against fp64 -------------------------------------------------------------------------------------------------

@shape_param
@pytest.mark.parametrize("cut", ["full", "truncated"])
def test_dense_transform_against_fp64(shape, cut):
    m, ld = SHAPES[shape][4:]
    m_new = m if cut == "full" else max(1, (2 * m) // 5 + 1)                       # 4, 17, 41, 81 and 2: inside a 32-column block
    rng = np.random.default_rng(7 * ld + m_new)
    T = rng.uniform(-1.0, 1.0, (m, m_new))
    lam_new = rng.uniform(0.5, 1.0, m_new)
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, shape)
        before = _phi(g)
        g.transform(T, lam_new)
        after = _phi(g)
        assert (g.info["m"], g.info["ld"], g.info["phi_bytes"]) == (m_new, ld, 4 * before.size)
        np.testing.assert_array_equal(g.eigenvalues, lam_new)
        g.close()
    _assert_transform(after, before, T, ld, "%s m_new %d" % (shape, m_new))


@pytest.mark.parametrize("m,ld", [(8, 32), (40, 64), (100, 128), (200, 256)])
def test_transform_many_tiles_per_wave(m, ld):
    """509 x 515 = 8191 tiles of 32 pixels and one of 23: more tiles than the grid has waves (at most 7 workgroups of 4 waves per
    CU), so every wave runs its tile loop more than once. Every element against fp64 (torch, on the device) at test 3's bound."""
    w, h = 509, 515
    n = w * h
    rng = np.random.default_rng(ld)
    m_new = m - 3
    T = rng.uniform(-1.0, 1.0, (m, m_new))
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["p"], g.info["m"], g.info["ld"]) == (324, m, ld)
        before = g.phi[:, :m].double()                                            # (a copy: the transform rewrites g.phi)
        t32 = torch.from_numpy(_fl32(T)).to(ctx.device)
        want, bound = before @ t32, (ld + 4) * EPS32 * (before.abs() @ t32.abs())
        g.transform(T, np.linspace(0.5, 1.0, m_new))
        torch.cuda.synchronize()
        err = (g.phi[:, :m_new].double() - want).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        ok = bool(torch.all(err <= bound)) and bool(torch.isfinite(g.phi).all()) and not bool(g.phi[:, m_new:].any())
        g.close()
    print("ld %d, %d tiles: max |Phi' - Phi fl32(T)| / bound %.3f" % (ld, (n + 31) // 32, worst))
    assert ok, (ld, worst)


# ---- 4. a column's bits do not depend on its neighbours -----------------------------------------------------------------------------

@shape_param
def test_a_column_does_not_depend_on_its_neighbours(shape):
    m, ld = SHAPES[shape][4:]
    rng = np.random.default_rng(31 + ld)
    T = rng.uniform(-1.0, 1.0, (m, m))
    cols = sorted({0, m // 2, m - 1})
    got = {}
    with glf.Context(0) as ctx:
        def run(TT):
            g, _, _ = _grey_graph(ctx, shape)
            g.transform(TT, np.linspace(0.5, 1.0, TT.shape[1]))
            out = _phi(g)
            g.close()
            return out
        full = run(T)
        for j in cols:
            other = rng.uniform(-2.0, 2.0, (m, m))                                # every other column differs
            other[:, j] = T[:, j]
            got[j] = (run(other), run(T[:, :j + 1]))
    for j in cols:
        np.testing.assert_array_equal(_bits(got[j][0][:, j]), _bits(full[:, j]), err_msg="column %d under another T" % j)
        np.testing.assert_array_equal(_bits(got[j][1][:, j]), _bits(full[:, j]), err_msg="column %d under m_new = %d" % (j, j + 1))
        assert not got[j][1][:, j + 1:].any()


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------

@shape_param
def test_two_handles_the_same_transform_the_same_bits(shape):
    m, ld = SHAPES[shape][4:]
    T = np.random.default_rng(ld).normal(size=(m, m))
    out = []
    with glf.Context(0) as ctx:
        for _ in range(2):
            g, _, _ = _grey_graph(ctx, shape)
            g.transform(T, g.eigenvalues)
            out.append(_phi(g))
            g.close()
    np.testing.assert_array_equal(_bits(out[0]), _bits(out[1]))


# ---- 6. the handle's state after a transform -----------------------------------------------------------------------------------------

@shape_param
def test_handle_state_after_a_transform(shape):
    width, h, _, p, m, ld = SHAPES[shape]
    m_new = max(2, (3 * m) // 4)
    rng = np.random.default_rng(3 * ld + 1)
    T = rng.uniform(-1.0, 1.0, (m, m_new)) / np.sqrt(m)
    lam_new = np.sort(rng.uniform(0.5, 1.1, m_new))
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        stale = g.gram()                                                          # cached by the handle now
        g.transform(T, lam_new)
        assert g.info == dict(pix=0, width=width, height=h, p=p, m=m_new, ld=ld, phi_bytes=4 * width * h * ld)
        np.testing.assert_array_equal(g.eigenvalues, lam_new)
        lam_raw = np.zeros(m_new)
        assert glf._lib.glf_graph_eigenvalues(g._g, glf._ptr(lam_raw)) == glf.OK
        np.testing.assert_array_equal(lam_raw, lam_new)
        phi = _phi(g)[:, :m_new].astype(np.float64)
        gram = g.gram()
        G, _ = g.normal_equations(None)
        c = g.project(d_sig)
        a = rng.normal(size=(5, m_new)) * np.abs(c).max(axis=0)
        ident, plane = np.array([0.0, 1.0, -0.5, 1.0, 0.0], dtype=np.float32), np.array([-1, 0, 1, 2, 2], dtype=np.int32)
        z = g.synthesize(a, ident, plane, d_sig).cpu().numpy()
        labels, sums, counts, _ = g.cluster_step(phi[:2, :min(m_new, 64)])          # dim = min(m_new, 64): accepted
        assert int(counts.sum()) == width * h
        if m_new < 64:
            with pytest.raises(glf.GlfError) as e:                                # dim > m_new: refused, whatever m was
                g.cluster_step(np.zeros((2, m_new + 1)))
            assert e.value.status == glf.ERR_INVALID
        with pytest.raises(ValueError):
            g.synthesize(np.zeros((1, m)))                                        # the Python object sees m_new too
        g.close()
    assert gram.shape == (m_new, m_new) and G.shape == (m_new, m_new) and c.shape == (3, m_new)
    G64, S = phi.T @ phi, np.abs(phi).T @ np.abs(phi)
    assert np.all(np.abs(gram - G64) <= (EPS_G + EPS_GRAM) * S)                   # recomputed,
    assert not np.all(np.abs(stale[:m_new, :m_new] - G64) <= (EPS_G + EPS_GRAM) * S)   # not the stale one
    assert np.all(np.abs(G - G64) <= EPS_G * S)
    n = phi.shape[0]
    for q in range(3):
        assert np.all(np.abs(c[q] - phi.T @ s[q]) <= n * 2.0 ** -51 * (np.abs(phi).T @ np.abs(s[q]))), (shape, q)
    for j in range(5):
        want, bound = _synth_want(phi, ld, a[j], ident[j], int(plane[j]), s)
        _assert_synth(z[j], want, bound, "%s after the transform, output %d" % (shape, j))


# ---- 7. the driver --------------------------------------------------------------------------------------------------------------------

@shape_param
@pytest.mark.parametrize("mode", ["ritz", "cholesky"])
def test_orthonormalize_is_its_three_steps(shape, mode):
    m, ld = SHAPES[shape][4:]
    with glf.Context(0) as ctx:
        ref, _, _ = _grey_graph(ctx, shape)
        g, _, _ = _grey_graph(ctx, shape)
        before = _phi(ref)
        np.testing.assert_array_equal(_bits(_phi(g)), _bits(before))              # identically built
        lam = ref.eigenvalues.copy()
        G, _ = ref.normal_equations(None)
        if mode == "ritz":
            T, lam_new = glf.basis_orthonormal(G, lam)
        else:
            T, lam_new = glf.basis_orthonormal(G), lam
        ref.transform(T, lam_new)
        st = g.orthonormalize(mode, passes=1, verify=True)
        after = _phi(g)
        np.testing.assert_array_equal(_bits(after), _bits(_phi(ref)))
        np.testing.assert_array_equal(g.eigenvalues, ref.eigenvalues)
        np.testing.assert_array_equal(g.eigenvalues, lam_new)
        G1, _ = g.normal_equations(None)
        assert st["passes"] == 1
        assert st["defect_in"] == float(np.abs(G - np.eye(m)).max())
        assert st["defect_out"] == float(np.abs(G1 - np.eye(m)).max())
        ref.close()
        # without verify: no defect_out; a second pass keeps the eigenvalues and their order
        g2, _, _ = _grey_graph(ctx, shape)
        st2 = g2.orthonormalize(mode, passes=2)
        assert st2["passes"] == 2 and st2["defect_in"] == st["defect_in"] and np.isnan(st2["defect_out"])
        np.testing.assert_array_equal(g2.eigenvalues, lam_new)
        G2, _ = g2.normal_equations(None)
        g2.close()
        g.close()
    if mode == "ritz":
        assert np.all(np.diff(lam_new) >= 0.0)
    # orthonormality of the read-back Phi' in f64 against what fl32(T) and the kernel's rounding allow
    P, B = _want(before, T, ld)
    phi1 = after[:, :m].astype(np.float64)
    got = float(np.abs(phi1.T @ phi1 - np.eye(m)).max())
    ref_term = float(np.abs(P.T @ P - np.eye(m)).max())
    aP = np.abs(P)
    round_term = float((aP.T @ B + B.T @ aP + B.T @ B).max())
    print("%s %s: defect_in %.3e, cond(G) %.3f, max |T| %.3f, max |Phi'^T Phi' - I| %.3e <= %.3e + %.3e; defect_out %.3e, after two passes %.3e"
          % (shape, mode, st["defect_in"], float(np.linalg.cond(G)), float(np.abs(T).max()), got, ref_term, round_term, st["defect_out"],
             float(np.abs(G2 - np.eye(m)).max())))
    assert got <= ref_term + round_term


# ---- 8. the operator is unchanged -----------------------------------------------------------------------------------------------------

@shape_param
def test_the_operator_is_unchanged(shape):
    """W = Phi diag(1 - lam) Phi^T before, and Graph.apply with the response 1 - lam' on the Ritz basis after.
    |apply - z0| <= (ld + 4) 2^-24 |Phi'| |a| (the apply test's bound on Phi', a = (1 - lam') Phi'^T s in f64)
                  + |Phi'| (|1 - lam'| o the projection bound N 2^-51 |Phi'|^T |s|)
                  + 4 max |z1 - z0|, z1 the f64 pipeline on P = Phi fl32(T): the basis term.
    Measured on an MI355X, random-normal plane of seed 5, as fractions of max |z0|, ld32 / ld64 / ld128 / ld256 / tiny:
      max |z1 - z0| (a quarter of the basis term)   2.1e-8 / 4.9e-8 / 4.8e-8 / 3.8e-8 / 3.3e-8
      max |Phi' a - z0| (f64 on the read-back Phi')  7.4e-8 / 1.5e-7 / 4.6e-7 / 6.2e-7 / 1.1e-7
      max |apply - z0|                               1.3e-7 / 2.1e-7 / 5.0e-7 / 6.9e-7 / 1.7e-7
    and max |apply - z0| / bound 0.059 / 0.089 / 0.070 / 0.052 / 0.083: the factor four was not needed at any shape (the apply
    test's own term, which grows with ld, carries the bound)."""
    width, h, _, _, m, ld = SHAPES[shape]
    rng = np.random.default_rng(5)
    s32 = rng.normal(size=(1, h, width)).astype(np.float32)
    s = s32.reshape(-1).astype(np.float64)
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, shape)
        phi0, lam = _phi(g)[:, :m].astype(np.float64), g.eigenvalues.copy()
        G, _ = g.normal_equations(None)
        T, lam_new = glf.basis_orthonormal(G, lam)
        g.orthonormalize("ritz")
        np.testing.assert_array_equal(g.eigenvalues, lam_new)
        out = g.apply(_dev(ctx, s32), (1.0 - g.eigenvalues)[None, :], ident=0.0).cpu().numpy().reshape(-1).astype(np.float64)
        phi1 = _phi(g)[:, :m].astype(np.float64)
        g.close()
    z0 = phi0 @ ((1.0 - lam) * (phi0.T @ s))
    P = phi0 @ _fl32(T)
    z1 = P @ ((1.0 - lam_new) * (P.T @ s))
    basis = 4.0 * float(np.abs(z1 - z0).max())
    a = (1.0 - lam_new) * (phi1.T @ s)
    cb = phi1.shape[0] * 2.0 ** -51 * (np.abs(phi1).T @ np.abs(s))
    bound = (ld + 4) * EPS32 * (np.abs(phi1) @ np.abs(a)) + np.abs(phi1) @ (np.abs(1.0 - lam_new) * cb) + basis
    err = np.abs(out - z0)
    zmax = float(np.abs(z0).max())
    print("%s: max |z1 - z0| / max |z0| %.3e (basis term 4x), max |Phi' a - z0| / max |z0| %.3e, max |apply - z0| / max |z0| %.3e, "
          "max |apply - z0| / bound %.3f" % (shape, basis / 4.0 / zmax, float(np.abs(phi1 @ a - z0).max()) / zmax, float(err.max()) / zmax,
                                             float((err / bound).max())))
    assert np.all(err <= bound), shape


# ---- 9. refusals on a live handle -----------------------------------------------------------------------------------------------------

def test_refusals_leave_phi_bit_identical():
    lib = glf._lib
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, "ld64")
        m = g.info["m"]
        before, info, lam = _phi(g), dict(g.info), g.eigenvalues.copy()
        T = np.random.default_rng(1).normal(size=(m + 1, m + 1))
        ok_lam = np.linspace(0.5, 1.0, m + 1)
        nan_T, inf_T, big_T = T[:m, :m].copy(), T[:m, :m].copy(), T[:m, :m].copy()
        nan_T[3, 5], inf_T[m - 1, m - 1], big_T[0, 1] = np.nan, -np.inf, 1e300     # (1e300 is finite, and no float)
        nan_lam, inf_lam = ok_lam[:m].copy(), ok_lam[:m].copy()
        nan_lam[2], inf_lam[m - 1] = np.nan, np.inf
        sq = np.ascontiguousarray(T[:m, :m])
        cases = {"T NULL": (m, None, ok_lam), "lam NULL": (m, sq, None), "m_new = 0": (0, sq, ok_lam), "m_new > m": (m + 1, T, ok_lam),
                 "NaN in T": (m, nan_T, ok_lam), "Inf in T": (m, inf_T, ok_lam), "T beyond float": (m, big_T, ok_lam),
                 "NaN in lam": (m, sq, nan_lam), "Inf in lam": (m, sq, inf_lam)}
        for what, (m_new, TT, ll) in cases.items():
            assert lib.glf_graph_transform(g._g, C.c_uint(m_new), glf._ptr(TT), glf._ptr(ll)) == glf.ERR_INVALID, what
        good = glf.BasisStats(struct_size=C.sizeof(glf.BasisStats))
        bad = glf.BasisStats(struct_size=C.sizeof(glf.BasisStats) + 8)
        for mode, passes, st in ((2, 1, good), (-1, 1, good), (1, 0, good), (1, 3, good), (0, -1, good), (1, 1, bad), (0, 2, bad)):
            assert lib.glf_graph_orthonormalize(g._g, mode, passes, 1, C.byref(st)) == glf.ERR_INVALID, (mode, passes)
        for kw in (dict(mode="qr"), dict(passes=0), dict(passes=3)):
            with pytest.raises(glf.GlfError) as e:
                g.orthonormalize(**kw)
            assert e.value.status == glf.ERR_INVALID
        with pytest.raises(glf.GlfError):
            g.transform(nan_T, ok_lam[:m])
        with pytest.raises(ValueError):
            g.transform(T, ok_lam)                                                # [m + 1, m + 1]
        np.testing.assert_array_equal(_bits(_phi(g)), _bits(before))
        assert g.info == info
        np.testing.assert_array_equal(g.eigenvalues, lam)
        gi = glf.GraphInfo(struct_size=C.sizeof(glf.GraphInfo))
        assert lib.glf_graph_get_info(g._g, C.byref(gi)) == glf.OK and gi.m == m
        # the next valid calls succeed
        st = g.orthonormalize("ritz", verify=True)
        assert st["defect_out"] < st["defect_in"]
        g.close()
