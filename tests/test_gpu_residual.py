"""The residual || A X - X (X^T A X) ||_F that stops the eigen-solve, in both forms -- the explicit sweep over L_A (RESIDUAL=sweep) and
the default derived from the PCG state, A X_new = (B - R_pcg) Tn -- against a float64 evaluation, at the first three states of a solve,
where the residual is 0.2 to 3.5 and a defect shows (at convergence everything is small). Needs an MI355X: -m gpu.

Through InversePowerIteration, which runs exactly K outer iterations and returns the vectors and st["residual"]: K >= 1 with
epsilon = 1e-30, max_outer = K and allow_noconv; K = 0 with epsilon = 1e30, because the entry point reads max_outer = 0 as "no cap"
(pipeline.hip: max_outer > 0 ? max_outer : 100000) -- the loop then never starts, which is the state asked for. The inner solves run
to the solver's 1e-5 and, a second time, to 0.3, where the PCG residual the derived form relies on is large (see the test).

A: L_A of the float64 oracle on a sorted random sample set of exactly p pixels of a glf.synth_image, rounded to f32 (what the device
stores), ld = round_up(p, 64). Reference: K = 0, the returned vectors V are the orthonormalised start block, renormalised: r_ref =
residual(A, V). K >= 1, they are the normalised pre-orthonormalisation block Y: r_ref = residual(A, cgs(Y).Q).
Bounds (tests/eigen_ref.py, residual_bound and derived_bound; models, as the operator's bound is):
  |r_sweep - r_ref| <= ||B||_F
  |r_derived - r_sweep| <= 2 its (gamma_op + 4 u) || |A| |Y| |T| ||_F for K >= 1, its = the inner iterations of the last outer step
The two modes are the same iterates: vectors and eigenvalues bit-identical, and at K = 0 the residual too (both take the sweep). Under
GS=seq the solver has no triangular map, so both modes are the sweep: everything bit-identical at every K."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import eigen_ref as er  # noqa: E402
import operator_ref as oref  # noqa: E402

KS = (0, 1, 2)


@pytest.fixture(scope="module", params=["f16s", "f32"])
def ctx(request):
    """Both contraction modes: the stored L_A is swept by k_block_matvec_f16s or k_block_matvec."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    c.set_contraction(glf.CONTRACT_F16_SPLIT if request.param == "f16s" else glf.CONTRACT_F32_MFMA)
    c.mode = request.param
    c.mats, c.runs = {}, {}
    yield c
    c.destroy(*c.mats.values())
    c.close()


@pytest.fixture(autouse=True)
def _default_kernel_selection(request):
    yield
    if "ctx" in request.fixturenames:
        request.getfixturevalue("ctx").reset_tuning()


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("GLF_EIGEN_ERROR_JSON")
    if path and er.RECORD:
        er.dump(path)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _solve(ctx, p, m, K, residual=None, gs=None, rtol=1e-5):
    """(V float32 [p, m], eigenvalues float32 [m], residual, inner iterations in all) after exactly K outer iterations."""
    key = (p, m, K, residual, gs, rtol)
    if key not in ctx.runs:
        if p not in ctx.mats:
            ctx.mats[p] = ctx.dense_from_numpy(er.laplacian_case(p), ld=oref.round_up(p, 64))
        ctx.set_tuning(RESIDUAL=residual, GS=gs)
        kw = dict(epsilon=1e30, max_outer=1) if K == 0 else dict(epsilon=1e-30, max_outer=K, allow_noconv=True)
        vecs, vals, st = ctx.InversePowerIteration(ctx.mats[p], m, inner_rtol=rtol, X0=glf.random_vectors(p, m, 1), **kw)
        ctx.set_tuning(RESIDUAL=None, GS=None)
        assert st["outer_its"] == K
        ctx.runs[key] = (ctx.mat_to_numpy(vecs), ctx.mat_to_numpy(vals), st["residual"], st["inner_its_total"])
        ctx.destroy(vecs, vals)
    return ctx.runs[key]


_REFS = {}


def _reference(p, m, K, V, wide=False):
    """(X_ref float64, cgs(V) or None, d) of a returned block, computed once per block (both contraction modes return their own)."""
    key = (p, m, K, V.tobytes())
    if key not in _REFS:
        if K == 0:
            _REFS[key] = (V.astype(np.float64), None, 0.0)
        else:
            ref = er.cgs(V)
            form = er.cgs_panels(V) if wide else er.cgs_gram_f32(V)
            d = max(er.deviation(form[0], form[1], ref)[0], er.renorm_deviation(V, ref))     # RENORMALISED_INPUT
            _REFS[key] = (ref.Q, ref, d)
    return _REFS[key]


def _assert_sweep(ctx, p, m, K, V, r, family, wide=False):
    A = er.laplacian_case(p).astype(np.float64)
    X, ref, d = _reference(p, m, K, V, wide)
    r_ref = er.residual(A, X)
    E = er.start_block_E(V) if K == 0 else er.orthonormalised_E(ref, d)
    B = float(np.linalg.norm(er.residual_bound(A, X, er.ld_for(m), ctx.mode, E)))
    ratio = er.record(family, ctx.mode, "p %d m %d K %d" % (p, m, K), abs(r - r_ref), B, d)
    print("%s p %d m %d K %d: r %.9g, fp64 %.9g, |r - r_ref| %.3g = %.3g of the bound %.3g (d %.3g)" % (ctx.mode, p, m, K, r, r_ref,
                                                                                                      abs(r - r_ref), ratio, B, d))
    assert np.isfinite(r) and abs(r - r_ref) <= B
    return A, ref


@pytest.mark.parametrize("rtol", [1e-5, 0.3], ids=["rtol1e-5", "rtol0.3"])
@pytest.mark.parametrize("p,m", er.RESID_SHAPES)
def test_both_forms_against_fp64(ctx, p, m, rtol):
    """rtol: the inner solves' tolerance. At the solver's 1e-5 (3 PCG steps) the PCG residual R the derived form subtracts is 1e-5
    of B, and leaving it out moves the residual by 1e-6, far inside the derived form's bound; at 0.3 (1 or 2 steps) R is a third
    of B and the derived form stands or falls with it."""
    its_before = 0
    for K in KS:
        Vd, ld_, rd, its_d = _solve(ctx, p, m, K, "derived", rtol=rtol)
        Vs, ls_, rs, its_s = _solve(ctx, p, m, K, "sweep", rtol=rtol)
        assert Vd.shape == (p, m) and np.isfinite(Vd).all()
        # the same run in both modes: the same iterates, only the evaluation differs
        np.testing.assert_array_equal(_bits(Vd), _bits(Vs))
        np.testing.assert_array_equal(_bits(ld_), _bits(ls_))
        assert its_d == its_s
        A, ref = _assert_sweep(ctx, p, m, K, Vs, rs, "sweep residual")
        if K == 0:
            assert rd == rs and its_s == 0          # both take the explicit sweep
        else:
            its = its_s - its_before
            assert its >= 1
            bd = er.derived_bound(A, Vs, ref.T, its, ctx.mode)
            ratio = er.record("derived residual", ctx.mode, "p %d m %d K %d rtol %g" % (p, m, K, rtol), abs(rd - rs), bd)
            print("%s p %d m %d K %d rtol %g: derived %.9g, sweep %.9g, %d inner iterations, difference %.3g = %.3g of the bound %.3g" % (
                ctx.mode, p, m, K, rtol, rd, rs, its, abs(rd - rs), ratio, bd))
            assert np.isfinite(rd) and abs(rd - rs) <= bd
        its_before = its_s
        # the column-by-column sweep leaves no triangular map: both modes are the explicit sweep
        Vqd, lqd, rqd, _ = _solve(ctx, p, m, K, "derived", "seq", rtol)
        Vqs, lqs, rqs, _ = _solve(ctx, p, m, K, "sweep", "seq", rtol)
        np.testing.assert_array_equal(_bits(Vqd), _bits(Vqs))
        np.testing.assert_array_equal(_bits(lqd), _bits(lqs))
        assert rqd == rqs and np.isfinite(rqd)


@pytest.mark.parametrize("K", [0, 1])
def test_more_than_256_vectors(ctx, K):
    """panels_residual (k_gsf_gram with a second operand, k_gsf_sub, k_col_sumsq) with the sweep's bound at ld 256; the difference in X
    from cgs_panels."""
    p, m = er.RESID_WIDE
    V, lam, r, its = _solve(ctx, p, m, K)
    assert V.shape == (p, m) and np.isfinite(V).all() and np.isfinite(lam).all()
    _assert_sweep(ctx, p, m, K, V, r, "panels residual", wide=True)
