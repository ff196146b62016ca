"""The references of tests/eigen_ref.py and the conditions its test blocks must meet. CPU only.

Blocks (eigen_ref.make_case, each seeded), float32 [n, m]:
  white     normal entries
  graded    U diag(s) V^T with singular values log-spaced over [1, 1e-3]; then column k scaled by 2^e_k, e_k spread evenly over
            [-20, 20] (powers of two leave Q unchanged and scale the norms exactly)
  zero      white with column m // 2 set to zero
  dup_last  white with the last column a bitwise copy of column 1
  sum_last  white with the last column f32(x_2 + x_7); needs m > 8
Conditions, asserted for every row of eigen_ref.cases() (G_kk = |v_k|^2, q_k = <u_k, u_k> of cgs()):
  white, graded        min_k q_k / G_kk >= 1e-8 (100 times above GSF_COND_FLOOR: the Gram-matrix form must not fall back) and
                       numpy.linalg.cond <= 1.1e3 with the column scaling undone
  dup_last, sum_last   q_(m-1) / G_(m-1, m-1) <= 1e-12 (100 times below the floor: the device must fall back)
  zero                 q == 0 in exactly one place

Departures from the residual bound as first written, named here and asserted below (eigen_ref's docstring has the code lines):
  RESID_VECTOR_CHAIN   k_resid (ld 128, 256) subtracts X G from Y in one chain of m fmaf, not ld / 2 links
  RENORMALISED_INPUT   for K >= 1 the block a solve returns is the solver's pre-orthonormalisation block after one more f32 rounding
                       per entry, so d also covers cgs()'s deviation under one such rounding (eigen_ref.renorm_deviation)
And one from the orthonormalisation's cases:
  PANEL_DUP_NO_FALLBACK  more than 256 vectors, the last column of the second panel a copy of column 1 of the first: the copy is
                       removed by the cross-panel subtraction (k_gsf_sub), what is left of it is rounding noise of length 1e-7 |v|
                       in no particular direction, and the panel's own Gram-matrix form -- which compares q_k with the G_kk of the
                       block it is given -- finds it well conditioned. So the panel does not fall back, and under GS=seq the FIRST
                       panel takes the sweep too: the default run cannot be bit-identical to the GS=seq run. Each run is compared
                       with cgs() under its own emulation's d instead, the last norm with 1e-5 |v| as everywhere."""
import numpy as np
import pytest

import glf
import oracle as orc
import eigen_ref as er

CASES = er.cases()
IDS = ["%s-%dx%d-ld%d" % c[:4] for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_block_meets_its_conditions(c):
    cls, n, m, ld, seed = c
    X, ref = er.case(*c)
    assert X.dtype == np.float32 and X.shape == (n, m) and np.isfinite(X).all()
    G = (X.astype(np.float64) ** 2).sum(axis=0)
    if cls in ("white", "graded"):
        ratio = (ref.q / G).min()
        V = np.ldexp(X.astype(np.float64), -er.graded_exponents(m)[None, :]) if cls == "graded" else X.astype(np.float64)
        cond = np.linalg.cond(V)
        print("%s %d x %d: min q / G %.3g, cond %.4g" % (cls, n, m, ratio, cond))
        assert ratio >= 1e-8 and ratio >= 100 * er.GSF_COND_FLOOR
        assert cond <= 1.1e3
    elif cls == "zero":
        assert (ref.q == 0).sum() == 1 and ref.q[m // 2] == 0 and ref.norms[m // 2] == 0
        assert not ref.Q[:, m // 2].any()
    else:
        ratio = ref.q[m - 1] / G[m - 1]
        print("%s %d x %d: q / G of the last column %.3g" % (cls, n, m, ratio))
        assert ratio <= 1e-12 and ratio <= er.GSF_COND_FLOOR / 100
        if cls == "dup_last":
            assert X[:, m - 1].tobytes() == X[:, 1].tobytes()


def test_the_table_holds_every_class_and_shape():
    assert {c[0] for c in CASES} == set(er.CLASSES)
    assert all(("graded", n, m, ld) in {c[:4] for c in CASES} for n, m, ld in er.SHAPES if m >= 2)
    assert all(m >= 9 for cls, n, m, ld, seed in CASES if cls == "sum_last")
    assert {ld for n, m, ld in er.SHAPES} == {32, 64, 128, 256} and all(ld >= er.ld_for(m) for n, m, ld in er.SHAPES)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_cgs_against_the_oracle_and_its_own_T(c):
    cls, n, m, ld, seed = c
    X, ref = er.case(*c)
    cm = np.abs(ref.Q).max(axis=0)
    XT = X.astype(np.float64) @ ref.T
    # Q = X T: T is cgs()'s own recurrence in float64; the product cancels over the block's condition (<= 1.1e3 where it is
    # defined at all), so 1e-10 of a column's largest entry is 1e3 x 2^-53 with a factor 1e3 to spare
    cols = er.compared(cls, m)
    assert (np.abs(XT - ref.Q)[:, cols] <= 1e-10 * cm[None, cols]).all()
    assert np.allclose(ref.norms ** 2, ref.q, rtol=1e-15, atol=0) and (np.triu(ref.T) == ref.T).all()
    if cls != "zero":          # orc.orthonormalise divides by zero there
        Qo, no = orc.orthonormalise(X.T.astype(np.float64))
        err = (np.abs(Qo.T - ref.Q) / cm[None, :])[:, cols].max()
        nerr = (np.abs(no - ref.norms) / ref.norms)[cols].max()
        print("%s %d x %d: cgs vs oracle %.3g (Q, relative to the column's largest), %.3g (norms)" % (cls, n, m, err, nerr))
        assert err <= 1e-12 and nerr <= 1e-12


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_emulations_deviate_by_a_finite_amount(c):
    cls, n, m, ld, seed = c
    forms = ("panels", "panels_seq") if ld == 0 else ("gram", "seq")
    for form in forms:
        d, dn = er.emulated(*c, form=form)
        print("%s %d x %d %s: d %.3g, d_norm %.3g" % (cls, n, m, form, d, dn))
        assert np.isfinite(d) and np.isfinite(dn)
        if form == "gram":
            assert d <= 2.0 ** -24 and dn == 0.0
        # the rule's floor governs unless the emulation says otherwise; either way the tolerance stays far below a wrong column
        assert 4 * max(d, 2.0 ** -23) < 0.05


@pytest.mark.parametrize("p,m", er.RESID_SHAPES + [er.RESID_WIDE])
def test_residual_reference_and_bound(p, m):
    """residual() against orc.residual_norm; a numpy float32 evaluation of the residual stays inside residual_bound under both stored
    forms (it is a worst case summed over every entry: the float32 evaluation uses 1e-5 of it); the bound still stays small enough that
    a residual reading 5 % low is beyond it at every shape (by a factor 2 at p = 129, m = 128, where X spans all but one
    dimension and the residual is small; 4 to 48 elsewhere)."""
    A32 = er.laplacian_case(p)
    A = A32.astype(np.float64)
    assert A32.shape == (p, p) and np.array_equal(A32, A32.T)
    X32 = er.cgs(glf.random_vectors(p, m, 1).T).Q.astype(np.float32)
    X = X32.astype(np.float64)
    r_ref = er.residual(A, X)
    assert abs(orc.residual_norm(A, X.T) - r_ref) <= 1e-12 * r_ref
    r32 = er.residual_f32(A32, X32)
    ld = er.ld_for(m)
    for mode in ("f16s", "f32"):
        B = float(np.linalg.norm(er.residual_bound(A, X, ld, mode, np.zeros_like(X))))
        BE = float(np.linalg.norm(er.residual_bound(A, X, ld, mode, er.start_block_E(X))))
        print("p %d m %d %s: r %.6g, |r32 - r| %.3g = %.3g of ||B||_F %.3g (with E: %.3g)" % (p, m, mode, r_ref, abs(r32 - r_ref),
                                                                                           abs(r32 - r_ref) / B, B, BE))
        assert abs(r32 - r_ref) <= B <= BE
        assert BE <= 0.05 * r_ref


def test_named_departures():
    # PANEL_DUP_NO_FALLBACK
    c = [c for c in CASES if c[0] == "dup_last" and not c[3]][0]
    cond = []
    Q, nr = er.cgs_panels(er.case(*c)[0], cond=cond)
    print("dup_last %d x %d: min q / G per panel as its Gram-matrix form sees it: %s; last norm %.3g" % (c[1], c[2], cond, nr[-1]))
    assert len(cond) == 2 and min(cond) >= 1e-8 and nr[-1] <= 1e-5 * np.linalg.norm(er.case(*c)[0][:, -1])
    # RESID_VECTOR_CHAIN
    assert er.resid_links(200, 256) == 200 and er.resid_links(100, 128) == 100
    assert er.resid_links(5, 32) == 17 and er.resid_links(64, 64) == 33
    # RENORMALISED_INPUT: a fresh rounding of every entry moves cgs() of a well-conditioned block by about one f32 rounding
    X, ref = er.case(*[c for c in CASES if c[:3] == ("white", 129, 64)][0])
    d_in = er.renorm_deviation(X, ref)
    print("renorm_deviation of white 129 x 64: %.3g" % d_in)
    assert 0 < d_in < 2.0 ** -20
