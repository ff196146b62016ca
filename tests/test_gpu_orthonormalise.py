"""OrthonormaliseVecs and NormaliseVecs through the C-ABI, in the Gram-matrix form (the default), as the column-by-column sweep (GS=seq
and the ill-conditioning fallback) and over panels of 256 vectors, against classical Gram-Schmidt in float64. Needs an MI355X: -m gpu.

Reference, emulations, blocks, shapes and the tolerance rule: tests/eigen_ref.py (its docstring holds the rounding points of each form
with the code they come from); tests/test_eigen_ref.py asserts on the CPU that every block meets the conditions that decide which form
the device must take. The tolerance comes from the reference, not from the kernels: with d the largest deviation of the form's numpy
emulation from cgs(), the device must agree with cgs() within 4 max(d, 2^-23) max|Q_ref[:, k]| in every entry of column k; norms within
relative 2^-24 (Gram-matrix form) or 4 max(d_norm, 2^-24) (sweep; panels, whose norms come after f32 rounding points as the sweep's do).

Set GLF_EIGEN_ERROR_JSON to a path to have the largest error / tolerance per family written there (tools/eigen_blocks_error.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import eigen_ref as er  # noqa: E402

CASES = er.cases()
NARROW = [c for c in CASES if c[0] in ("white", "graded") and c[3]]
STRUCT = [c for c in CASES if c[0] in ("zero", "dup_last", "sum_last") and c[3]]
WIDE = [c for c in CASES if c[0] == "white" and not c[3]]
WIDE_DUP = [c for c in CASES if c[0] == "dup_last" and not c[3]]


def _id(c):
    return "%s-%dx%d-ld%d" % c[:4]


@pytest.fixture(scope="module", params=["f16s", "f32"])
def ctx(request):
    """Both contraction modes, as in test_gpu_parity.py (neither block contracts with K_B: the kernels are the same in both)."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    c.set_contraction(glf.CONTRACT_F16_SPLIT if request.param == "f16s" else glf.CONTRACT_F32_MFMA)
    c.mode = request.param
    c.runs = {}
    yield c
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


def _upload(ctx, X, ld, pad=0.0):
    """The block on the device with leading dimension ld (0: what dense_from_numpy chooses), columns m .. ld - 1 filled with `pad`."""
    n, m = X.shape
    if not ld:
        return ctx.dense_from_numpy(X)
    full = np.full((n, ld), pad, dtype=np.float32)
    full[:, :m] = X
    mat = ctx.dense_from_numpy(full, ld=ld)
    mat.cols = m
    return mat


def _run(ctx, c, gs=None, pad=0.0, normalise=False):
    """(the block as stored [n, ld], norms) after OrthonormaliseVecs / NormaliseVecs on a row of the table, run once per context."""
    key = (c, gs, pad, normalise)
    if key not in ctx.runs:
        X, _ = er.case(*c)
        ctx.set_tuning(GS=gs)
        mat = _upload(ctx, X, c[3], pad)
        norms = (ctx.NormaliseVecs if normalise else ctx.OrthonormaliseVecs)(mat)
        full = ctx.mat_to_numpy(mat, padded=True)
        ctx.destroy(mat)
        ctx.set_tuning(GS=None)
        assert norms.shape == (c[2],) and full.shape[0] == c[1]
        ctx.runs[key] = (full, norms)
    return ctx.runs[key]


def _check(ctx, c, full, norms, form, family, cols=None, gram_norms=False):
    """The tolerance rule on the columns `cols` (default: all) of one result; returns the worst error / tolerance."""
    cls, n, m, ld, seed = c
    _, ref = er.case(*c)
    d, dn = er.emulated(*c, form=form)
    Q = full[:, :m].astype(np.float64)
    sel = np.arange(m)[slice(0, m) if cols is None else cols]
    tol = er.q_tol(ref, d)
    err = np.abs(Q - ref.Q).max(axis=0)
    rtol = er.norm_rtol(None if gram_norms else dn)
    nz = sel[ref.norms[sel] > 0]
    nerr = float((np.abs(norms[nz] - ref.norms[nz]) / ref.norms[nz]).max()) if nz.size else 0.0
    live = sel[tol[sel] > 0]
    ratio = float((err[live] / tol[live]).max()) if live.size else 0.0
    print("%s %s %s: d %.3g, worst |Q - Q_ref| / tol %.3f; norms %.3g against %.3g" % (ctx.mode, _id(c), form, d, ratio, nerr, rtol))
    er.record(family, ctx.mode, "%s %s" % (_id(c), form), float((err[live] / np.abs(ref.Q).max(axis=0)[live]).max()) if live.size else 0.0,
              4.0 * max(d, 2.0 ** -23), d)
    er.record(family + " norms", ctx.mode, "%s %s" % (_id(c), form), nerr, rtol, dn)
    assert np.isfinite(full).all() and np.isfinite(norms).all()
    bad = sel[err[sel] > tol[sel]]
    assert bad.size == 0, "%d columns beyond the tolerance, first %d: error %.3e, tolerance %.3e" % (bad.size, bad[0], err[bad[0]], tol[bad[0]])
    assert nerr <= rtol, (nerr, rtol)
    return ratio


@pytest.mark.parametrize("gs", [None, "seq"], ids=["gram", "seq"])
@pytest.mark.parametrize("c", NARROW, ids=_id)
def test_against_cgs(ctx, c, gs):
    """white and graded blocks at every shape, in both forms. The graded blocks (cond 1e3, q / G down to 3e-5, column scales 2^-20 ..
    2^20) pass the Gram-matrix form's 2^-21 only if that form ran: the sweep's own d is 1e-3 there."""
    cls, n, m, ld, seed = c
    full, norms = _run(ctx, c, gs)
    assert full.shape == (n, ld) and not full[:, m:].any()
    form = "seq" if gs else "gram"
    _check(ctx, c, full, norms, form, "%s ld %d" % ("sweep" if gs else "gram", ld), gram_norms=not gs)
    if cls == "white" and not gs:
        Q = full[:, :m].astype(np.float64)
        defect = np.abs(Q.T @ Q - np.eye(m)).max()
        er.record("gram orthogonality", ctx.mode, _id(c), defect, (m + 4) * 2.0 ** -23)
        assert defect <= (m + 4) * 2.0 ** -23


@pytest.mark.parametrize("c", NARROW, ids=_id)
def test_normalise(ctx, c):
    cls, n, m, ld, seed = c
    X, _ = er.case(*c)
    full, norms = _run(ctx, c, normalise=True)
    ref = np.linalg.norm(X.astype(np.float64), axis=0)
    nerr = float((np.abs(norms - ref) / ref).max())
    unit = float(np.abs(np.linalg.norm(full[:, :m].astype(np.float64), axis=0) - 1.0).max())
    er.record("normalise norms", ctx.mode, _id(c), nerr, 2.0 ** -24)
    er.record("normalise unit length", ctx.mode, _id(c), unit, 2.0 ** -22)
    assert nerr <= 2.0 ** -24 and unit <= 2.0 ** -22
    # direction: the norm within 2^-24, one division in f64 and one rounding to f32
    assert (np.abs(full[:, :m].astype(np.float64) - X.astype(np.float64) / ref) <= 2.0 ** -22 * np.abs(X / ref)).all()
    assert not full[:, m:].any()


@pytest.mark.parametrize("gs", [None, "seq"], ids=["gram", "seq"])
@pytest.mark.parametrize("c", [c for c in STRUCT if c[0] == "zero"], ids=_id)
def test_zero_column(ctx, c, gs):
    """Both forms take a zero column by an explicit branch: it comes back zero with norm exactly 0, the others as without it."""
    cls, n, m, ld, seed = c
    full, norms = _run(ctx, c, gs)
    assert norms[m // 2] == 0.0 and not _bits(full[:, m // 2]).any()
    _check(ctx, c, full, norms, "seq" if gs else "gram", "%s ld %d" % ("sweep" if gs else "gram", ld), gram_norms=not gs)


@pytest.mark.parametrize("c", [c for c in STRUCT if c[0] != "zero"], ids=_id)
def test_dependent_last_column_falls_back(ctx, c):
    """A dependent last column under the default setting: bit-identical to GS=seq (the fallback ran, and the fused attempt left X
    untouched); the earlier columns and norms within the sweep's tolerance of cgs(); the last norm at most 1e-5 |v_(m-1)|; its
    direction is rounding noise and is not compared."""
    cls, n, m, ld, seed = c
    X, ref = er.case(*c)
    full, norms = _run(ctx, c)
    full_seq, norms_seq = _run(ctx, c, "seq")
    assert np.isfinite(full).all() and np.isfinite(norms).all()
    vlast = np.linalg.norm(X[:, m - 1].astype(np.float64))
    print("%s %s: last norm %.3g of |v| %.3g" % (ctx.mode, _id(c), norms[m - 1], vlast))
    assert norms[m - 1] <= 1e-5 * vlast
    _check(ctx, c, full, norms, "seq", "fallback", cols=er.compared(cls, m))
    np.testing.assert_array_equal(_bits(full), _bits(full_seq))
    np.testing.assert_array_equal(norms.view(np.uint64), norms_seq.view(np.uint64))


@pytest.mark.parametrize("c", [c for c in NARROW if c[0] == "white" and c[1:4] in er.PAD_SHAPES], ids=_id)
@pytest.mark.parametrize("how", ["gram", "seq", "normalise"])
def test_padding_columns_are_neither_read_nor_written(ctx, c, how):
    """Columns m .. ld - 1 filled with 7.0 come back bit-identical, and columns 0 .. m - 1 and the norms are bit-identical to the run
    with zero padding."""
    cls, n, m, ld, seed = c
    gs, normalise = ("seq" if how == "seq" else None), how == "normalise"
    full0, norms0 = _run(ctx, c, gs, normalise=normalise)
    full7, norms7 = _run(ctx, c, gs, pad=7.0, normalise=normalise)
    assert ld > m
    np.testing.assert_array_equal(_bits(full7[:, m:]), _bits(np.full((n, ld - m), 7.0, dtype=np.float32)))
    np.testing.assert_array_equal(_bits(full7[:, :m]), _bits(full0[:, :m]))
    np.testing.assert_array_equal(norms7.view(np.uint64), norms0.view(np.uint64))


@pytest.mark.parametrize("c", WIDE, ids=_id)
def test_more_than_256_vectors(ctx, c):
    """One-column last panel, two panels, three panels: k_gsf_gram with a second operand, k_gsf_sub and the panel loop."""
    cls, n, m, ld, seed = c
    full, norms = _run(ctx, c)
    assert full.shape == (n, er.PANEL * -(-m // er.PANEL)) and not full[:, m:].any()
    _check(ctx, c, full, norms, "panels", "panels")


@pytest.mark.parametrize("gs", [None, "seq"], ids=["gram", "seq"])
@pytest.mark.parametrize("c", WIDE_DUP, ids=_id)
def test_more_than_256_vectors_dependent_last_column(ctx, c, gs):
    """The last column of the second panel a copy of column 1 of the first. The cross-panel subtraction leaves rounding noise of it,
    which the panel's own Gram-matrix form finds well conditioned: no fallback, and no bit-identity with GS=seq, under which the first
    panel takes the sweep as well (PANEL_DUP_NO_FALLBACK in tests/test_eigen_ref.py, asserted there on the emulation). Each run against
    cgs() under its own emulation's d on the columns before the last; the last norm at most 1e-5 |v|; everything finite."""
    cls, n, m, ld, seed = c
    X, ref = er.case(*c)
    full, norms = _run(ctx, c, gs)
    vlast = np.linalg.norm(X[:, m - 1].astype(np.float64))
    print("%s %s %s: last norm %.3g of |v| %.3g" % (ctx.mode, _id(c), gs, norms[m - 1], vlast))
    assert norms[m - 1] <= 1e-5 * vlast
    _check(ctx, c, full, norms, "panels_seq" if gs else "panels", "panels sweep" if gs else "panels", cols=er.compared(cls, m))
