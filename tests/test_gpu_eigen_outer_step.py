"""The eigen-solve's outer step where it does less than it did: the orthonormalised start block kept in the context, the Gram-Schmidt
flag read after the residual's synchronise, the first PCG step enqueued without a round trip. Needs an MI355X: -m gpu.

Cache (whole path): a context that has filtered one image answers the next one, and every change of the cache key (seed, m, size) or of
the Gram-Schmidt form, bit for bit as a fresh context under the same settings does: output, float output, eigenvalues and counts.

Deferred flag (InversePowerIteration on eigen_ref.laplacian_case): a start block whose last column copies its first makes the
Gram-matrix form raise its flag on the start block, and both the default and GS=seq orthonormalise it by the column sweep. The block
the first solve makes of it is well-conditioned again (q_k / G_kk above GSF_COND_FLOOR), so the loop's own Gram-Schmidt takes the
Gram-matrix form in the default and the sweep under GS=seq: the two runs are not bit-identical beyond the first solve's block (the
eigenvalues after K = 1 differ in the last bit at p 129, m 64, and the residuals at 1e-8, with the commit before this one too).
Asserted instead, after exactly K = 1 and 2 outer iterations: everything finite, the block returned at K = 1 bit-identical to
GS=seq's, the residual within eigen_ref.residual_bound of the float64 residual of cgs(V) (E from the larger deviation of the two
Gram-Schmidt forms, either may have run), and a second run the same bits.

First step without a synchronise: that is the solver's own; glf_operator_solve, whose right-hand side may be zero, keeps the round
trip -- an all-zero block takes 0 steps and answers zeros, one zero column among others stays frozen while the others are solved to
the same bits as without it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import eigen_ref as er  # noqa: E402
import operator_ref as oref  # noqa: E402
import test_gpu_operator as top  # noqa: E402
from test_gpu_operator import _bits, _operator  # noqa: E402

COUNTS = ("p", "m", "outer_its", "inner_its_total", "matvecs")


def _context():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return glf.Context(0)


# ---- the cached start block -------------------------------------------------------------------------------------------------------

def _image(side, seed):
    return glf.synth_image(side, side, seed=seed)


def _filter(ctx, img, m, seed=1):
    h, w = img.shape
    opt = glf.default_options(num_samples=max(64, (w * h) // 100), num_eigvals=m, seed=seed)
    out, zf, info = ctx.image_processing(ctx.to_device(img), opt, want_float=True)
    return out.cpu().numpy(), zf.cpu().numpy(), info


def _fresh(img, m, seed=1, **tuning):
    with _context() as c:
        c.set_tuning(**tuning)
        return _filter(c, img, m, seed)


def _assert_same(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": u8 output")
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]), err_msg=what + ": float output")
    np.testing.assert_array_equal(np.asarray(got[2]["eigvals"]).view(np.uint64), np.asarray(want[2]["eigvals"]).view(np.uint64),
                                  err_msg=what + ": eigenvalues")
    for k in COUNTS:
        assert got[2][k] == want[2][k], (what, k, got[2][k], want[2][k])


@pytest.mark.parametrize("m", [20, 64], ids=["m20-ld32", "m64-ld64"])
def test_cached_start_block_answers_as_a_fresh_context(m):
    img1, img2, small = _image(256, 3), _image(256, 4), _image(128, 5)
    with _context() as a:
        first = _filter(a, img1, m)
        assert first[2]["outer_its"] >= 1 and np.isfinite(first[1]).all()
        _assert_same(_filter(a, img2, m), _fresh(img2, m), "second image of one size")           # a hit
        _assert_same(_filter(a, img1, m), first, "the first image again")                         # a hit gives the miss's bits
        _assert_same(_filter(a, img2, m, seed=7), _fresh(img2, m, seed=7), "another seed")
        m2 = 32 if m == 20 else 48
        _assert_same(_filter(a, img2, m2, seed=7), _fresh(img2, m2, seed=7), "another m")
        _assert_same(_filter(a, small, m2, seed=7), _fresh(small, m2, seed=7), "another size")
        a.set_tuning(GS="seq")
        _assert_same(_filter(a, small, m2, seed=7), _fresh(small, m2, seed=7, GS="seq"), "GS=seq on the same key")
        _assert_same(_filter(a, small, m2, seed=7), _fresh(small, m2, seed=7, GS="seq"), "GS=seq again")
        a.reset_tuning()
        _assert_same(_filter(a, small, m2, seed=7), _fresh(small, m2, seed=7), "after reset_tuning")


# ---- the Gram-Schmidt flag, read after the residual ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = _context()
    c.mats = {}
    yield c
    c.destroy(*c.mats.values())
    c.close()


def _solve(ctx, p, m, K, X0, gs=None):
    if p not in ctx.mats:
        ctx.mats[p] = ctx.dense_from_numpy(er.laplacian_case(p), ld=oref.round_up(p, 64))
    ctx.set_tuning(GS=gs)
    try:
        vecs, vals, st = ctx.InversePowerIteration(ctx.mats[p], m, epsilon=1e-30, max_outer=K, allow_noconv=True, X0=X0)
    finally:
        ctx.set_tuning(GS=None)
    assert st["outer_its"] == K
    out = (ctx.mat_to_numpy(vecs), ctx.mat_to_numpy(vals), st["residual"], st["inner_its_total"])
    ctx.destroy(vecs, vals)
    return out


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("p,m", [(129, 5), (129, 64), (1000, 5), (1000, 64)])
def test_deferred_flag_takes_the_fallback(ctx, p, m, K):
    X0 = glf.random_vectors(p, m, 1)
    X0[m - 1] = X0[0]
    V, lam, r, its = _solve(ctx, p, m, K, X0)
    Vs, lams, rs, its_s = _solve(ctx, p, m, K, X0, gs="seq")
    assert V.shape == (p, m) and np.isfinite(V).all() and np.isfinite(lam).all() and np.isfinite(r)
    if K == 1:     # the block returned is the first solve's, from the start block both runs orthonormalised by the column sweep
        np.testing.assert_array_equal(_bits(V), _bits(Vs))        # (the eigenvalues are the last Gram-Schmidt's norms: its form's)
        assert its == its_s
    A = er.laplacian_case(p).astype(np.float64)
    ref = er.cgs(V)
    d = max(er.renorm_deviation(V, ref), *(er.deviation(f[0], f[1], ref)[0] for f in (er.cgs_gram_f32(V), er.cgs_sweep_f32(V))))
    r_ref = er.residual(A, ref.Q)
    B = float(np.linalg.norm(er.residual_bound(A, ref.Q, er.ld_for(m), "f16s", er.orthonormalised_E(ref, d))))
    print("p %d m %d K %d: residual %.9g (GS=seq %.9g, fp64 %.9g), |r - r_ref| %.3g of the bound %.3g, %d inner iterations (%d)" % (
        p, m, K, r, rs, r_ref, abs(r - r_ref), B, its, its_s))
    assert abs(r - r_ref) <= B
    V2, lam2, r2, its2 = _solve(ctx, p, m, K, X0)          # and the same bits a second time
    np.testing.assert_array_equal(_bits(V2), _bits(V))
    np.testing.assert_array_equal(_bits(lam2), _bits(lam))
    assert r2 == r and its2 == its


# ---- glf_operator_solve keeps its round trip ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def octx():
    c = _context()
    c.set_contraction(glf.CONTRACT_F16_SPLIT)
    c.mode, c.graphs = "f16s", {}
    yield c
    for d_img, K_B, L_B, alpha, D in c.graphs.values():
        c.destroy(K_B)
    c.close()


@pytest.mark.parametrize("form", ["dense", "band"])
def test_operator_solve_with_zero_columns(octx, form):
    shape, ld, m = "edge128", 64, 59
    p = top._ref(shape).p
    L_B = top._grey(octx, shape)[2]
    rows = oref.round_up(p, 64)
    B = np.zeros((rows, ld), dtype=np.float32)
    B[:p, :m] = np.random.default_rng(11).standard_normal((p, m)).astype(np.float32)
    try:
        with _operator(octx, form, L_B, ld_hint=ld) as op:
            X0, R0, info0 = op.solve_numpy(np.zeros_like(B), m, 1e-5, max_it=100)
            assert info0["iters"] == 0 and info0["unconverged"] == 0 and info0["matvecs"] == 0
            assert not X0.any() and not R0.any()
            X, R, info = op.solve_numpy(B, m, 1e-5, max_it=100)
            assert info["status"] == glf.OK and info["unconverged"] == 0 and info["iters"] >= 1
            Bz = B.copy()
            Bz[:, 3] = 0.0
            Xz, Rz, infoz = op.solve_numpy(Bz, m, 1e-5, max_it=100)
            assert infoz["status"] == glf.OK and infoz["unconverged"] == 0 and 1 <= infoz["iters"] <= info["iters"]
            assert not Xz[:, 3].any() and not Rz[:, 3].any()                     # frozen from the start
            others = [c for c in range(ld) if c != 3]
            np.testing.assert_array_equal(_bits(Xz[:, others]), _bits(X[:, others]))
            np.testing.assert_array_equal(_bits(Rz[:, others]), _bits(R[:, others]))
            rr = (Rz[:p].astype(np.float64) ** 2).sum(axis=0)
            bn2 = (Bz[:p].astype(np.float64) ** 2).sum(axis=0)
            assert (rr[:m] <= 1e-10 * bn2[:m] * (1 + 1e-12)).all()              # the stopping rule, every column
    finally:
        octx.reset_tuning()
