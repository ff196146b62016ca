"""The eigen-solve's carried operand maxima and its column-split second-level reductions. Needs an MI355X: -m gpu.

1. Carried maxima equal swept maxima. The kernels that write an operand of the block PCG (k_cg_init, k_cg_pupdate, k_cg_pack) leave
   the block maxima of |operand| behind, and the band-form operator takes its per-column scales from them instead of reading the block
   again (k_col_absmax_part). OPERAND_MAXIMA=sweep makes the operator find them itself. A maximum does not depend on the order or the
   partition, so the two settings are the same computation: u8 output, float output, eigenvalues and the iteration counts bit for bit.
   The sample counts are no multiples of the 128 block rows (the ragged last block); the 1024^2 cases issue narrow sweeps (k_cg_pack's
   maxima, packed widths 32 and 64 below ld 64 / 128).

2. The second-level reductions (wg_reduce_partials: 8 columns per workgroup, 128 thread rows, 8 blocks a batch) where a reduction goes
   wrong: p = 100 (one block: 127 thread rows have nothing), 129 (a second block of one row), 1000 (8 blocks), 2601 (21 blocks); m = 5
   (ld 32, 27 padding columns whose sums and maxima are zero), 64, 100 (ld 128). InversePowerIteration on the stored float64-oracle
   Laplacian of tests/eigen_ref.py for exactly K = 1 and 2 outer iterations, the way tests/test_gpu_residual.py drives it, against the
   float64 evaluation with that module's bounds: |r_sweep - r_ref| <= ||residual_bound||_F, |r_derived - r_sweep| <= derived_bound;
   the vectors and eigenvalues of the two residual modes bit-identical (the same iterates), and a second run of each the same bits
   (the sums keep a fixed order). The entry point takes 0 < m < p: at (p 100, m 100) the test holds it to its refusal.

3. The outer loop without its block copies. By default the PCG leaves its solution Y where it built it, A X_new = (B - R) Tn and X_new =
   Y Tn are written out of place and the buffers are swapped; RESIDUAL=sweep and GS=seq keep the copies and the in-place map. The same
   operations on the same operands: the bit-identity of the two residual modes in part 2 is that check, and GS=seq is held to the
   float64 evaluation with its own deviation d (cgs_sweep_f32), both of its modes being the explicit sweep."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import eigen_ref as er  # noqa: E402
import operator_ref as oref  # noqa: E402


# ---- 1. carried against swept maxima ------------------------------------------------------------------------------------------------

# size, sample fraction, m, epsilon, narrow sweeps expected
WHOLE_PATH = [(256, 0.01, 20, 0.1, False), (256, 0.01, 64, 0.1, False), (1024, 0.005, 64, 0.05, True), (1024, 0.005, 100, 0.05, True)]


def _whole_path_both_ways(size, frac, m, eps, narrow, mv):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    img = glf.synth_image(size, size, seed=5)
    res = {}
    for maxima in (None, "sweep"):
        c = glf.Context(0)
        try:
            c.set_tuning(MV_PATH=mv, OPERAND_MAXIMA=maxima)
            opt = glf.default_options(num_samples=int(size * size * frac), num_eigvals=m, epsilon=eps)
            out, zf, info = c.image_processing(c.to_device(img), opt, want_float=True)
            res[maxima] = (out.cpu().numpy(), zf.cpu().numpy(), info)
        finally:
            c.close()
    a, b = res[None], res["sweep"]
    print("%d^2 m %d: p %d, %d outer iterations, %d sweeps, %d of them narrow" % (size, m, a[2]["p"], a[2]["outer_its"], a[2]["matvecs"],
                                                                               a[2]["narrow_sweeps"]))
    assert a[2]["matvec_path"] == {"band": 4, "rank": 3, "grid": 1}[mv] and a[2]["p"] % 128 != 0
    if narrow:
        assert a[2]["narrow_sweeps"] > 0
    for k in ("outer_its", "inner_its_total", "matvecs", "narrow_sweeps"):
        assert a[2][k] == b[2][k], k
    np.testing.assert_array_equal(a[2]["eigvals"].view(np.int64), b[2]["eigvals"].view(np.int64))
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32))
    np.testing.assert_array_equal(a[0], b[0])


@pytest.mark.parametrize("size,frac,m,eps,narrow", WHOLE_PATH, ids=["256-m20", "256-m64", "1024-m64", "1024-m100"])
def test_carried_maxima_equal_swept_maxima(size, frac, m, eps, narrow):
    _whole_path_both_ways(size, frac, m, eps, narrow, "band")


@pytest.mark.parametrize("mv", ["grid", "rank"])
def test_grid_and_rank_forms_take_the_carried_maxima(mv):
    """The two grid-factored forms feed the carried block maxima to their own second level (k_col_absmax_fin): the same identity."""
    _whole_path_both_ways(256, 0.01, 64, 0.1, True, mv)


# ---- 2. the second-level reductions -------------------------------------------------------------------------------------------------

PS = (100, 129, 1000, 2601)
MS = (5, 64, 100)
KS = (1, 2)


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    c.mode = "f16s"          # the default contraction: the stored L_A is swept by k_block_matvec_f16s
    c.mats = {}
    yield c
    c.destroy(*c.mats.values())
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _solve(ctx, p, m, K, residual=None, gs=None):
    if p not in ctx.mats:
        ctx.mats[p] = ctx.dense_from_numpy(er.laplacian_case(p), ld=oref.round_up(p, 64))
    ctx.set_tuning(RESIDUAL=residual, GS=gs)
    try:
        vecs, vals, st = ctx.InversePowerIteration(ctx.mats[p], m, inner_rtol=1e-5, X0=glf.random_vectors(p, m, 1), epsilon=1e-30,
                                                   max_outer=K, allow_noconv=True)
    finally:
        ctx.set_tuning(RESIDUAL=None, GS=None)
    assert st["outer_its"] == K
    got = (ctx.mat_to_numpy(vecs), ctx.mat_to_numpy(vals), st["residual"], st["inner_its_total"])
    ctx.destroy(vecs, vals)
    return got


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("p", PS)
def test_second_level_reductions(ctx, p, m):
    if m >= p:      # (p 100, m 100): the entry point takes 0 < m < p only and says so; no kernel runs
        with pytest.raises(glf.GlfError) as refusal:
            _solve(ctx, p, m, 1)
        assert refusal.value.status == glf.ERR_INVALID and "m < p" in str(refusal.value)
        return
    A = er.laplacian_case(p).astype(np.float64)
    its_before = 0
    for K in KS:
        Vd, ld_, rd, its_d = _solve(ctx, p, m, K, "derived")
        Vs, ls_, rs, its_s = _solve(ctx, p, m, K, "sweep")
        assert Vd.shape == (p, m) and np.isfinite(Vd).all() and np.isfinite(ld_).all()
        # the two residual modes are the same iterates
        np.testing.assert_array_equal(_bits(Vd), _bits(Vs))
        np.testing.assert_array_equal(_bits(ld_), _bits(ls_))
        assert its_d == its_s
        # fixed order: a second run gives the same bits, residual included
        for mode, first in (("derived", (Vd, ld_, rd, its_d)), ("sweep", (Vs, ls_, rs, its_s))):
            V2, l2, r2, its2 = _solve(ctx, p, m, K, mode)
            np.testing.assert_array_equal(_bits(V2), _bits(first[0]))
            np.testing.assert_array_equal(_bits(l2), _bits(first[1]))
            assert r2 == first[2] and its2 == first[3]
        # against float64: the returned block is the normalised pre-orthonormalisation block Y, the residual is that of cgs(Y).Q
        ref = er.cgs(Vs)
        form = er.cgs_gram_f32(Vs)
        d = max(er.deviation(form[0], form[1], ref)[0], er.renorm_deviation(Vs, ref))
        r_ref = er.residual(A, ref.Q)
        B = float(np.linalg.norm(er.residual_bound(A, ref.Q, er.ld_for(m), ctx.mode, er.orthonormalised_E(ref, d))))
        its = its_s - its_before
        assert its >= 1
        bd = er.derived_bound(A, Vs, ref.T, its, ctx.mode)
        print("p %d m %d K %d: sweep %.9g, fp64 %.9g, difference %.3g of the bound %.3g; derived %.9g, %d inner iterations, difference "
              "from the sweep %.3g of the bound %.3g" % (p, m, K, rs, r_ref, abs(rs - r_ref), B, rd, its, abs(rd - rs), bd))
        assert np.isfinite(rs) and abs(rs - r_ref) <= B
        assert np.isfinite(rd) and abs(rd - rs) <= bd
        its_before = its_s
        # 3. GS=seq keeps the block copies of the outer loop and has no triangular map: both residual modes are the explicit sweep,
        # bit for bit, and the result stands against float64 with the column-by-column sweep's own deviation d
        Vq, lq, rq, _ = _solve(ctx, p, m, K, "derived", "seq")
        Vqs, lqs, rqs, _ = _solve(ctx, p, m, K, "sweep", "seq")
        np.testing.assert_array_equal(_bits(Vq), _bits(Vqs))
        np.testing.assert_array_equal(_bits(lq), _bits(lqs))
        assert rq == rqs
        refq = er.cgs(Vq)
        formq = er.cgs_sweep_f32(Vq)
        dq = max(er.deviation(formq[0], formq[1], refq)[0], er.renorm_deviation(Vq, refq))
        rq_ref = er.residual(A, refq.Q)
        Bq = float(np.linalg.norm(er.residual_bound(A, refq.Q, er.ld_for(m), ctx.mode, er.orthonormalised_E(refq, dq))))
        print("p %d m %d K %d GS=seq: sweep %.9g, fp64 %.9g, difference %.3g of the bound %.3g (d %.3g)" % (p, m, K, rq, rq_ref,
                                                                                                       abs(rq - rq_ref), Bq, dq))
        assert np.isfinite(rq) and abs(rq - rq_ref) <= Bq
