"""The compact graph handle (glf_graph_compact / Graph.compact): Phi stored as f16 with one power-of-two scale per column, read by the
f16 instances of the handle's kernels through the second loader of csrc/phi_tile.hpp.

Shapes: those of tests/test_gpu_graph.py -- 61 x 47 = 2867 pixels (the last 32-pixel tile is partial) at ld 32 / 64 / 128 / 256, and
`tiny` (160 pixels); 509 x 515 for the tile loop.

1. The quantisation is the one include/glf.h states, bit for bit, against numpy on the f32 Phi read before compacting.
   The `scaled` variant transforms the handle first by a diagonal T with the entries 2^-20, 1, 3 * 2^10 in turn, so that neighbouring
   columns need different exponents. A column scaling leaves the ratio of an entry to its column's maximum as it was, and the
   eigenvectors of these images hold no entry below 2^-28 of their column's maximum; so the variant also multiplies the rows
   px % 7 == 3 of Phi by 2^-24 in place (the phi view, before compacting): the entries of those rows that were at 2^-15 .. 2^-5
   of the column's maximum land in the f16 subnormal range, smaller ones round to zero, and the test asserts that nonzero
   subnormals are among the stored values.
2. The contract: on a compact handle every call returns, bit for bit, what it returns on an f32 handle whose Phi is Q = dequantize()
   (the `twin`: a second build of the same image whose phi view is overwritten in place). Outputs for synthesize: the coefficients,
   identity terms and plane map of test_gpu_graph._outputs.
3. The error against the handle before compaction, derived from the format alone ("Compact graph handle"):
   |Q - Phi| <= 2^-11 |Phi| + 2^(e_c - 25) per entry, so with no identity term, componentwise,
     |out16 - out32| <= (2^-11 + 2 (ld + 4) 2^-24) (|Phi| |a|) + sum_c 2^(e_c - 25) |a_c|
   (out16 - out32 = (Q - Phi) fl32(a) + acc16 - acc32, each side's f32 accumulation error bounded as _synth_want does, by
   (ld + 4) 2^-24 |Phi| |a|: a fused chain of ld terms rounds ld times, and the 4 units of slack also cover fl32(a) and, on the
   compact side, |Q| <= (1 + 2^-11) |Phi| + 2^(e_c - 25) in place of |Phi|), and for project_wide
     |c16 - c32| <= (2^-11 + 2 eps(N)) (|t|^T |Phi|) + 2^(e_c - 25) sum_px |t|, t = fl32(w s), eps of test_gpu_graph_project_wide.
4. Graph.apply with the smoothing response 1 - lam on the three test planes, compact against f32, both on the wide route:
   max |z16 - z32| / max |z32| per shape is printed (the README records it), and the bound of test 3 applied to the chain
   project_wide -> scale -> synthesize is asserted.
5. Refusals, idempotence, determinism across builds, a Phi that is not finite, the debug pool.
6. The tile loop: 509 x 515 at ld 64, every wave runs its loop more than once.
7. The same shape: a handle that made every call as f32 before it was compacted against one compacted before its first call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _dev, _grey_graph, _outputs  # noqa: E402
from test_gpu_graph_project_wide import _eps, _planes32  # noqa: E402

LD_SHAPES = ["ld32", "ld64", "ld128", "ld256"]


def _same(a, b, what=""):
    """Bit for bit, for numpy arrays and device tensors of any one dtype."""
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ia = np.ascontiguousarray(a).view("u%d" % a.dtype.itemsize)
    ib = np.ascontiguousarray(b).view("u%d" % b.dtype.itemsize)
    bad = int(np.count_nonzero(ia != ib))
    assert bad == 0, "%s: %d of %d elements differ in bits" % (what, bad, ia.size)


def _prepare(g, variant):
    """The `scaled` variant of the module text, in place on an f32 handle."""
    if variant == "plain":
        return
    m = g.info["m"]
    diag = np.array([(2.0 ** -20, 1.0, 3.0 * 2.0 ** 10)[c % 3] for c in range(m)])
    g.transform(np.diag(diag), g.eigenvalues)
    g.phi[3::7] *= 2.0 ** -24
    torch.cuda.synchronize()


def _rule(phi32, m):
    """(e int32 [ld], half float16 [N, ld], Q float32 [N, ld]) of the f32 Phi [N, ld] by the stated rule, in numpy."""
    ld = phi32.shape[1]
    mx = np.abs(phi32).max(axis=0)
    assert np.isfinite(mx).all()
    e = np.zeros(ld, dtype=np.int32)
    for c in range(m):
        if mx[c] > 0:
            e[c] = max(int(np.frexp(mx[c])[1]) - 1, -100) - 14                   # ilogb = frexp's exponent - 1
    half = (phi32.astype(np.float64) * 2.0 ** -e.astype(np.float64)).astype(np.float16)   # the product is exact in f64; RNE, subnormals kept
    q = np.ldexp(half.astype(np.float32), e).astype(np.float32)
    return e, half, q


def _pair(ctx, shape, variant="plain"):
    """(compact handle, its f32 twin with Phi = Q, planes f64 [3, N], device planes, the f32 Phi read before compacting, e)."""
    gc, s, d_sig = _grey_graph(ctx, shape)
    _prepare(gc, variant)
    phi32 = gc.phi.cpu().numpy().copy()
    gc.compact()
    gt, _, _ = _grey_graph(ctx, shape)
    _prepare(gt, variant)
    gt.phi.copy_(gc.dequantize())
    torch.cuda.synchronize()
    assert gt.storage == glf.PHI_F32 and gc.storage == glf.PHI_F16 and gt.info["m"] == gc.info["m"]
    return gc, gt, s, d_sig, phi32, gc.column_exponents()


# ---- 1. the quantisation is the stated one -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["plain", "scaled"])
@pytest.mark.parametrize("shape", LD_SHAPES)
def test_quantisation_is_the_stated_one(shape, variant):
    w, h, _, _, m, ld = SHAPES[shape]
    n = w * h
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, shape)
        _prepare(g, variant)
        assert g.storage == glf.PHI_F32 and not g.column_exponents().any()
        phi32 = g.phi.cpu().numpy().copy()
        _same(g.dequantize(), phi32, "dequantize of an f32 handle is a copy of Phi")
        lam = g.eigenvalues.copy()
        g.compact()
        assert g.storage == glf.PHI_F16 and g.phi is None
        assert g.info == dict(pix=0, width=w, height=h, p=SHAPES[shape][3], m=m, ld=ld, phi_bytes=2 * n * ld)
        np.testing.assert_array_equal(g.eigenvalues, lam)
        e, q = g.column_exponents(), g.dequantize().cpu().numpy()
        g.close()
    want_e, half, want_q = _rule(phi32, m)
    np.testing.assert_array_equal(e, want_e)
    _same(q, want_q, "%s %s: dequantize against the rule" % (shape, variant))
    assert not q[:, m:].any() and not e[m:].any()
    top = np.abs(half[:, :m].astype(np.float64)).max(axis=0)
    assert np.all((top >= 2.0 ** 14) & (top <= 2.0 ** 15))                        # every column's largest stored magnitude (2^15: rounded up)
    # the entry error the header states
    phi64, q64 = phi32.astype(np.float64), q.astype(np.float64)
    big = np.abs(phi64) >= 2.0 ** (e.astype(np.float64) - 14)
    assert np.all(np.abs(q64 - phi64)[big] <= 2.0 ** -11 * np.abs(phi64)[big])
    assert np.all((np.abs(q64 - phi64) <= 2.0 ** (e.astype(np.float64) - 25))[~big])
    sub = (half != 0) & (np.abs(half.astype(np.float32)) < 2.0 ** -14)
    print("%s %s: exponents %d .. %d, %d nonzero f16 subnormals, %d entries rounded to zero" %
          (shape, variant, e[:m].min(), e[:m].max(), int(sub.sum()), int(((half == 0) & (phi32 != 0)).sum())))
    if variant == "scaled":
        assert len(set(e[:m].tolist())) >= 3
        assert sub.any(), "no stored value is a nonzero f16 subnormal: the case proves nothing"


# ---- 2. bit for bit against the f32 twin ---------------------------------------------------------------------------------------------

def _weight_plane(ctx, h, w):
    rng = np.random.default_rng(17)
    x = rng.uniform(0.0, 3.0, (h, w)).astype(np.float32)
    x[rng.uniform(size=(h, w)) < 0.1] = 0.0
    return _dev(ctx, x)


@pytest.mark.parametrize("variant", ["plain", "scaled"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_twin_synthesize_project_normal(shape, variant):
    w, h, _, _, m, ld = SHAPES[shape]
    rng = np.random.default_rng(11)
    with glf.Context(0) as ctx:
        gc, gt, s, d_sig, _, _ = _pair(ctx, shape, variant)
        d_w = _weight_plane(ctx, h, w)
        q64 = gt.phi.cpu().numpy()[:, :m].astype(np.float64)
        c = (q64.T @ s.T).T
        for nout in (1, 5, 32):
            a, ident, plane = _outputs(nout, gc.eigenvalues, c, rng)
            _same(gc.synthesize(a, ident, plane, d_sig), gt.synthesize(a, ident, plane, d_sig), "synthesize nout %d" % nout)
        a = _outputs(5, gc.eigenvalues, c, rng)[0]
        _same(gc.synthesize(a), gt.synthesize(a), "synthesize, no identity term")
        d32 = _dev(ctx, _planes32(h, w))
        for nplanes in (1, 5, 32):
            for wt in (None, d_w):
                _same(gc.project_wide(d32[:nplanes].contiguous(), wt), gt.project_wide(d32[:nplanes].contiguous(), wt),
                      "project_wide %d planes, weight %s" % (nplanes, wt is not None))
        four = torch.cat([d_sig, d_sig[:1]]).contiguous()
        for wt in (None, d_w):
            for planes in (None, four):
                Gc, bc = gc.normal_equations(wt, planes)
                Gt, bt = gt.normal_equations(wt, planes)
                _same(Gc, Gt, "normal_equations G")
                _same(bc, bt, "normal_equations b")
                assert np.isfinite(Gc).all() and np.array_equal(Gc, Gc.T)
        gc.close()
        gt.close()


@pytest.mark.parametrize("shape", ["ld64", "ld256"])
def test_twin_gram_robust_cluster_drivers(shape):
    w, h, _, _, m, ld = SHAPES[shape]
    rng = np.random.default_rng(29)
    with glf.Context(0) as ctx:
        gc, gt, s, d_sig, _, _ = _pair(ctx, shape)
        d_w = _weight_plane(ctx, h, w)
        # gram: the normal-equations pass with w = NULL, cached
        Gt = gt.normal_equations(None)[0]
        _same(gc.gram(), Gt, "gram")
        _same(gc.gram(), Gt, "gram, cached")
        # robust_step: at the plain fit's coefficients, with outliers in the planes
        planes = d_sig[1:3].clone()
        planes.view(2, -1)[:, ::37] += 50.0
        G0, b0 = gt.normal_equations(d_w, planes)
        a0 = glf.fit_coeffs(G0 + 1e-6 * np.trace(G0) / m * np.eye(m), b0)
        res0 = planes.view(2, -1).cpu().numpy().astype(np.float64) - a0 @ gt.phi.cpu().numpy()[:, :m].astype(np.float64).T
        sigma = list(1.4826 * np.median(np.abs(res0), axis=1))                       # the scale of the bulk: the outliers lie far beyond it
        for loss in ("huber", "tukey"):
            rc = gc.robust_step(planes, a0, loss, sigma=sigma, weight=d_w, want_weights=True, want_residuals=True)
            rt = gt.robust_step(planes, a0, loss, sigma=sigma, weight=d_w, want_weights=True, want_residuals=True)
            for name, x, y in zip(("G", "b", "loss", "mass", "w_eff", "residuals"), rc, rt):
                _same(np.float64(x) if isinstance(x, float) else x, np.float64(y) if isinstance(y, float) else y, "robust_step %s %s" % (loss, name))
            assert 0.0 < rc[3] < float(d_w.sum()) and np.isfinite(rc[2])               # some pixels were down-weighted
        # cluster steps: a non-trivial scale, centroids from rows of the embedding
        k, dim = 5, min(m, 64)
        scale = 1.0 / np.sqrt(0.05 + gc.eigenvalues[:dim])
        scale[1] = 0.0                                                                # a dropped column
        q = gt.phi.cpu().numpy()[:, :dim].astype(np.float64)
        emb = q * scale
        rows = rng.choice(q.shape[0], k, replace=False)
        unit = emb / np.maximum(np.linalg.norm(emb, axis=1, keepdims=True), 1e-300)
        prev = _dev(ctx, rng.integers(0, k, (h, w)).astype(np.int32))
        for name, fc, ft in (("cluster_step", gc.cluster_step, gt.cluster_step), ):
            xc, xt = fc(emb[rows], scale, prev), ft(emb[rows], scale, prev)
            for part, x, y in zip(("labels", "sums", "counts", "changed"), xc, xt):
                _same(np.int64(x) if isinstance(x, int) else x, np.int64(y) if isinstance(y, int) else y, "%s %s" % (name, part))
            assert xc[3] > 0 and xc[2].sum() == w * h
        for mode, kw, cent in (("weight", dict(weight=d_w), emb[rows]), ("normalize", dict(normalize=True), unit[rows]),
                               ("combined", dict(normalize=True, weight=d_w), unit[rows]), ("plain", dict(), emb[rows])):
            xc, xt = gc.cluster_step_ex(cent, scale, prev, **kw), gt.cluster_step_ex(cent, scale, prev, **kw)
            for part, x, y in zip(("labels", "sums", "counts", "mass", "changed"), xc, xt):
                _same(np.int64(x) if isinstance(x, int) else x, np.int64(y) if isinstance(y, int) else y, "cluster_step_ex %s %s" % (mode, part))
            assert xc[4] > 0
        # the drivers end to end
        for kw in (dict(), dict(normalize=True, weight=d_w)):
            lc, cc, ic = gc.segment(4, dim=dim, scale=scale, seed=5, max_iter=12, **kw)
            lt, ct, it = gt.segment(4, dim=dim, scale=scale, seed=5, max_iter=12, **kw)
            assert ic["iterations"] == it["iterations"] >= 2 and ic["converged"] == it["converged"] and ic["changed_last"] == it["changed_last"]
            _same(lc, lt, "segment labels")
            _same(cc, ct, "segment centroids")
            _same(ic["counts"], it["counts"], "segment counts")
        for sig in (sigma, None):                                                     # given, and estimated from the sampled rows
            fc, nc = gc.fit_robust(planes, d_w, "huber", sigma=sig, ridge=1e-6, max_iter=6, return_info=True)
            ft, nt = gt.fit_robust(planes, d_w, "huber", sigma=sig, ridge=1e-6, max_iter=6, return_info=True)
            assert nc["iterations"] == nt["iterations"] >= 2 and nc["converged"] == nt["converged"]
            _same(fc, ft, "fit_robust fit")
            for key in ("coeffs", "weights", "sigma", "objective"):
                _same(nc[key], nt[key], "fit_robust %s" % key)
        _same(gc.fit(d_sig, d_w, ridge=1e-6), gt.fit(d_sig, d_w, ridge=1e-6), "fit")
        gc.close()
        gt.close()


# ---- 3. the error against the uncompacted handle ---------------------------------------------------------------------------------------

def _assert_within(err, bound, what):
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: max |compact - f32| / bound %.3f" % (what, worst))
    assert np.all(err <= bound), (what, worst)
    return worst


@pytest.mark.parametrize("shape", list(SHAPES))
def test_error_against_the_uncompacted_handle(shape):
    w, h, _, _, m, ld = SHAPES[shape]
    n = w * h
    rng = np.random.default_rng(31)
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        d_w = _weight_plane(ctx, h, w)
        phi = g.phi.cpu().numpy()[:, :m].astype(np.float64)
        c = (phi.T @ s.T).T
        a = _outputs(32, g.eigenvalues, c, rng)[0]
        d32 = _dev(ctx, _planes32(h, w))
        out32 = g.synthesize(a).cpu().numpy().reshape(32, n).astype(np.float64)
        c32 = {wt is not None: g.project_wide(d32, wt) for wt in (None, d_w)}
        g.compact()
        e = g.column_exponents()[:m].astype(np.float64)
        out16 = g.synthesize(a).cpu().numpy().reshape(32, n).astype(np.float64)
        c16 = {wt is not None: g.project_wide(d32, wt) for wt in (None, d_w)}
        g.close()
    floor = 2.0 ** (e - 25)
    bound = (2.0 ** -11 + 2 * (ld + 4) * 2.0 ** -24) * (np.abs(a) @ np.abs(phi).T) + (np.abs(a) @ floor)[:, None]
    _assert_within(np.abs(out16 - out32), bound, "%s synthesize, 32 outputs" % shape)
    s32 = _planes32(h, w).reshape(32, n)
    for weighted in (False, True):
        t = (s32 * d_w.cpu().numpy().reshape(1, n) if weighted else s32).astype(np.float32).astype(np.float64)   # fl32(w s)
        bound = (2.0 ** -11 + 2 * _eps(n)) * (np.abs(t) @ np.abs(phi)) + np.abs(t).sum(axis=1)[:, None] * floor[None, :]
        _assert_within(np.abs(c16[weighted] - c32[weighted]), bound, "%s project_wide, 32 planes, weight %s" % (shape, weighted))


# ---- 4. a user-level figure --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_apply_smoothing_compact_against_f32(shape):
    """z = Phi diag(1 - lam) Phi^T s on the wide route of both handles. The bound is test 3's, link by link: dc >= |c16 - c32| by the
    project_wide bound; a = (1 - lam) c in f64, so |a16 - a32| <= |1 - lam| dc and both |a| <= |1 - lam| (|t|^T |Phi| + dc); then
    z16 - z32 = (Q - Phi) a16 + Phi (a16 - a32) + acc16 - acc32: the synthesize bound on the larger |a|, plus |Phi| |a16 - a32|."""
    w, h, _, _, m, ld = SHAPES[shape]
    n = w * h
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        phi = g.phi.cpu().numpy()[:, :m].astype(np.float64)
        resp = 1.0 - g.eigenvalues
        z32 = g.apply(d_sig, resp, ident=0.0, wide=True).cpu().numpy().reshape(3, n).astype(np.float64)
        g.compact()
        e = g.column_exponents()[:m].astype(np.float64)
        z16 = g.apply(d_sig, resp, ident=0.0).cpu().numpy().reshape(3, n).astype(np.float64)   # (a compact handle: always the wide route)
        g.close()
    floor = 2.0 ** (e - 25)
    t = s.astype(np.float32).astype(np.float64)
    dc = (2.0 ** -11 + 2 * _eps(n)) * (np.abs(t) @ np.abs(phi)) + np.abs(t).sum(axis=1)[:, None] * floor[None, :]
    c_abs = np.abs(t) @ np.abs(phi)                                                # >= |c| of either handle, up to its own rounding
    a_abs = np.abs(resp) * (c_abs + dc)
    da = np.abs(resp) * dc
    bound = (2.0 ** -11 + 2 * (ld + 4) * 2.0 ** -24) * (a_abs @ np.abs(phi).T) + (a_abs @ floor)[:, None] + da @ np.abs(phi).T
    _assert_within(np.abs(z16 - z32), bound, "%s apply, smoothing" % shape)
    rel = np.abs(z16 - z32).max(axis=1) / np.abs(z32).max(axis=1)
    print("%s apply, smoothing response: max |z16 - z32| / max |z32| per plane %s" % (shape, " ".join("%.3e" % x for x in rel)))


# ---- 5. refusals and idempotence -------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_untouched():
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld64")
        m = g.info["m"]
        g.compact()
        before = g.dequantize()
        e = g.column_exponents()
        for what, call, names in (("transform", lambda: g.transform(np.eye(m), g.eigenvalues), ("compact", "transform")),
                                  ("orthonormalize", lambda: g.orthonormalize(), ("compact", "orthonormalize")),
                                  ("project", lambda: g.project(d_sig), ("compact", "glf_graph_project_wide"))):
            with pytest.raises(glf.GlfError) as err:
                call()
            assert err.value.status == glf.ERR_UNSUPPORTED, what
            for name in names:
                assert name in str(err.value), (what, str(err.value))
            _same(g.dequantize(), before, "dequantize after the refused %s" % what)
            assert g.storage == glf.PHI_F16 and g.info["m"] == m
        with pytest.raises(glf.GlfError) as err:                                      # there is no way back
            g.compact(glf.PHI_F32)
        assert err.value.status == glf.ERR_UNSUPPORTED
        g.compact()                                                                   # a second compaction: nothing
        _same(g.dequantize(), before, "dequantize after a second compact")
        np.testing.assert_array_equal(g.column_exponents(), e)
        g2, _, _ = _grey_graph(ctx, "ld64")                                           # a second build of the same image
        g2.compact(glf.PHI_F32)                                                       # f32 on an f32 handle: nothing
        assert g2.storage == glf.PHI_F32 and g2.phi is not None
        g2.compact()
        np.testing.assert_array_equal(g2.column_exponents(), e)
        _same(g2.dequantize(), before, "the halves of two builds")
        g.close()
        g2.close()


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), -float("inf")])
def test_a_phi_that_is_not_finite_refuses_compaction(poison):
    rng = np.random.default_rng(3)
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld64")
        m = g.info["m"]
        a = rng.normal(size=(2, m))
        before = g.synthesize(a)
        keep = float(g.phi[2000, 7])
        g.phi[2000, 7] = poison
        torch.cuda.synchronize()
        with pytest.raises(glf.GlfError) as err:
            g.compact()
        assert err.value.status == glf.ERR_INVALID and "column 7" in str(err.value)
        assert g.storage == glf.PHI_F32 and g.phi is not None and g.info["phi_bytes"] == 4 * g.phi.numel()
        bad = g.synthesize(a).cpu().numpy().reshape(2, -1)                            # still an f32 handle
        assert not np.isfinite(bad[:, 2000]).any() and np.isfinite(np.delete(bad, 2000, axis=1)).all()
        g.phi[2000, 7] = keep
        torch.cuda.synchronize()
        _same(g.synthesize(a), before, "synthesize after the refused compaction")
        g.compact()                                                                   # and with the entry restored it compacts
        assert g.storage == glf.PHI_F16
        g.close()


def test_debug_pool_finds_nothing(monkeypatch):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    rng = np.random.default_rng(7)
    with glf.Context(0) as ctx:
        for shape in ("ld32", "ld256"):
            w, h, _, _, m, ld = SHAPES[shape]
            g, s, d_sig = _grey_graph(ctx, shape)
            d_w = _weight_plane(ctx, h, w)
            g.compact()
            g.dequantize()
            a = rng.normal(size=(3, m))
            g.synthesize(a, [1.0, 0.5, 0.0], [0, 1, -1], d_sig)
            g.project_wide(d_sig, d_w)
            g.normal_equations(d_w, d_sig)
            g.gram()
            g.fit(d_sig, d_w, ridge=1e-6)
            g.robust_step(d_sig[:2].contiguous(), a[:2], "tukey", sigma=1.0, weight=d_w, want_weights=True, want_residuals=True)
            g.fit_robust(d_sig[:2].contiguous(), d_w, "huber", ridge=1e-6, max_iter=3)
            dim = min(m, 64)
            cent = rng.normal(size=(3, dim)) * 1e-2
            g.cluster_step(cent)
            g.cluster_step_ex(cent, normalize=True, weight=d_w)
            g.segment(3, dim=dim, max_iter=4)
            g.segment(3, dim=dim, max_iter=4, normalize=True, weight=d_w)
            g.apply(d_sig, 1.0 - g.eigenvalues, ident=0.0)
            assert g.eigenvalues.shape == (m,)
            g.close()
        assert ctx.debug_violations() == 0


# ---- 6. the tile loop --------------------------------------------------------------------------------------------------------------

def test_many_tiles_per_wave():
    w, h, m, ld = 509, 515, 40, 64
    n = w * h
    rng = np.random.default_rng(ld)
    opt = glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        d_img = ctx.to_device(glf.synth_image(w, h, seed=3))
        gc, gt = ctx.graph(d_img, opt), ctx.graph(d_img, opt)
        assert (gc.info["m"], gc.info["ld"]) == (m, ld)
        gc.compact()
        gt.phi.copy_(gc.dequantize())
        torch.cuda.synchronize()
        d32 = _dev(ctx, _planes32(h, w))
        d_sig = d32[:3].contiguous()
        c = gt.project_wide(d_sig)
        a, ident, plane = _outputs(32, gc.eigenvalues, c, rng)
        _same(gc.synthesize(a, ident, plane, d_sig), gt.synthesize(a, ident, plane, d_sig), "synthesize, 32 outputs, %d tiles" % ((n + 31) // 32))
        _same(gc.project_wide(d32), gt.project_wide(d32), "project_wide, 32 planes")
        gc.close()
        gt.close()


# ---- 7. calls as f32, then compaction, then the same calls ------------------------------------------------------------------------------

def _every_pass(g, a, ident, plane, d_sig, d32, d_w, rng_seed):
    """Every pass over Phi that sizes its grid from a cached occupancy, and the two that do not, once each: name -> output."""
    rng = np.random.default_rng(rng_seed)
    m = g.info["m"]
    out = {"synthesize": g.synthesize(a, ident, plane, d_sig)}
    for r in (5, 40):                                                                 # one and two accumulator tiles
        R, cen = rng.normal(0.0, 1.0, (m, r)) / np.sqrt(m), rng.normal(0.0, 1e-3, (3, r))
        out["quadform r=%d" % r] = g.quadform(R, cen)
    for key, x in g.classify(a[:8], ident[:8], plane[:8], d_sig, rng.normal(0.0, 1.0, 8), want=("label", "best", "margin")).items():
        out["classify " + key] = x
    out["edges"] = g.edges()
    step = g.robust_step(d_sig[:2].contiguous(), a[:2], "huber", sigma=[30.0, 45.0], weight=d_w, want_weights=True, want_residuals=True)
    for key, x in zip(("G", "b", "loss", "mass", "w_eff", "residuals"), step):
        out["robust_step " + key] = np.float64(x) if isinstance(x, float) else x
    for key, x in zip(("labels", "sums", "counts", "changed"), g.cluster_step(rng.normal(size=(5, m)) * 1e-2)):
        out["cluster_step " + key] = np.int64(x) if isinstance(x, int) else x
    out["normal_equations G"], out["normal_equations b"] = g.normal_equations(d_w, d_sig)
    out["project_wide"] = g.project_wide(d32, d_w)
    return out


def test_calls_before_compaction_leave_no_trace():
    """Handle A makes every call once as f32, is compacted and makes them again; handle B is compacted before its first call. 509 x 515
    has more tiles than resident waves (asserted), so the occupancy a handle caches per kernel decides the grid, and with it the
    partial sums of the passes that reduce: what A cached for the f32 instances must not reach its f16 instances."""
    w, h, m, ld = 509, 515, 40, 64
    n = w * h
    opt = glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        d_img = ctx.to_device(glf.synth_image(w, h, seed=3))
        ga, gb = ctx.graph(d_img, opt), ctx.graph(d_img, opt)
        assert (ga.info["m"], ga.info["ld"]) == (m, ld)
        _same(ga.phi, gb.phi, "the two builds")
        d32 = _dev(ctx, _planes32(h, w))
        d_sig, d_w = d32[:3].contiguous(), _weight_plane(ctx, h, w)
        a, ident, plane = _outputs(32, ga.eigenvalues, ga.project_wide(d_sig), np.random.default_rng(ld))
        first = _every_pass(ga, a, ident, plane, d_sig, d32, d_w, 41)
        assert set(first) >= {"synthesize", "quadform r=40", "classify margin", "edges", "robust_step mass", "cluster_step sums", "project_wide"}
        ga.compact()
        gb.compact()
        got, want = _every_pass(ga, a, ident, plane, d_sig, d32, d_w, 41), _every_pass(gb, a, ident, plane, d_sig, d32, d_w, 41)
        assert list(got) == list(want) == list(first)
        for key in want:
            _same(got[key], want[key], "%s after f32 calls and compaction, against compaction first" % key)
        ga.close()
        gb.close()
