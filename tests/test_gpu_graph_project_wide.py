"""The wide projection on a graph handle: glf_graph_project_wide (k_graph_project_wide: c_k = Phi^T diag(w) s_k for up to 32 planes in
one pass over Phi on v_mfma_f32_32x32x2_f32, t = fl32(w s) against Phi as stored, f32 chains of C = glf.GRAPH_NORMAL_CHAIN pixel terms
added into f64), Graph.project_wide on top of it, and Graph.apply / Graph.fit beyond 4 planes.

Shapes: those of tests/test_gpu_graph.py. 61 x 47 = 2867 pixels = 89 whole 32-pixel tiles and one of 19 pixels, at ld 32 / 64 / 128
(one column group) and 256 (two groups of 128 columns); `tiny` is 160 pixels, fewer tiles than two workgroups have waves. 509 x 515
has more tiles than the largest grid has waves, so every wave runs its tile loop and flushes whole chains.

The bound, from the reference alone: componentwise
  |c - c64| <= ((C + 3) 2^-24 + N 2^-51) (|w s|^T |Phi|)
The products inside the MFMA are fused, so an f32 chain of C terms has C rounded additions; one more rounding is fl32(w s); two units
cover the 1 / (1 - n u) factor of the first-order bound; the f64 term is the summation bound of the flushed chains and of the
reference, the form of the existing bound on b (tests/test_gpu_graph_fit.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _bits, _grey_graph, _phi64, _synth_want  # noqa: E402
from test_gpu_graph_fit import RIDGE, SMOOTH, WEIGHTS, _coeff_bound, _dev_weight, _reference, _weight  # noqa: E402
from test_gpu_pix_signals import _test_planes  # noqa: E402

C = glf.C
CHAIN = glf.GRAPH_NORMAL_CHAIN
K = glf.GRAPH_MAX_PLANES


def _eps(n):
    return (CHAIN + 3) * 2.0 ** -24 + n * 2.0 ** -51


def _planes32(h, w, count=K):
    """float32 [count, h, w]: the three test planes, then seeded noise planes (sigma 30, signed), every third on an offset of 5000
    and every third of the rest negated and scaled by 100."""
    rng = np.random.default_rng(23)
    extra = rng.normal(0.0, 30.0, (count - 3, h, w))
    extra[0::3] += 5000.0
    extra[1::3] *= -100.0
    return np.concatenate([_test_planes(h, w), extra.astype(np.float32)]).astype(np.float32)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _same(a, b, msg=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _want(phi, w, s):
    """(c64 [k, m], the bound [k, m]) in numpy f64 of planes s [k, N] float64; w None = 1."""
    ws = s if w is None else w.astype(np.float64)[None, :] * s
    return ws @ phi, _eps(phi.shape[0]) * (np.abs(ws) @ np.abs(phi))


def _assert_c(c, c64, bound, what):
    err = np.abs(c - c64)
    print("%s: max |c - c64| / bound %.3f (max err %.3e)" % (what, float((err / np.maximum(bound, 1e-300)).max()), float(err.max())))
    assert c.shape == c64.shape, what
    assert np.all(err <= bound), what


# ---- 1. against fp64 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_project_wide_against_fp64(shape, kind):
    width, h = SHAPES[shape][:2]
    few = (1, 5, 17)[(list(SHAPES).index(shape) + WEIGHTS.index(kind)) % 3]
    sig = _planes32(h, width)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi64(g)
        w = _weight(kind, phi.shape[0])
        d_w, d_sig = _dev_weight(ctx, w, h, width), _dev(ctx, sig)
        got = {K: g.project_wide(d_sig, d_w), few: g.project_wide(d_sig[:few].contiguous(), d_w)}
        g.close()
    s = sig.reshape(K, -1).astype(np.float64)
    for k, c in got.items():
        c64, bound = _want(phi, w, s[:k])
        _assert_c(c, c64, bound, "%s %s nplanes %d" % (shape, kind, k))
    if kind == "zeros":
        assert not got[K].any() and not got[few].any()


# ---- 2. single entries: the transposition, the pitch and the tail ---------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld32", "ld64", "ld128", "ld256"])
def test_single_entries_give_the_rows_of_phi(shape):
    width, h, _, _, m, _ = SHAPES[shape]
    n = width * h
    where = {0: 0, 5: 31, 9: 32, 17: 1501, 30: 2848, 31: 2866}                   # slot: pixel (2848: the first of the partial tile)
    sig = np.zeros((K, n), dtype=np.float32)
    for slot, px in where.items():
        sig[slot, px] = 1.0
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi64(g)
        d_sig = _dev(ctx, sig.reshape(K, h, width))
        plain = g.project_wide(d_sig)
        twice = g.project_wide(d_sig, torch.full((h, width), 2.0, dtype=torch.float32, device=ctx.device))
        g.close()
    assert plain.shape == (K, m)
    for slot in range(K):
        want = phi[where[slot]] if slot in where else np.zeros(m)
        np.testing.assert_array_equal(plain[slot], want, err_msg="slot %d" % slot)
        np.testing.assert_array_equal(twice[slot], 2.0 * want, err_msg="slot %d, weight 2" % slot)


# ---- 3. independence and repeatability ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld64", "ld256"])
def test_a_plane_depends_on_nothing_beside_it(shape):
    width, h = SHAPES[shape][:2]
    n = width * h
    sig = _planes32(h, width, 40)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        d_sig = _dev(ctx, sig)
        d_w = _dev_weight(ctx, _weight("uniform", n), h, width)
        P = 2                                                                    # the depth-like plane

        def at(slot, count):
            """the planes 3 .. with plane P put into `slot` of `count`"""
            idx = [3 + j for j in range(count)]
            idx[slot] = P
            return d_sig[idx].contiguous()

        alone = g.project_wide(d_sig[P:P + 1].contiguous(), d_w)
        for slot, count in ((0, K), (7, K), (31, K), (3, 5), (0, 5)):
            _same(g.project_wide(at(slot, count), d_w)[slot], alone[0], "slot %d of %d" % (slot, count))
        full = g.project_wide(d_sig[:K].contiguous(), d_w)
        _same(g.project_wide(d_sig[:K].contiguous(), d_w), full, "two calls")
        _same(full[P], alone[0], "plane %d among 32" % P)
        ones = torch.ones((h, width), dtype=torch.float32, device=ctx.device)
        unweighted = g.project_wide(d_sig[:K].contiguous())
        _same(g.project_wide(d_sig[:K].contiguous(), ones), unweighted, "weight None against a plane of ones")
        assert not g.project_wide(d_sig[:K].contiguous(), torch.zeros_like(ones)).any()
        scaled = g.project_wide((d_sig[:K] * 8.0).contiguous(), (d_w * 0.25).contiguous())
        _same(scaled, 2.0 * full, "planes x 8, weight / 4")
        forty = g.project_wide(d_sig, d_w)                                      # 32 + 8 planes: two calls of the C entry
        assert forty.shape == (40, g.info["m"])
        _same(forty[:K], full)
        _same(forty[K:], g.project_wide(d_sig[K:].contiguous(), d_w))
        g.close()


# ---- 4. the grid-strided loop: more tiles than the grid has waves ---------------------------------------------------------------------

@pytest.mark.parametrize("m,ld", [(8, 32), (40, 64), (100, 128), (200, 256)])
def test_project_wide_many_tiles_per_wave(m, ld):
    """509 x 515 = 8191 tiles of 32 pixels and one of 23, the graph of test_normal_equations_many_tiles_per_wave: every wave takes
    several tiles and flushes whole chains. Reference and bound in torch f64 on the device."""
    width, h = 509, 515
    n = width * h
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 1024                                          # more tiles than the largest grid (ld 32) has waves
        g = ctx.graph(ctx.to_device(glf.synth_image(width, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["p"], g.info["m"], g.info["ld"]) == (324, m, ld)
        d_sig = _dev(ctx, _planes32(h, width))
        d_w = _dev_weight(ctx, _weight("uniform", n), h, width)
        c = g.project_wide(d_sig, d_w)
        phi = g.phi[:, :m].double()
        ws = d_w.reshape(1, n).double() * d_sig.reshape(K, n).double()
        c64 = (ws @ phi).cpu().numpy()
        bound = _eps(n) * (ws.abs() @ phi.abs()).cpu().numpy()
        g.close()
    _assert_c(c, c64, bound, "509 x 515 ld %d" % ld)


# ---- 5. after a change of basis ---------------------------------------------------------------------------------------------------------

def test_project_wide_after_a_transform():
    width, h, _, _, m, _ = SHAPES["ld64"]
    m_new = 17
    rng = np.random.default_rng(5)
    sig = _planes32(h, width)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, "ld64")[0]
        g.transform(rng.uniform(-1.0, 1.0, (m, m_new)), rng.uniform(0.5, 1.0, m_new))
        assert g.info["m"] == m_new
        phi = _phi64(g)
        w = _weight("uniform", width * h)
        d_w, d_sig = _dev_weight(ctx, w, h, width), _dev(ctx, sig)
        got = {k: g.project_wide(d_sig[:k].contiguous(), d_w) for k in (K, 5)}
        g.close()
    assert phi.shape[1] == m_new
    s = sig.reshape(K, -1).astype(np.float64)
    for k, c in got.items():
        assert c.shape == (k, m_new)
        c64, bound = _want(phi, w, s[:k])
        _assert_c(c, c64, bound, "after a transform to m = 17, nplanes %d" % k)


# ---- 6. agreement with the existing calls -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld32", "ld128"])
def test_project_wide_agrees_with_project_and_normal_equations(shape):
    width, h = SHAPES[shape][:2]
    n = width * h
    sig = _planes32(h, width)[[0, 1, 2, 3]]
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi = _phi64(g)
        w = _weight("uniform", n)
        d_w, d_sig = _dev_weight(ctx, w, h, width), _dev(ctx, sig)
        wide, old = g.project_wide(d_sig), g.project(d_sig)
        wide_w, b = g.project_wide(d_sig, d_w), g.normal_equations(d_w, d_sig)[1]
        g.close()
    s = sig.reshape(4, -1).astype(np.float64)
    for what, got, ref, wt in (("project", wide, old, None), ("normal_equations' b", wide_w, b, w)):
        mag = np.abs(s if wt is None else wt.astype(np.float64)[None, :] * s) @ np.abs(phi)
        bound = (_eps(n) + n * 2.0 ** -51) * mag                                 # the wide bound plus the f64 call's own
        err = np.abs(got - ref)
        print("%s against %s: max diff / bound %.3f" % (shape, what, float((err / np.maximum(bound, 1e-300)).max())))
        assert np.all(err <= bound), what


# ---- 7. end to end: apply and fit beyond four planes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("nplanes,nresp,shape", [(8, 3, "ld64"), (12, 4, "ld128")])
def test_apply_beyond_four_planes(nplanes, nresp, shape):
    width, h, _, _, m, ld = SHAPES[shape]
    sig = _planes32(h, width)[:nplanes]
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi, lam = _phi64(g), g.eigenvalues.copy()
        d_sig = _dev(ctx, sig)
        weights = np.stack([0.5 * lam, 1.0 - lam, -(lam + 5.0), 3.0 * lam])[:nresp]
        ident = np.array([1.0, 0.0, 1.0, 1.0], dtype=np.float32)[:nresp]
        out = g.apply(d_sig, weights, ident).cpu().numpy()
        c = g.project_wide(d_sig)                                                # (the call apply made: the same bits)
        g.close()
    assert out.shape == (nresp, nplanes, h, width) and np.isfinite(out).all()
    s = sig.reshape(nplanes, -1).astype(np.float64)
    c64, cb = _want(phi, None, s)
    worst = 0.0
    for r in range(nresp):
        for k in range(nplanes):
            sb = _synth_want(phi, ld, weights[r] * c[k], ident[r], k, s)[1]
            want = float(ident[r]) * s[k] + phi @ (weights[r] * c64[k])
            bound = np.abs(phi) @ (np.abs(weights[r]) * cb[k]) + sb
            err = np.abs(out[r, k].reshape(-1).astype(np.float64) - want)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (r, k)
    print("apply %d planes x %d responses at %s: max |out - want| / bound %.3f" % (nplanes, nresp, shape, worst))


def test_apply_keeps_its_route_up_to_four_planes():
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld64")
        lam = g.eigenvalues
        two = d_sig[1:3].contiguous()
        weights = np.stack([0.5 * lam, 1.0 - lam, -(lam + 5.0)])
        ident = np.array([1.0, 0.0, 1.0], dtype=np.float32)
        c = g.project(two)
        a = (weights[:, None, :] * c[None, :, :]).reshape(6, -1)
        want = g.synthesize(a, np.repeat(ident, 2), np.tile(np.arange(2, dtype=np.int32), 3), two).cpu().numpy()
        for got in (g.apply(two, weights, ident), g.apply(two, weights, ident, wide=None)):
            _same(got.cpu().numpy().reshape(6, -1), want.reshape(6, -1))
        forced = g.apply(two, weights, ident, wide=True).cpu().numpy()           # the wide projection on request: close, not the same route
        assert forced.shape == (3, 2, SHAPES["ld64"][1], SHAPES["ld64"][0]) and np.isfinite(forced).all()
        g.close()


@pytest.mark.parametrize("shape", ["ld32", "ld256"])
def test_fit_beyond_four_planes_against_fp64(shape):
    """Graph.fit with 8 planes under a 30 % mask: G from normal_equations, b from project_wide. The tolerance is the perturbation bound
    of test_fit_against_fp64 with b's bound replaced by the wide one."""
    width, h, _, _, m, ld = SHAPES[shape]
    n = width * h
    sig = _planes32(h, width)[:8]
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi, lam = _phi64(g), g.eigenvalues.copy()
        w = _weight("mask", n)
        d_w, d_sig = _dev_weight(ctx, w, h, width), _dev(ctx, sig)
        got = g.fit(d_sig, d_w, smooth=SMOOTH, ridge=RIDGE)
        G, b = g.normal_equations(d_w)[0], g.project_wide(d_sig, d_w)            # the calls fit made: the same bits
        assert tuple(got.shape) == (8, h, width) and bool(torch.isfinite(got).all())
        got = got.cpu().numpy().reshape(8, n)
        g.close()
    s = sig.reshape(8, -1).astype(np.float64)
    a_got = glf.fit_coeffs(G, b, (RIDGE + SMOOTH * lam) * np.trace(G) / m)
    G64, S, b64, _ = _reference(phi, w, s)
    bw = _want(phi, w, s)[1]
    r = (RIDGE + SMOOTH * lam) * np.trace(G64) / m
    a64 = np.linalg.solve(G64 + np.diag(r), b64.T).T
    rownorm = np.linalg.norm(phi, axis=1)
    for k in range(8):
        cb = _coeff_bound(G64, S, lam, r, a64[k], bw[k])
        ce = float(np.linalg.norm(a_got[k] - a64[k]))
        print("%s plane %d: ||a - a64|| %.3e <= %.3e" % (shape, k, ce, cb))
        assert ce <= cb, (shape, k)
        sb = _synth_want(phi, ld, a_got[k], 0.0, -1, s)[1]
        err = np.abs(got[k].astype(np.float64) - phi @ a64[k])
        bound = sb + rownorm * cb
        print("%s plane %d: max |fit - Phi64 a64| / bound %.3f" % (shape, k, float((err / np.maximum(bound, 1e-300)).max())))
        assert np.all(err <= bound), (shape, k)


# ---- 8. the work buffers on a debug pool ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld32", "ld256"])
def test_project_wide_on_a_debug_pool(monkeypatch, shape):
    width, h = SHAPES[shape][:2]
    sig = _planes32(h, width)
    w = _weight("uniform", width * h)
    monkeypatch.delenv("GLF_POOL_DEBUG", raising=False)
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        phi_normal = g.phi.cpu().numpy()
        normal = g.project_wide(_dev(ctx, sig), _dev_weight(ctx, w, h, width))
        g.close()
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, shape)[0]
        _same(g.phi.cpu().numpy(), phi_normal, "Phi on the two pools")
        d_sig, d_w = _dev(ctx, sig), _dev_weight(ctx, w, h, width)
        c = g.project_wide(d_sig, d_w)
        ctx.image_processing(ctx.to_device(glf.synth_image(96, 80, seed=4)), glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.1))
        c2 = g.project_wide(d_sig, d_w)
        _same(c, normal, "debug pool against the normal pool")
        _same(c2, c)
        assert np.isfinite(c).all()
        assert ctx.debug_violations() == 0
        g.close()
        assert ctx.debug_violations() == 0


# ---- 9. refusals on a live handle -------------------------------------------------------------------------------------------------------

def test_project_wide_refusals_on_a_live_handle():
    lib = glf._lib
    width, h = SHAPES["ld32"][:2]
    with glf.Context(0) as ctx:
        g = _grey_graph(ctx, "ld32")[0]
        m = g.info["m"]
        d_sig = _dev(ctx, _planes32(h, width, 34))
        d_w = _dev_weight(ctx, _weight("uniform", width * h), h, width)
        first = g.project_wide(d_sig[:K].contiguous(), d_w)
        fill = np.full((34, m), 12345.0)
        W, P = C.c_void_p(d_w.data_ptr()), C.c_void_p(d_sig.data_ptr())
        for nplanes, planes, null_c in ((0, P, False), (33, P, False), (-1, P, False), (3, None, False), (K, None, False), (3, P, True)):
            hc = fill.copy()
            rc = lib.glf_graph_project_wide(g._g, W, C.c_int(nplanes), planes, None if null_c else glf._ptr(hc))
            assert rc == glf.ERR_INVALID, (nplanes, planes is None, null_c)
            np.testing.assert_array_equal(hc, fill)
        with pytest.raises(ValueError):
            g.project_wide(d_sig[:, :-1].contiguous())
        with pytest.raises(ValueError):
            g.project_wide(d_sig[:3].contiguous(), d_w[:-1].contiguous())
        with pytest.raises(AssertionError):
            g.project_wide(d_sig[:3].double())
        _same(g.project_wide(d_sig[:K].contiguous(), d_w), first)                 # nothing faulted: the next valid call gives the same bits
        g.close()
