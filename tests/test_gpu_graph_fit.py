"""The weighted least-squares fit on a graph handle: glf_graph_normal_equations (k_graph_normal: G = Phi^T diag(w) Phi on
v_mfma_f32_32x32x2_f32 in f32 chains of C = glf.GRAPH_NORMAL_CHAIN pixel terms added into f64, b = Phi^T diag(w) s in f64), the host
solve glf_fit_coeffs and Graph.fit on top of them.

Shapes: those of tests/test_gpu_graph.py. 61 x 47 = 2867 pixels is a multiple neither of 32 nor of any C <= 256, so the last staged
tile and the last chain are partial, at ld 32 / 64 / 128 / 256 (one tile; the three tiles of one superblock pair; diagonal and
off-diagonal pairs, Phi read 2 and 4 times); `tiny` is 160 pixels: 5 tiles, fewer than one chain holds and fewer than the waves of two
workgroups. 509 x 515 has more tiles than the largest grid has waves, so every wave runs its tile loop and flushes whole chains.

Bounds, from the reference alone. With S = sum_px |w phi_i phi_j|:
  |G - G64| <= (C + 3) 2^-24 S     the rounding of w phi, a C-term f32 chain, the f64 tail
  |b - b64| <= N 2^-51 sum_px |w s phi_j|     the f64 summation bound of both sides; the products are exact in f64
The fit's coefficients: the standard perturbation bound of a linear system, see _coeff_bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _bits, _grey_graph, _phi64, _synth_want  # noqa: E402
from test_gpu_pix_signals import _test_planes  # noqa: E402

C = glf.C
CHAIN = glf.GRAPH_NORMAL_CHAIN
EPS_G = (CHAIN + 3) * 2.0 ** -24
EPS_GRAM = (64 + 3) * 2.0 ** -24           # k_phi_gram: chains of 64
WEIGHTS = ("none", "mask", "uniform", "zeros", "tail")
MAX_GRID_WAVES = 4 * 1024                  # the most waves a k_graph_normal grid has along the pixels (ld 32)


def _weight(kind, n):
    """The weight planes, float32 [n] (None: no plane): a 0/1 mask with 30 % ones, uniform in [0, 3), all zeros, zero everywhere
    except the last 19 pixels (the partial tile of the 32-pixel staging at 2867 pixels)."""
    rng = np.random.default_rng(17)
    if kind == "none":
        return None
    if kind == "mask":
        return (rng.uniform(size=n) < 0.3).astype(np.float32)
    if kind == "uniform":
        return rng.uniform(0.0, 3.0, n).astype(np.float32)
    w = np.zeros(n, dtype=np.float32)
    if kind == "tail":
        w[-19:] = rng.uniform(0.5, 2.0, 19).astype(np.float32)
    return w


def _same(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _dev_weight(ctx, w, h, width):
    return None if w is None else torch.from_numpy(w.reshape(h, width)).to(ctx.device)


def _reference(phi, w, s):
    """(G64, S, b64 [k, m], the bound of b [k, m]) in numpy f64; w None = 1."""
    wv = np.ones(phi.shape[0]) if w is None else w.astype(np.float64)
    G64 = phi.T @ (wv[:, None] * phi)
    S = np.abs(phi).T @ (np.abs(wv)[:, None] * np.abs(phi))
    ws = wv[None, :] * s
    return G64, S, ws @ phi, phi.shape[0] * 2.0 ** -51 * (np.abs(ws) @ np.abs(phi))


def _assert_normal(G, b, G64, S, b64, bb, what):
    eg = np.abs(G - G64)
    print("%s: max |G - G64| / bound %.3f, max |b - b64| / bound %.3e" %
          (what, float((eg / np.maximum(EPS_G * S, 1e-300)).max()), float((np.abs(b - b64) / np.maximum(bb, 1e-300)).max()) if b.size else 0.0))
    assert np.all(eg <= EPS_G * S), what
    assert np.all(np.abs(b - b64) <= bb), what
    np.testing.assert_array_equal(G, G.T, err_msg=what)


# ---- 1. the normal equations against fp64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_normal_equations_against_fp64(shape, kind):
    width, h = SHAPES[shape][:2]
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        phi = _phi64(g)
        w = _weight(kind, phi.shape[0])
        four = torch.cat([d_sig, d_sig[:1]]).contiguous()
        G, b = g.normal_equations(_dev_weight(ctx, w, h, width), four)
        gram = g.gram() if kind == "none" else None
        g.close()
    m = phi.shape[1]
    assert G.shape == (m, m) and b.shape == (4, m)
    s4 = np.concatenate([s, s[:1]])
    G64, S, b64, bb = _reference(phi, w, s4)
    _assert_normal(G, b, G64, S, b64, bb, "%s %s" % (shape, kind))
    np.testing.assert_array_equal(b[3], b[0])                                    # (the same plane twice: the same bits)
    if kind == "zeros":
        assert not G.any() and not b.any()
    if kind == "none":                                                           # the unweighted Gram matrix of the handle
        assert np.all(np.abs(G - gram) <= (EPS_G + EPS_GRAM) * S)


# ---- 2. independence and repeatability ------------------------------------------------------------------------------------------------

def test_G_and_b_do_not_depend_on_the_planes_beside_them():
    width, h = SHAPES["ld64"][:2]
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld64")
        w = _dev_weight(ctx, _weight("uniform", width * h), h, width)
        four = torch.cat([d_sig, d_sig[2:3]]).contiguous()
        G0, b0 = g.normal_equations(w)
        G1, b1 = g.normal_equations(w, d_sig[2:3].contiguous())
        G3, b3 = g.normal_equations(w, d_sig)
        G4, b4 = g.normal_equations(w, four)
        G4b, b4b = g.normal_equations(w, four)
        rep = g.normal_equations(w, torch.cat([d_sig[2:3]] * 4).contiguous())[1]
        g.close()
    assert b0.shape == (0, G0.shape[0])
    for G in (G1, G3, G4, G4b):
        _same(G, G0)
    _same(b4, b4b)
    _same(b3, b4[:3])
    for row in (b3[2], b4[2], b4[3], rep[0], rep[1], rep[2], rep[3]):            # plane 2: alone, among three, among four, repeated
        _same(row, b1[0])


# ---- 3. the grid-strided loop: more tiles than the grid has waves ------------------------------------------------------------------

@pytest.mark.parametrize("m,ld", [(8, 32), (40, 64), (100, 128), (200, 256)])
def test_normal_equations_many_tiles_per_wave(m, ld):
    """509 x 515 = 8191 tiles of 32 pixels and one of 23: every wave takes several tiles, whole chains are flushed into f64 and the
    next tile's loads fly under the MFMAs. Reference and bounds in torch f64 on the device."""
    width, h = 509, 515
    n = width * h
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"] and (n + 31) // 32 > MAX_GRID_WAVES
        assert glf.Sampling(width, h, 300).size == 324
        g = ctx.graph(ctx.to_device(glf.synth_image(width, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["p"], g.info["m"], g.info["ld"]) == (324, m, ld)
        sig = _test_planes(h, width)
        four = torch.from_numpy(np.concatenate([sig, sig[:1]])).to(ctx.device)
        w = _dev_weight(ctx, _weight("uniform", n), h, width)
        G, b = g.normal_equations(w, four)
        phi = g.phi[:, :m].double()
        wd = w.reshape(n).double()
        ws = wd[None, :] * four.reshape(4, n).double()
        G64 = (phi.T @ (wd[:, None] * phi)).cpu().numpy()
        S = (phi.abs().T @ (wd[:, None] * phi.abs())).cpu().numpy()
        b64 = (ws @ phi).cpu().numpy()
        bb = n * 2.0 ** -51 * (ws.abs() @ phi.abs()).cpu().numpy()
        g.close()
    _assert_normal(G, b, G64, S, b64, bb, "509 x 515 ld %d" % ld)


# ---- 4. the fit end to end ------------------------------------------------------------------------------------------------------------

SMOOTH, RIDGE = 0.1, 0.1


def _coeff_bound(G64, S, lam, r, a64, eb):
    """||a - a64||_2 <= kappa (||Eb|| + ||EG||_F ||a64||) / (1 - kappa ||EG||_F), kappa = ||(G64 + diag r)^-1||_2, EG = EPS_G S, plus
    the penalty's own dependence on trace(G) in the numerator. The condition kappa ||EG||_F <= 0.5 holds for any Phi:
    S_ij <= sqrt(G_ii G_jj) gives ||S||_F <= trace(G), and kappa <= m / (RIDGE trace(G)), so the product is at most
    EPS_G m / RIDGE <= 0.031 at C = 256, m = 200."""
    m = lam.size
    kappa = 1.0 / float(np.linalg.eigvalsh(G64 + np.diag(r)).min())
    eg = EPS_G * float(np.linalg.norm(S))
    assert kappa * eg <= 0.5, (kappa, eg)
    na = float(np.linalg.norm(a64))
    pen = EPS_G * (RIDGE + SMOOTH * float(lam.max())) * float(np.trace(S)) / m * kappa * na
    return (kappa * (float(np.linalg.norm(eb)) + eg * na) + pen) / (1.0 - kappa * eg)


@pytest.mark.parametrize("shape", ["ld32", "ld64", "ld256"])
def test_fit_against_fp64(shape):
    width, h, _, _, m, ld = SHAPES[shape]
    n = width * h
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        phi, lam = _phi64(g), g.eigenvalues.copy()
        w = _weight("mask", n)
        d_w = _dev_weight(ctx, w, h, width)
        got = g.fit(d_sig, d_w, smooth=SMOOTH, ridge=RIDGE)
        G, b = g.normal_equations(d_w, d_sig)                                     # the same call fit made: the same bits
        a0 = np.ones(m)                                                           # every column alike: the plane is led by Phi's large columns
        hole = (phi @ a0).astype(np.float32)
        filled = g.fit(torch.from_numpy(hole.reshape(1, h, width)).to(ctx.device), d_w, smooth=SMOOTH, ridge=RIDGE)
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(filled).all())
        got, filled = got.cpu().numpy().reshape(3, n), filled.cpu().numpy().reshape(n)
        g.close()
    a_got = glf.fit_coeffs(G, b, (RIDGE + SMOOTH * lam) * np.trace(G) / m)
    G64, S, b64, bb = _reference(phi, w, s)
    r = (RIDGE + SMOOTH * lam) * np.trace(G64) / m
    a64 = np.linalg.solve(G64 + np.diag(r), b64.T).T
    rownorm = np.linalg.norm(phi, axis=1)
    for k in range(3):
        cb = _coeff_bound(G64, S, lam, r, a64[k], bb[k])
        ce = float(np.linalg.norm(a_got[k] - a64[k]))
        print("%s plane %d: ||a - a64|| %.3e <= %.3e (||a64|| %.3e)" % (shape, k, ce, cb, float(np.linalg.norm(a64[k]))))
        assert ce <= cb, (shape, k)
        _, sb = _synth_want(phi, ld, a_got[k], 0.0, -1, s)
        err = np.abs(got[k].astype(np.float64) - phi @ a64[k])
        bound = sb + rownorm * cb
        print("%s plane %d: max |fit - Phi64 a64| / bound %.3f" % (shape, k, float((err / np.maximum(bound, 1e-300)).max())))
        assert np.all(err <= bound), (shape, k)
    # hole filling: where w = 0, the fit of a plane in the span of Phi is closer to the plane than the zero image is
    masked = w == 0
    d_fit = float(np.linalg.norm(filled[masked].astype(np.float64) - hole[masked]))
    d_zero = float(np.linalg.norm(hole[masked].astype(np.float64)))
    print("%s hole filling on %d masked pixels: |fit - plane| %.3e, |plane| %.3e" % (shape, int(masked.sum()), d_fit, d_zero))
    assert d_fit < d_zero


# ---- 5. the work buffers on a debug pool ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld32", "ld256"])
def test_normal_equations_on_a_debug_pool(monkeypatch, shape):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    width, h = SHAPES[shape][:2]
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        w = _dev_weight(ctx, _weight("uniform", width * h), h, width)
        four = torch.cat([d_sig, d_sig[:1]]).contiguous()
        G, b = g.normal_equations(w, four)
        ctx.image_processing(ctx.to_device(glf.synth_image(96, 80, seed=4)), glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.1))
        G2, b2 = g.normal_equations(w, four)
        _same(G2, G)
        _same(b2, b)
        assert np.isfinite(G).all() and np.isfinite(b).all()
        assert ctx.debug_violations() == 0
        g.close()
        assert ctx.debug_violations() == 0


# ---- 6. refusals on a live handle -----------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_handle():
    lib = glf._lib
    width, h = SHAPES["ld32"][:2]
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld32")
        m = g.info["m"]
        w = _dev_weight(ctx, _weight("uniform", width * h), h, width)
        first = g.normal_equations(w, d_sig)
        Gb, bb = np.zeros((m, m)), np.zeros((5, m))
        W, P = C.c_void_p(w.data_ptr()), C.c_void_p(d_sig.data_ptr())
        for nplanes, planes, hG, hb in ((-1, P, Gb, bb), (5, P, Gb, bb), (1, None, Gb, bb), (3, None, Gb, bb), (1, P, Gb, None), (3, P, Gb, None),
                                        (0, None, None, None), (3, P, None, bb)):
            rc = lib.glf_graph_normal_equations(g._g, W, C.c_int(nplanes), planes, glf._ptr(hG), glf._ptr(hb))
            assert rc == glf.ERR_INVALID, (nplanes, planes is None, hG is None, hb is None)
        with pytest.raises(ValueError):
            g.normal_equations(w[:-1].contiguous())
        with pytest.raises(ValueError):
            g.normal_equations(w.reshape(1, h, width))
        with pytest.raises(AssertionError):
            g.normal_equations(w.double())
        with pytest.raises(AssertionError):
            g.fit(d_sig, w.double())
        again = g.normal_equations(w, d_sig)
        _same(again[0], first[0])
        _same(again[1], first[1])
        g.close()
