"""Per-pixel quadratic forms on a graph handle (glf_graph_quadform / Graph.quadform, .leverage, .fit_loo, .distance, .rows):
q_k(px) = |R^T phi_px - t_k|^2 in one pass over Phi (k_graph_quadform: k_graph_synthesize's contraction, then an f32 epilogue that
squares and sums in registers).

Shapes: those of tests/test_gpu_graph.py -- 61 x 47 = 2867 pixels (89 whole tiles and one of 19 pixels) at ld 32 / 64 / 128 / 256,
and `tiny` (160 pixels); 509 x 515 in one test, so that waves run their tile loop more than once.

The bound (test 2, DESIGN.md "Per-pixel quadratic forms"), from the reference alone: with y64 = Phi fl32(R) in f64 on the handle's own
Phi, x64_c = y64_c - fl32(t_c), delta_c = (ld + 4) 2^-24 (|Phi| |R_c|) (the committed synthesize bound, _synth_want) and
eps_c = delta_c + 2^-24 (|x64_c| + delta_c):
    |q - q64| <= sum_c (2 |x64_c| eps_c + eps_c^2) + (r + 1) 2^-24 sum_c (|x64_c| + eps_c)^2.
The first sum is the error of the squares of x = x64 +- eps, the second the r fmaf roundings, the half-wave addition (and, through
the grouped Python call, the accumulating additions: fewer than r + 1 roundings on every path) of a sum of r non-negative terms.

Leave-one-out budget (test 6): (|e - e64| + |e64| w |v - v64| / (1 - h64)) / (1 - h64), the first term from the synthesize bound, the
second from the bound above. The f64 refit takes the library's own G and b (its normal equations, f32 chains added into f64) and
downdates them by the pixel, G - w phi phi^T and b - w phi s: setting one weight to zero changes nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_graph import SHAPES, _dev, _grey_graph, _opt, _phi64  # noqa: E402
from test_gpu_graph_cluster import TWO_TONE_SEED, _two_tone  # noqa: E402
from test_gpu_graph_compact import LD_SHAPES, _pair, _same  # noqa: E402

U = 2.0 ** -24
ALL_SHAPES = LD_SHAPES + ["tiny"]
STORAGES = ["f32", "compact"]
SENTINEL = -77.0


def _fl32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _handle(ctx, shape, storage):
    """(graph, its own Phi [N, m] in f64: Q on a compact handle)."""
    g, _, _ = _grey_graph(ctx, shape)
    if storage == "compact":
        g.compact()
        return g, g.dequantize().cpu().numpy()[:, :g.info["m"]].astype(np.float64)
    return g, _phi64(g)


def _want(phi, ld, R, t=None, exact=False):
    """(q64 [ncent, N], bound [ncent, N]) by the module text; t None: one centre at the origin. exact: y64 = Phi R with R as given
    in f64 instead of fl32(R) -- what _synth_want compares against: the 4 units of slack in delta cover the fl32 of a coefficient."""
    R32 = _fl32(R)
    r = R32.shape[1]
    t32 = np.zeros((1, r)) if t is None else _fl32(np.atleast_2d(t))
    y = phi @ (np.asarray(R, dtype=np.float64) if exact else R32)
    delta = (ld + 4) * U * (np.abs(phi) @ np.abs(R32))
    q, bound = [], []
    for k in range(t32.shape[0]):
        x = np.abs(y - t32[k])
        eps = delta + U * (x + delta)
        q.append((x * x).sum(axis=1))
        bound.append((2.0 * x * eps + eps * eps).sum(axis=1) + (r + 1) * U * ((x + eps) ** 2).sum(axis=1))
    return np.stack(q), np.stack(bound)


def _assert_within(got, want, bound, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    err = np.abs(got.reshape(want.shape).astype(np.float64) - want)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: max |q - q64| / bound %.3f (max err %.3e)" % (what, frac, float(err.max())))
    assert np.isfinite(got).all() and np.all(err <= bound), (what, frac)
    return frac


def _metric(phi, m, r, rng):
    """R [m, r] at the scale that makes the columns of Phi R of order one."""
    return rng.normal(size=(m, r)) / (np.sqrt(m) * max(float(np.abs(phi).max()), 1e-30))


def _centres(phi, R, ncent, rng):
    """Centres among the values of Phi R: the first is a pixel's own row (the cancellation case), the rest perturbed rows."""
    y = phi @ _fl32(R)
    rows = rng.integers(0, phi.shape[0], ncent)
    t = y[rows] + rng.normal(size=(ncent, R.shape[1])) * y.std()
    t[0] = y[rows[0]]
    return t


# ---- 1. bit for bit against glf_graph_synthesize -------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", LD_SHAPES)
def test_single_column_is_the_square_of_synthesize(shape, storage):
    rng = np.random.default_rng(SHAPES[shape][5])
    with glf.Context(0) as ctx:
        g, phi = _handle(ctx, shape, storage)
        m = g.info["m"]
        for c in (0, 5, 31, 32, 63):
            for r in sorted({c + 1, 32 if c < 32 else 64, 64}):
                R = np.zeros((m, r))
                R[:, c] = _metric(phi, m, 1, rng)[:, 0]
                t = np.zeros((1, r))
                t[0, c] = float(rng.normal())
                y = g.synthesize(R[:, c][None])[0]
                x = y - float(np.float32(t[0, c]))                                   # torch f32: one subtraction
                want = (x.double() ** 2).float()                                    # the exact square, rounded once
                _same(g.quadform(R, t)[0], want, "%s %s column %d of %d" % (shape, storage, c, r))
                _same(g.quadform(R)[0], (y.double() ** 2).float(), "%s %s column %d of %d, no centre" % (shape, storage, c, r))
        g.close()


# ---- 2. against fp64, every pixel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_quadform_against_fp64(shape, storage):
    ld = SHAPES[shape][5]
    rng = np.random.default_rng(7 + ld)
    worst = 0.0
    with glf.Context(0) as ctx:
        g, phi = _handle(ctx, shape, storage)
        m = g.info["m"]
        for r in (1, 8, 33, 64):
            R = _metric(phi, m, r, rng)
            for ncent in (1, 5, 32):
                t = _centres(phi, R, ncent, rng)
                got = g.quadform(R, t)
                assert tuple(got.shape) == (ncent, SHAPES[shape][1], SHAPES[shape][0]) and got.dtype == torch.float32
                q64, bound = _want(phi, ld, R, t)
                worst = max(worst, _assert_within(got, q64, bound, "%s %s r %d ncent %d" % (shape, storage, r, ncent)))
        g.close()
    print("%s %s: largest fraction of the bound %.3f" % (shape, storage, worst))


@pytest.mark.parametrize("storage", STORAGES)
def test_grouped_call_against_fp64(storage):
    """r = 200 columns in four launches (64 + 64 + 64 + 8, accumulating) and 33 centres in two groups, at ld 256."""
    rng = np.random.default_rng(200)
    with glf.Context(0) as ctx:
        g, phi = _handle(ctx, "ld256", storage)
        R = _metric(phi, g.info["m"], 200, rng)
        t = _centres(phi, R, 33, rng)
        got = g.quadform(R, t)
        q64, bound = _want(phi, 256, R, t)
        _assert_within(got, q64, bound, "ld256 %s r 200 ncent 33 (grouped)" % storage)
        _same(g.quadform(R, t[32:])[0], got[32], "a centre of the second group against alone")
        g.close()


def test_quadform_many_tiles_per_wave():
    """509 x 515 = 8192 tiles: more than the resident waves take at once, so every wave runs its tile loop more than once -- the
    prefetch under the MFMAs, fresh accumulators, the reuse of the wave's image. r = 64, 5 centres at ld 64, every pixel against
    fp64 (torch, on the device) at the bound of test 2."""
    w, h, m, ld, r, ncent = 509, 515, 40, 64, 64, 5
    n = w * h
    rng = np.random.default_rng(64)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["m"], g.info["ld"]) == (m, ld)
        phi = g.phi[:, :m].double()
        R = _metric(np.array([float(phi.abs().max())]), m, r, rng)
        R32 = torch.from_numpy(_fl32(R)).to(ctx.device)
        y = phi @ R32
        rows = rng.integers(0, n, ncent)
        t = y[torch.from_numpy(rows).to(ctx.device)].cpu().numpy() + rng.normal(size=(ncent, r)) * float(y.std())
        t[0] = y[int(rows[0])].cpu().numpy()
        got = g.quadform(R, t)
        delta = (ld + 4) * U * (phi.abs() @ R32.abs())
        ok, worst = True, 0.0
        for k in range(ncent):
            x = (y - torch.from_numpy(_fl32(t[k])).to(ctx.device)).abs()
            eps = delta + U * (x + delta)
            bound = (2.0 * x * eps + eps * eps).sum(1) + (r + 1) * U * ((x + eps) ** 2).sum(1)
            err = (got[k].reshape(n).double() - (x * x).sum(1)).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            ok = ok and bool(torch.all(err <= bound)) and bool(torch.isfinite(got[k]).all())
        one = g.quadform(R, t[3:4])
        _same(one[0], got[3], "centre 3 of 5 against alone")
        g.close()
    print("ld %d, %d tiles: max |q - q64| / bound %.3f" % (ld, (n + 31) // 32, worst))
    assert ok, worst


# ---- 3. invariances, bit for bit -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", LD_SHAPES)
def test_invariances(shape):
    w, h, ld = SHAPES[shape][0], SHAPES[shape][1], SHAPES[shape][5]
    n = w * h
    rng = np.random.default_rng(31 + ld)
    with glf.Context(0) as ctx:
        g, phi = _handle(ctx, shape, "f32")
        m = g.info["m"]
        for r in (8, 40):
            R = _metric(phi, m, r, rng)
            t = _centres(phi, R, 32, rng)
            full = g.quadform(R, t)
            _same(g.quadform(R, t), full, "two calls")
            for k in (0, 4, 31):                                                 # alone, and among fewer neighbours
                _same(g.quadform(R, t[k:k + 1])[0], full[k], "centre %d alone" % k)
            _same(g.quadform(R, t[:5]), full[:5], "5 of 32 centres")
            for pad in (32 - r if r < 32 else 3, 64 - r):                        # zero columns, within the block count and across it
                Rz, tz = np.hstack([R, np.zeros((m, pad))]), np.hstack([t, np.zeros((32, pad))])
                _same(g.quadform(Rz, tz), full, "%d zero columns appended to %d" % (pad, r))
            _same(g.quadform(2.0 * R, 2.0 * t), 4.0 * full, "R and t times 2")
            base = _dev(ctx, rng.normal(size=(32, h, w)).astype(np.float32) * float(full.mean()))
            acc = base.clone()
            assert g.quadform(R, t, out=acc, accumulate=True) is acc
            _same(acc, base + full, "accumulate against the plain result added in f32")
            # a padded output buffer: what lies past the last plane's N pixels stays
            buf = torch.full((5 * n + 64,), SENTINEL, dtype=torch.float32, device=ctx.device)
            Rc, tc = np.ascontiguousarray(R), np.ascontiguousarray(t[:5])
            torch.cuda.synchronize()
            rc = glf._lib.glf_graph_quadform(g._g, C.c_uint(r), glf._ptr(Rc), C.c_uint(5), glf._ptr(tc), 0, C.c_void_p(buf.data_ptr()))
            assert rc == glf.OK
            _same(buf[:5 * n].view(5, h, w), full[:5], "the raw call")
            assert bool(torch.all(buf[5 * n:] == SENTINEL))
        g.close()


@pytest.mark.parametrize("variant", ["plain", "scaled"])
@pytest.mark.parametrize("shape", LD_SHAPES)
def test_compact_equals_its_f32_twin(shape, variant):
    rng = np.random.default_rng(5)
    with glf.Context(0) as ctx:
        gc, gt, _, _, _, e = _pair(ctx, shape, variant)
        m = gc.info["m"]
        q = gt.phi.cpu().numpy()[:, :m].astype(np.float64)
        colmax = np.maximum(np.abs(q).max(axis=0), 1e-300)
        for r in (8, 64):
            R = rng.normal(size=(m, r)) / (np.sqrt(m) * colmax[:, None])         # every column of Q at order one, whatever its scale
            t = _centres(q, R, 5, rng)
            _same(gc.quadform(R, t), gt.quadform(R, t), "%s %s r %d" % (shape, variant, r))
        seeds = [0, 1234, q.shape[0] - 1]
        _same(gc.rows(seeds), gt.rows(seeds), "rows")
        _same(gc.rows(seeds), gt.phi.cpu().numpy()[seeds, :m], "rows against Q")
        _same(gc.distance(seeds), gt.distance(seeds), "%s %s distance" % (shape, variant))
        if variant == "scaled":
            assert len(set(e[:m].tolist())) >= 3
        gc.close()
        gt.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_output_untouched():
    lib = glf._lib
    with glf.Context(0) as ctx:
        g, phi = _handle(ctx, "ld64", "f32")
        m, n = g.info["m"], phi.shape[0]
        rng = np.random.default_rng(9)
        R, t = np.ascontiguousarray(_metric(phi, m, 64, rng)), rng.normal(size=(32, 64))
        out = torch.full((32, n), SENTINEL, dtype=torch.float32, device=ctx.device)
        torch.cuda.synchronize()
        O = C.c_void_p(out.data_ptr())
        with_nan, with_inf, too_big, t_nan, t_big = R.copy(), R.copy(), R.copy(), t.copy(), t.copy()
        with_nan[3, 7] = np.nan
        with_inf[m - 1, 63] = -np.inf
        too_big[0, 0] = 1e39                                                      # finite in f64, not in f32
        t_nan[31, 63] = np.nan
        t_big[0, 0] = -1e300
        cases = {"r = 0": (0, R, 1, t), "r = 65": (65, R, 1, t), "ncent = 0": (64, R, 0, t), "ncent = 33": (64, R, 33, t),
                 "R NULL": (64, None, 1, t), "NaN in R": (64, with_nan, 1, t), "Inf in R": (64, with_inf, 1, None),
                 "an R beyond f32": (64, too_big, 32, t), "NaN in t": (64, R, 32, t_nan), "a t beyond f32": (64, R, 1, t_big)}
        for what, (r, RR, ncent, tt) in cases.items():
            for accumulate in (0, 1):
                assert lib.glf_graph_quadform(g._g, C.c_uint(r), glf._ptr(RR), C.c_uint(ncent), glf._ptr(tt), accumulate, O) == glf.ERR_INVALID, what
        assert lib.glf_graph_quadform(g._g, C.c_uint(64), glf._ptr(R), C.c_uint(1), glf._ptr(t), 0, None) == glf.ERR_INVALID
        assert lib.glf_graph_quadform(None, C.c_uint(64), glf._ptr(R), C.c_uint(1), glf._ptr(t), 0, O) == glf.ERR_INVALID
        torch.cuda.synchronize()
        assert bool(torch.all(out == SENTINEL))
        # (a NaN in row 31 of t is not read by a call of one centre)
        assert lib.glf_graph_quadform(g._g, C.c_uint(64), glf._ptr(R), C.c_uint(1), glf._ptr(t_nan), 0, O) == glf.OK
        rows = np.full((3, m), SENTINEL, dtype=np.float32)
        px = np.array([0, n, 5], dtype=np.int64)
        for nrows, pp, rr in ((0, px, rows), (33, px, rows), (3, None, rows), (3, px, None), (3, px, rows), (2, np.array([-1, 0], dtype=np.int64), rows)):
            assert lib.glf_graph_rows(g._g, C.c_uint(nrows), glf._ptr(pp), glf._ptr(rr)) == glf.ERR_INVALID, nrows
        assert np.all(rows == SENTINEL)
        with pytest.raises(ValueError):
            g.quadform(np.zeros((m + 1, 3)))
        with pytest.raises(ValueError):
            g.quadform(R, np.zeros((2, 63)))
        with pytest.raises(ValueError):
            g.quadform(R, accumulate=True)
        with pytest.raises(glf.GlfError) as e:                                   # G_w with w = 0 and no penalty: not positive definite
            g.leverage(torch.zeros((SHAPES["ld64"][1], SHAPES["ld64"][0]), dtype=torch.float32, device=ctx.device))
        assert e.value.status == glf.ERR_INVALID
        # nothing faulted, and the next valid call succeeds
        q64, bound = _want(phi, 64, R, t[:2])
        _assert_within(g.quadform(R, t[:2]), q64, bound, "after the refusals")
        g.close()


# ---- 5. leverage ---------------------------------------------------------------------------------------------------------------------

def _mask(ctx, h, w, seed=17):
    """A 30 % mask: weight 0 on three pixels in ten, 1 elsewhere."""
    x = (np.random.default_rng(seed).uniform(size=(h, w)) >= 0.3).astype(np.float32)
    return _dev(ctx, x), x.reshape(-1).astype(np.float64)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_leverage(shape, storage):
    w, h, ld = SHAPES[shape][0], SHAPES[shape][1], SHAPES[shape][5]
    with glf.Context(0) as ctx:
        g, phi = _handle(ctx, shape, storage)
        m = g.info["m"]
        d_w, wv = _mask(ctx, h, w)
        for smooth, ridge in ((1.0, 1e-3), (0.0, 1e-2)):
            v = g.leverage(d_w, smooth=smooth, ridge=ridge)
            assert tuple(v.shape) == (h, w) and v.dtype == torch.float32
            G = g.normal_equations(d_w)[0]
            pen = (ridge + smooth * g.eigenvalues) * (np.trace(G) / m)
            assert np.all(pen > 0.0)
            M = G + np.diag(pen)
            R = glf.fit_factor(G, pen)
            want = np.einsum("ij,ij->i", phi, np.linalg.solve(M, phi.T).T)
            # the bound of test 2 on fit_factor's R, and the factor's own f64 error: tests/test_quad_host.py's 1e-12 cond
            q64, bound = _want(phi, ld, R, exact=True)
            cond = float(np.linalg.cond(M))
            assert np.all(np.abs(q64[0] - want) <= 1e-12 * cond * want)
            tol = bound[0] + 1e-12 * cond * want
            vv = v.cpu().numpy().reshape(-1).astype(np.float64)
            _assert_within(vv, want, tol, "%s %s leverage smooth %g ridge %g" % (shape, storage, smooth, ridge))
            # sum_px w v = trace(M^-1 G_w), G_w exact on the handle's Phi
            Gw = phi.T @ (wv[:, None] * phi)
            tr, got = float(np.trace(np.linalg.solve(M, Gw))), float((wv * vv).sum())
            print("%s %s: sum w v %.9g, trace %.9g, bound %.3e" % (shape, storage, got, tr, float((wv * tol).sum())))
            assert abs(got - tr) <= float((wv * tol).sum())
            hh = wv * vv
            assert np.all(vv >= 0.0) and np.all(hh < 1.0), float(hh.max())
        g.close()


# ---- 6. leave-one-out ----------------------------------------------------------------------------------------------------------------

def _loo_case(ctx, shape, storage):
    """(g, phi, weight device / numpy, planes device / numpy): a plane in the span of the first 4 columns plus noise, and a ramp."""
    w, h = SHAPES[shape][:2]
    g, phi = _handle(ctx, shape, storage)
    rng = np.random.default_rng(23)
    d_w, wv = _mask(ctx, h, w)
    span = (phi[:, :4] / np.abs(phi[:, :4]).max(axis=0)) @ rng.normal(size=4)
    s = np.stack([span + 0.1 * rng.normal(size=span.size), np.linspace(-1.0, 1.0, span.size)]).astype(np.float32)
    return g, phi, d_w, wv, _dev(ctx, s.reshape(2, h, w)), s.astype(np.float64)


def _loo64(phi, ld, G, b, pen, wv, s):
    """The f64 fit on the library's normal equations: (a [np, m], e64 [np, N], v64 [N], budget of e / (1 - w v) [np, N])."""
    M = G + np.diag(pen)
    a = np.linalg.solve(M, b.T).T
    e64 = s - a @ phi.T
    de = (ld + 4) * U * (np.abs(a) @ np.abs(phi).T)                               # the synthesize bound of z = Phi a
    R = glf.fit_factor(G, pen)
    v64, dv = _want(phi, ld, R, exact=True)
    h64 = wv * v64[0]
    budget = (de + np.abs(e64) * wv * dv[0] / (1.0 - h64)) / (1.0 - h64)
    return a, e64, v64[0], h64, budget


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ["tiny", "ld32"])
def test_leave_one_out_is_the_refit(shape, storage):
    ld = SHAPES[shape][5]
    with glf.Context(0) as ctx:
        g, phi, d_w, wv, d_s, s = _loo_case(ctx, shape, storage)
        m, n = g.info["m"], phi.shape[0]
        G, b = g.normal_equations(d_w, d_s)
        pen = (1e-3 + 1.0 * g.eigenvalues) * (np.trace(G) / m)
        z = g.fit(d_s, d_w, smooth=1.0, ridge=1e-3).cpu().numpy().reshape(2, n).astype(np.float64)
        v = g.leverage(d_w, smooth=1.0, ridge=1e-3).cpu().numpy().reshape(n).astype(np.float64)
        g.close()
    loo = (s - z) / (1.0 - wv * v)
    a, e64, v64, h64, budget = _loo64(phi, ld, G, b, pen, wv, s)
    live = np.flatnonzero(wv > 0)
    picks = live[np.linspace(0, live.size - 1, 12).astype(int)]
    M = G + np.diag(pen)
    for px in picks:
        f = phi[px]
        Mi = M - wv[px] * np.outer(f, f)                                         # that pixel's weight set to zero
        for k in range(2):
            ai = np.linalg.solve(Mi, b[k] - wv[px] * s[k, px] * f)
            refit = s[k, px] - f @ ai
            # the identity e64 / (1 - h64) = the refit holds in f64 to the solves' m 2^-53 cond ~ 1e-11: 1e-9 of the value covers it
            tol = budget[k, px] + 1e-9 * abs(refit)
            print("%s %s pixel %d plane %d: loo %.9g refit %.9g, |diff| / budget %.3f" % (shape, storage, px, k, loo[k, px], refit,
                                                                                       abs(loo[k, px] - refit) / tol))
            assert abs(loo[k, px] - refit) <= tol, (px, k)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ["tiny", "ld32"])
def test_fit_loo_scores_and_choice(shape, storage):
    ld = SHAPES[shape][5]
    smooths = (0.0, 1.0, 100.0)
    with glf.Context(0) as ctx:
        g, phi, d_w, wv, d_s, s = _loo_case(ctx, shape, storage)
        m = g.info["m"]
        G, b = g.normal_equations(d_w, d_s)
        scores, fit, best = g.fit_loo(d_s, d_w, smooths, ridge=1e-3)
        fits = [g.fit(d_s, d_w, smooth=sm, ridge=1e-3) for sm in smooths]
        lam = g.eigenvalues.copy()
        g.close()
    assert scores.shape == (3, 2)
    want = np.zeros((3, 2))
    for i, sm in enumerate(smooths):
        pen = (1e-3 + sm * lam) * (np.trace(G) / m)
        a, e64, v64, h64, budget = _loo64(phi, ld, G, b, pen, wv, s)
        loo64 = e64 / (1.0 - h64)
        want[i] = (wv * loo64 ** 2).sum(axis=1) / wv.sum()
        tol = (wv * (2.0 * np.abs(loo64) * budget + budget ** 2)).sum(axis=1) / wv.sum() + 1e-9 * want[i]
        print("%s %s smooth %g: scores %s, f64 %s, |diff| / budget %s" % (shape, storage, sm, scores[i], want[i], np.abs(scores[i] - want[i]) / tol))
        assert np.all(np.abs(scores[i] - want[i]) <= tol), (sm, scores[i], want[i])
    first = int(np.argmin(want.sum(axis=1)))
    assert best == first
    _same(fit, fits[first], "the fit of the candidate the f64 scores rank first")


# ---- 7. distance ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ["ld32", "ld64", "ld128", "tiny"])
def test_distance_from_seeds(shape, storage):
    w, h, ld = SHAPES[shape][0], SHAPES[shape][1], SHAPES[shape][5]
    n = w * h
    seeds = [0, n // 2 + 7, n - 1]                                               # the last one in the partial tile
    with glf.Context(0) as ctx:
        g, phi = _handle(ctx, shape, storage)
        m, lam = g.info["m"], g.eigenvalues.copy()
        for dim, resp in ((None, None), (max(m // 2, 1), np.exp(-3.0 * lam))):   # m = 100 at ld 128: two groups of columns
            d2 = g.distance(seeds, response=resp, dim=dim)
            assert tuple(d2.shape) == (3, h, w)
            dd = m if dim is None else dim
            g32 = _fl32(1.0 - lam if resp is None else resp)
            R = np.diag(g32)[:, :dd]
            t = g32[None, :dd] * phi[seeds, :dd]
            flat = d2.reshape(3, n).cpu().numpy()
            for i, px in enumerate(seeds):
                assert flat[i, px] == 0.0 and not np.signbit(flat[i, px]), (i, px, flat[i, px])
            q64, bound = _want(phi, ld, R, t)
            _assert_within(flat, q64, bound, "%s %s distance dim %d" % (shape, storage, dd))
        g.close()


def test_distance_separates_the_two_halves():
    """The two-tone image of the cluster tests, a seed in the left half, dim = m: the median D^2 over the left half against the
    median over the right half, in f64 on the handle's Phi and from the library."""
    w, h = SHAPES["ld32"][:2]
    seed = (h // 2) * w + w // 4
    left = (np.arange(w) < w // 2)[None].repeat(h, axis=0).reshape(-1)
    for storage in STORAGES:
        with glf.Context(0) as ctx:
            g = ctx.graph(ctx.to_device(_two_tone(TWO_TONE_SEED)), _opt("ld32"))
            if storage == "compact":
                g.compact()
                phi = g.dequantize().cpu().numpy()[:, :g.info["m"]].astype(np.float64)
            else:
                phi = _phi64(g)
            m = g.info["m"]
            d2 = g.distance([seed], dim=m).cpu().numpy().reshape(-1).astype(np.float64)
            g32 = _fl32(1.0 - g.eigenvalues)
            g.close()
        d64 = (((phi - phi[seed]) * g32) ** 2).sum(axis=1)
        med = [float(np.median(x[left])) for x in (d64, d2)] + [float(np.median(x[~left])) for x in (d64, d2)]
        print("%s: median D^2 left %.6e (f64) %.6e (library), right %.6e (f64) %.6e (library), ratio right / left %.2f" %
              (storage, med[0], med[1], med[2], med[3], med[3] / med[1]))
        assert med[0] < med[2], "the f64 distance on the handle's Phi does not order the halves"
        assert med[1] < med[3]
