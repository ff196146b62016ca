"""The robust fit on a graph handle: glf_graph_robust_step (k_graph_residual_weight: the residuals at the previous iterate on
k_graph_synthesize's MFMA shape and the IRLS weight w_eff = w u(q) as its epilogue, then glf_graph_normal_equations' own pass under
w_eff) and the driver glf_graph_fit_robust, under the Huber, Cauchy and Tukey losses.

Shapes: those of tests/test_gpu_graph.py -- 61 x 47 = 2867 pixels at ld 32 / 64 / 128 / 256 (a partial last tile, 1 / 1 / 2 / 4 staged
chunks per tile), `tiny` (160 pixels: fewer tiles than two workgroups have waves) -- and 509 x 515 (8192 tiles: more than any grid
has waves, so the grid-strided loop iterates and a lane sums several pixels).

What is pinned (include/glf.h) and checked bit for bit: the residual planes are planes - synthesize(a_prev) in one f32 subtraction;
G and b are normal_equations(weight_out, planes). Against f64:
  |u - u64(q64)| <= 2^-20, u = weight_out / w, q64 from the emitted residuals in f64: u <= 1, at most 4 f32 roundings in u and
  nplanes + 1 in q, which enter with |q du/dq| <= 1 for all three losses: < 12 x 2^-24.
  |loss - sum w rho64(q32)| <= 2^-44 sum |w rho|, q32 the pinned f32 arithmetic restated here (an f32 product, then fmaf emulated
  exactly in f64 with the double rounding repaired, see _fmaf_sq): rho is formed in f64 from (double) q32 on both sides, so what is
  left is the f64 summation (a lane's few pixels, 128 lanes, the workgroups) and a few ulp of the device's log1p.
  mass = the f64 sum of (double) weight_out to N 2^-52 relative.
The driver against an f64 IRLS on the handle's own Phi: see _irls_bound and test_driver_against_an_f64_irls."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_graph_robust_abi import DEFAULT_C, LOSSES, table64  # noqa: E402
from test_gpu_graph import SHAPES, _bits, _dev, _grey_graph, _phi64, _synth_want  # noqa: E402
from test_gpu_graph_fit import EPS_G, _dev_weight, _same, _weight  # noqa: E402
from test_gpu_pix_signals import _test_planes  # noqa: E402

C = glf.C
F32 = np.float32
BIG = (509, 515)


def _fmaf_sq(x32, q32):
    """fmaf(x, x, q) of float32 arrays, exactly: x * x is exact in f64 (24 x 24 bits); s = RN64(p + q) with its error e from TwoSum;
    RN32(s) is RN32(p + q) unless s sits exactly half way between two floats while e != 0 -- then the float on e's side is right."""
    p, q = x32.astype(np.float64) ** 2, q32.astype(np.float64)
    s = p + q
    bb = s - p
    e = (p - (s - bb)) + (q - bb)
    f = s.astype(F32)
    d = s - f.astype(np.float64)
    g = np.nextafter(f, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
    fix = (d != 0) & (np.abs(g.astype(np.float64) - s) == np.abs(d)) & (e != 0)
    return np.where(fix, np.where(e > 0, np.maximum(f, g), np.minimum(f, g)), f).astype(F32)


def test_fmaf_restatement_repairs_the_double_rounding():
    """x = 1 + 2^-12: x^2 = 1 + 2^-11 + 2^-24 is exactly half way between two floats, and a q of +/- 2^-60 is lost in the f64 sum."""
    x = np.array([1.0 + 2.0 ** -12], dtype=F32)                                  # x^2 = 1 + 2^-11 + 2^-24: a tie of f32 at 1 + 2^-11 (+ 2^-24)
    up = _fmaf_sq(x, np.array([2.0 ** -60], dtype=F32))                          # just above the tie: rounds up, though RN64 lands on the tie
    dn = _fmaf_sq(x, np.array([-2.0 ** -60], dtype=F32))                         # just below: rounds down
    tie = _fmaf_sq(x, np.array([0.0], dtype=F32))                                # the tie itself: to even
    base = F32(1.0 + 2.0 ** -11)
    assert dn[0] == base and up[0] == np.nextafter(base, F32(2.0)) and tie[0] in (base, np.nextafter(base, F32(2.0)))
    assert tie[0] == F32(np.float64(x[0]) ** 2)


def _q32(res32, sigma):
    """q of the pinned f32 arithmetic from the emitted residual planes [k, N] float32."""
    q = np.zeros(res32.shape[1], dtype=F32)
    for k in range(res32.shape[0]):
        q = _fmaf_sq(res32[k] * F32(1.0 / sigma[k]), q)
    return q


def _constant(loss, c):
    return DEFAULT_C[loss] if not c else c


def _big_graph(ctx, m):
    width, h = BIG
    g = ctx.graph(ctx.to_device(glf.synth_image(width, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
    sig = _test_planes(h, width)
    return g, _dev(ctx, sig)


def _start(g, d_planes, rng, rel=0.1):
    """(a_prev, sigma, the f64 residual planes on the device): the plain fit's coefficients perturbed by 10 %, and the scale of
    every plane from glf.robust_scale of its f64 residuals at a_prev."""
    G, b = g.normal_equations(None, d_planes)
    a = glf.fit_coeffs(G, b) * (1.0 + rel * rng.uniform(-1.0, 1.0, b.shape))
    k, n = d_planes.shape[0], g.phi.shape[0]
    res = d_planes.reshape(k, n).double() - torch.from_numpy(a).to(g.phi.device) @ g.phi[:, :g.info["m"]].double().T
    res = res.cpu().numpy()
    return a, np.array([glf.robust_scale(res[j]) for j in range(k)]), res


def _check_step(g, d_planes, w, a, sigma, loss, c, what):
    """One robust_step with both optional outputs against everything the header pins; -> its outputs."""
    k, h, width = d_planes.shape
    n = h * width
    d_w = None if w is None else torch.from_numpy(w.reshape(h, width)).to(d_planes.device)
    G, b, lo, ma, wout, rout = g.robust_step(d_planes, a, loss, c=c, sigma=sigma, weight=d_w, want_weights=True, want_residuals=True)
    # the residual planes: one f32 subtraction from synthesize's bits
    want_res = d_planes - g.synthesize(a)
    assert torch.equal(rout.view(torch.int32), want_res.view(torch.int32)), what
    res32, weff = rout.cpu().numpy().reshape(k, n), wout.cpu().numpy().reshape(n)
    wv = np.ones(n) if w is None else w.astype(np.float64)
    cc = _constant(loss, c)
    # the weights against f64 on the emitted residuals
    q64 = ((res32.astype(np.float64) / sigma[:, None]) ** 2).sum(axis=0)
    u64, _ = table64(loss, cc, q64)
    live = wv > 0
    eu = np.abs(weff[live].astype(np.float64) / wv[live] - u64[live])
    assert np.all(weff[~live] == 0), what
    # G and b: the weighted fit's own pass under the emitted weights
    G2, b2 = g.normal_equations(wout, d_planes)
    _same(G, G2)
    _same(b, b2)
    # loss and mass
    _, rho = table64(loss, cc, _q32(res32, sigma).astype(np.float64))
    terms = wv * rho
    want_loss, scale = math.fsum(terms), math.fsum(np.abs(terms))
    want_mass = math.fsum(weff.astype(np.float64))
    print("%s: max |u - u64| %.3e (2^-20 = %.3e), |loss - want| / sum|w rho| %.3e (2^-44 = %.3e), |mass - want| / mass %.3e" %
          (what, float(eu.max()) if eu.size else 0.0, 2.0 ** -20, abs(lo - want_loss) / max(scale, 1e-300), 2.0 ** -44,
           abs(ma - want_mass) / max(abs(want_mass), 1e-300)))
    assert np.all(eu <= 2.0 ** -20), what
    assert abs(lo - want_loss) <= 2.0 ** -44 * scale, what
    assert abs(ma - want_mass) <= n * 2.0 ** -52 * math.fsum(np.abs(weff.astype(np.float64))), what
    return G, b, lo, ma, wout, rout, u64


# ---- 1. the step against fp64 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_step_against_fp64(shape):
    """Every ld and `tiny`; every loss, 1 and 3 planes, no weight / a 0-1 mask / a weight on the last 19 pixels only. The input
    condition: at the constant's default, between 5 % and 95 % of the pixels have u < 1 under Huber (the residuals straddle c)."""
    rng = np.random.default_rng(23)
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        n = s.shape[1]
        for k in (1, 3):
            d_planes = d_sig[:k].contiguous()
            a, sigma, res64 = _start(g, d_planes, rng)
            q = ((res64 / sigma[:, None]) ** 2).sum(axis=0)
            frac = float((table64("huber", DEFAULT_C["huber"], q)[0] < 1.0).mean())
            print("%s, %d plane(s): sigma %s, u < 1 on %.1f %% of the pixels" % (shape, k, sigma, 100 * frac))
            assert 0.05 <= frac <= 0.95, (shape, k, frac)
            for loss in LOSSES:
                for kind in ("none", "mask", "tail"):
                    w = _weight(kind, n)
                    if kind == "tail" and n < 19:
                        continue
                    _check_step(g, d_planes, w, a, sigma, loss, None, "%s %s %d plane(s) w=%s" % (shape, loss, k, kind))
        g.close()


@pytest.mark.parametrize("m,ld", [(40, 64), (200, 256)])
def test_step_many_tiles_per_wave(m, ld):
    """509 x 515: every wave takes several tiles, the next tile's loads fly under the MFMAs and a lane sums several pixels."""
    rng = np.random.default_rng(29)
    with glf.Context(0) as ctx:
        g, d_sig = _big_graph(ctx, m)
        assert g.info["ld"] == ld and (g.phi.shape[0] + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        a, sigma, _ = _start(g, d_sig, rng)
        w = _weight("uniform", g.phi.shape[0])
        for loss, c in (("huber", None), ("cauchy", 1.0), ("tukey", 3.0)):
            _check_step(g, d_sig, w, a, sigma, loss, c, "509 x 515 ld %d %s" % (ld, loss))
        g.close()


# ---- 3. limits -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld32", "ld128"])
def test_limits_of_the_constant(shape):
    rng = np.random.default_rng(31)
    width, h = SHAPES[shape][:2]
    n = width * h
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        a, sigma, _ = _start(g, d_sig, rng)
        w = _weight("uniform", n)
        d_w = _dev_weight(ctx, w, h, width)
        # Huber with an enormous constant: every u is 1, the step is the weighted fit's normal equations
        G, b, lo, ma, wout, _ = g.robust_step(d_sig, a, "huber", c=1e18, sigma=sigma, weight=d_w, want_weights=True)
        G0, b0 = g.normal_equations(d_w, d_sig)
        assert torch.equal(wout.view(torch.int32), d_w.view(torch.int32))
        _same(G, G0)
        _same(b, b0)
        assert ma == math.fsum(w.astype(np.float64)) or abs(ma - math.fsum(w.astype(np.float64))) <= n * 2.0 ** -52 * ma
        # Tukey with a tiny constant: every pixel is rejected
        c = 1e-6
        G, b, lo, ma, wout, _ = g.robust_step(d_sig, a, "tukey", c=c, sigma=sigma, weight=d_w, want_weights=True)
        assert not wout.any() and not G.any() and not b.any() and ma == 0.0
        want = c * c / 6.0 * math.fsum(w.astype(np.float64))
        assert abs(lo - want) <= n * 2.0 ** -52 * want
        g.close()


# ---- 4. independence, repeatability, scaling -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld64", "ld256"])
def test_independence_repeatability_scaling(shape):
    rng = np.random.default_rng(37)
    width, h = SHAPES[shape][:2]
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        a, sigma, _ = _start(g, d_sig, rng)
        d_w = _dev_weight(ctx, _weight("uniform", width * h), h, width)
        for loss in LOSSES:
            full = g.robust_step(d_sig, a, loss, sigma=sigma, weight=d_w, want_weights=True, want_residuals=True)
            again = g.robust_step(d_sig, a, loss, sigma=sigma, weight=d_w, want_weights=True, want_residuals=True)
            bare = g.robust_step(d_sig, a, loss, sigma=sigma, weight=d_w)
            assert bare[4] is None and bare[5] is None
            for x, y, z in zip(full[:2], again[:2], bare[:2]):
                _same(x, y)
                _same(x, z)
            assert full[2:4] == again[2:4] == bare[2:4]
            assert torch.equal(full[4].view(torch.int32), again[4].view(torch.int32))
            assert torch.equal(full[5].view(torch.int32), again[5].view(torch.int32))
            # planes, coefficients and scales times two: the same q, so the same weights and G; b exactly doubled
            twice = g.robust_step((2.0 * d_sig).contiguous(), 2.0 * a, loss, sigma=2.0 * sigma, weight=d_w, want_weights=True, want_residuals=True)
            assert torch.equal(twice[4].view(torch.int32), full[4].view(torch.int32))
            assert torch.equal(twice[5].view(torch.int32), (2.0 * full[5]).view(torch.int32))
            _same(twice[0], full[0])
            _same(twice[1], 2.0 * full[1])
            assert twice[3] == full[3]
        # a plane's residual plane does not depend on the planes beside it
        three = g.robust_step(d_sig, a, "huber", sigma=sigma, want_residuals=True)[5]
        for k in range(3):
            one = g.robust_step(d_sig[k:k + 1].contiguous(), a[k:k + 1], "huber", sigma=sigma[k:k + 1], want_residuals=True)[5]
            assert torch.equal(one[0].view(torch.int32), three[k].view(torch.int32)), k
        g.close()


# ---- 5. the driver against an f64 IRLS -----------------------------------------------------------------------------------------------

RIDGE = 1e-4
NOISE = np.array([1.0, 0.1, 10.0])


def _ref_step(phi, s, wv, a, sigma, loss, c):
    """One IRLS step in f64 at the iterate a [k, m] -> (G, b [k, m], the data term sum w rho, w_eff)."""
    res = s - a @ phi.T
    q = ((res / sigma[:, None]) ** 2).sum(axis=0)
    u, rho = table64(loss, c, q)
    weff = wv * u
    return phi.T @ (weff[:, None] * phi), (weff[None, :] * s) @ phi, float((wv * rho).sum()), weff


def _objective(lo, pen, a, sigma):
    """The function the iteration decreases: the step solves (G + diag(pen)) a_k = b_k, the minimiser over a_k of
    sum w_eff res_k^2 + a_k^T diag(pen) a_k -- the penalty is in the units of the plain weighted fit, which the step is where every
    u = 1. The loss counts res_k in units of sigma_k and halves the square, so there the penalty is a_k^T diag(pen) a_k / (2 sigma_k^2):
    with rho concave in q and d rho / d q = u / 2, sum w [rho(q_0) + u_0 (q - q_0) / 2] + that penalty majorises the objective, touches
    it at the iterate and is minimised by the step."""
    return lo + float(((pen[None, :] * a ** 2).sum(axis=1) / (2.0 * sigma ** 2)).sum())


def _irls_bound(phi, s, wv, weff, pen, a_next):
    """||a - a64||_2 per plane for the solve after a step: test_gpu_graph_fit._coeff_bound's construction, the standard perturbation
    bound kappa (||Eb|| + ||EG||_F ||a64||) / (1 - kappa ||EG||_F) with kappa = ||(G64 + diag pen)^-1||_2, where the weight error
    2^-20 w of the step joins the rounding of the normal equations: EG = EPS_G S + 2^-20 S_w with S = |Phi|^T diag(|w_eff|) |Phi|
    and S_w the same under w itself, Eb = N 2^-51 sum |w_eff s phi| + 2^-20 sum |w s phi|. The penalty is the caller's vector on
    both sides and adds nothing. The bound needs kappa ||EG||_F <= 0.5, asserted on the numbers."""
    ap = np.abs(phi)
    S, Sw = ap.T @ (np.abs(weff)[:, None] * ap), ap.T @ (np.abs(wv)[:, None] * ap)
    G64 = phi.T @ (weff[:, None] * phi)
    kappa = 1.0 / float(np.linalg.eigvalsh(G64 + np.diag(pen)).min())
    eg = EPS_G * float(np.linalg.norm(S)) + 2.0 ** -20 * float(np.linalg.norm(Sw))
    assert kappa * eg <= 0.5, (kappa, eg)
    eb = phi.shape[0] * 2.0 ** -51 * (np.abs(weff[None, :] * s) @ ap) + 2.0 ** -20 * (np.abs(wv[None, :] * s) @ ap)
    return np.array([(kappa * (float(np.linalg.norm(eb[k])) + eg * float(np.linalg.norm(a_next[k])))) / (1.0 - kappa * eg)
                     for k in range(s.shape[0])])


def _ref_irls(phi, s, wv, pen, sigma, loss, c, iters):
    """The f64 IRLS from the plain weighted fit: iterates a_0 .. a_iters, the objective at each step's input, the weights of each step."""
    G0 = phi.T @ (wv[:, None] * phi)
    a = [np.linalg.solve(G0 + np.diag(pen), ((wv[None, :] * s) @ phi).T).T]
    obj, weffs = [], []
    for _ in range(iters):
        G, b, lo, weff = _ref_step(phi, s, wv, a[-1], sigma, loss, c)
        obj.append(_objective(lo, pen, a[-1], sigma))
        weffs.append(weff)
        a.append(np.linalg.solve(G + np.diag(pen), b.T).T)
    return a, obj, weffs


def _leading(g, cols=8):
    """The handle cut to its leading columns (ld stays): the later columns of these handles live on a few pixels each, and a fit
    whose coefficient hangs on one reweighted pixel converges slowly under any loss."""
    m = g.info["m"]
    if m > cols:
        g.transform(np.eye(m)[:, :cols], g.eigenvalues[:cols])
    return g


def _span_planes(phi, rng, frac, amp):
    """Three planes in the span of Phi with a standard deviation near 30 NOISE_k, Gaussian noise of standard deviation NOISE_k and a
    fraction frac of each plane's pixels moved by +/- amp NOISE_k -> float32 [3, N]."""
    n, m = phi.shape
    a_true = rng.normal(size=(3, m))
    a_true *= (30.0 * NOISE / (a_true @ phi.T).std(axis=1))[:, None]
    s = a_true @ phi.T + NOISE[:, None] * rng.normal(size=(3, n))
    for k in range(3):
        hit = rng.uniform(size=n) < frac
        s[k, hit] += amp * NOISE[k] * rng.choice([-1.0, 1.0], int(hit.sum()))
    return s.astype(F32)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape,ridge", [("ld32", RIDGE), ("ld32", 0.0), ("ld64", RIDGE), ("ld256", RIDGE)])
def test_driver_against_an_f64_irls(shape, ridge, loss):
    """Input: the handle's 8 leading columns (ld 32 as built; ld 64 and 256 cut to them by transform, so that the driver runs on the
    kernels of every staging width), three planes in their span under noise with 5 % of the pixels moved by 20 standard deviations
    of the noise, uniform weights in [0, 3), a ridge of 1e-4 trace(G_w) / m (and once none), the scales from the f64 plain fit's
    residuals, the default constants. The reference runs on its own from its own plain fit.
      * per iteration the library's coefficients lie within _irls_bound of the reference's, up to the first iteration whose
        reference iterate is within that bound of its predecessor (from there on both have converged and the bound says nothing);
      * the reference's objective (_objective) does not increase: majorise-minimise, in f64, 2^-40 of slack for its own rounding;
      * the library's objective[i + 1] <= objective[i] + 2 E, E = sum_px w c sum_k bound_k(px) / sigma_k + 2^-40 objective:
        the data term moves by at most |psi| <= c per unit of r, and the residual the library forms is within _synth_want's
        componentwise bound bound_k of the f64 one;
      * every loss reports converged within 20 iterations (measured: 3 to 9);
      * the driver is the loop a caller can write: normal_equations + fit_coeffs, then robust_step + fit_coeffs, bit for bit."""
    width, h, _, _, _, ld = SHAPES[shape]
    n = width * h
    rng = np.random.default_rng(41)
    c = DEFAULT_C[loss]
    with glf.Context(0) as ctx:
        g = _leading(_grey_graph(ctx, shape)[0])
        m = g.info["m"]
        assert (m, g.info["ld"]) == (8, ld)
        phi = _phi64(g)
        s32 = _span_planes(phi, rng, 0.05, 20.0)
        s = s32.astype(np.float64)
        d_planes = _dev(ctx, s32.reshape(3, h, width))
        w = _weight("uniform", n)
        d_w = _dev_weight(ctx, w, h, width)
        wv = w.astype(np.float64)
        pen = np.full(m, ridge * float(np.trace(phi.T @ (wv[:, None] * phi))) / m)
        lib_pen = pen if ridge else None
        res0 = s - _ref_irls(phi, s, wv, pen, None, None, None, 0)[0][0] @ phi.T
        sigma = np.array([glf.robust_scale(res0[k], wv) for k in range(3)])
        a64, obj64, weffs = _ref_irls(phi, s, wv, pen, sigma, loss, c, 20)
        fit, info = g.fit_robust(d_planes, d_w, loss=loss, sigma=sigma, penalty=lib_pen, return_info=True)
        its = info["iterations"]
        # the caller's loop
        G, b = g.normal_equations(d_w, d_planes)
        mine = [glf.fit_coeffs(G, b, lib_pen)]
        objs = []
        for i in range(its):
            G, b, lo, ma, wout, _ = g.robust_step(d_planes, mine[-1], loss, sigma=sigma, weight=d_w, want_weights=True)
            objs.append(_objective(lo, pen, mine[-1], sigma))
            mine.append(glf.fit_coeffs(G, b, lib_pen))
        _same(info["coeffs"], mine[-1])
        assert torch.equal(info["weights"].view(torch.int32), wout.view(torch.int32)) and info["mass"] == ma
        np.testing.assert_allclose(info["objective"], np.array(objs), rtol=2.0 ** -48, atol=0.0)    # (the penalty's sum is ordered differently)
        np.testing.assert_array_equal(info["sigma"], sigma)
        assert torch.equal(fit.view(torch.int32), g.synthesize(mine[-1]).view(torch.int32))
        for i in (1, 2):                                                          # a shorter run is a prefix
            if i < its:
                short = g.fit_robust(d_planes, d_w, loss=loss, sigma=sigma, penalty=lib_pen, max_iter=i, return_info=True)[1]
                _same(short["coeffs"], mine[i])
                assert short["iterations"] == i and short["converged"] == 0
        g.close()
    objs = list(info["objective"])
    print("%s ridge %g %s: %d iterations, converged %d, objective %.9e -> %.9e (reference %.9e -> %.9e)" %
          (shape, ridge, loss, its, info["converged"], objs[0], objs[-1], obj64[0], obj64[its - 1]))
    # the reference's objective does not increase
    for i in range(len(obj64) - 1):
        assert obj64[i + 1] <= obj64[i] * (1.0 + 2.0 ** -40), (i, obj64[i], obj64[i + 1])
    # per iteration within the perturbation bound
    for i in range(its + 1):
        weff = wv if i == 0 else weffs[i - 1]
        bound = _irls_bound(phi, s, wv, weff, pen, a64[i])
        err = np.linalg.norm(mine[i] - a64[i], axis=1)
        print("  iterate %d: max ||a - a64|| / bound %.3e" % (i, float((err / bound).max())))
        assert np.all(err <= bound), (shape, loss, i, err, bound)
        if i > 0 and np.all(np.linalg.norm(a64[i] - a64[i - 1], axis=1) <= bound):
            break
    # the library's objective
    sb = [sum((_synth_want(phi, ld, mine[i][k], 0.0, -1, s)[1] / sigma[k] for k in range(3)), np.zeros(n)) for i in range(its)]
    for i in range(its - 1):
        E = c * float((wv * np.maximum(sb[i], sb[i + 1])).sum()) + 2.0 ** -40 * objs[i]
        assert objs[i + 1] <= objs[i] + 2.0 * E, (shape, loss, i, objs[i], objs[i + 1], E)
    assert info["converged"] == 1 and its <= 20, (shape, loss, its)


# ---- 6. it rejects outliers ----------------------------------------------------------------------------------------------------------

# loss: (f, A, c)
OUTLIERS = {"huber": (0.1, 100.0, 1.345), "cauchy": (0.1, 100.0, 2.385), "tukey": (0.05, 100.0, 7.0)}


@pytest.mark.parametrize("loss", LOSSES)
def test_fit_rejects_outliers(loss):
    """ld64 shape, all 40 columns. s = Phi a_true + noise of standard deviation sigma0 = 1 (a_true: every column alike, scaled so that
    the clean plane has a standard deviation of 30), then a fraction f of the pixels replaced by s +/- A sigma0, seed 43; the scale
    is the driver's estimate, no penalty, up to 30 steps. Huber and Cauchy: f = 0.1, A = 100 and the default constants 1.345 and
    2.385. Tukey: f = 0.05, A = 100, c = 7: from the plain fit, which 10 % of such outliers bend, its non-convex loss settles in a
    local minimum at the default constant (reference RMS error 1.09 against the plain fit's 1.72; nothing cleverer than the plain
    start is done).
    Conditions on the input, checked on the f64 reference alone: its robust fit's RMS error against Phi a_true on the clean pixels
    is at most a quarter of its plain fit's, at least 90 % of the corrupted pixels have w_eff < 0.1 and at least 90 % of the clean ones
    w_eff > 0.5 (measured: 0.990 / 0.999 for huber, 0.990 / 0.997 for cauchy, 0.994 / 1.000 for tukey; the missing corrupted pixels
    are those a column of Phi follows on its own). Then the library's fit is within _irls_bound of the reference's and its weight
    map meets the same two fractions."""
    width, h, _, _, m, ld = SHAPES["ld64"]
    n = width * h
    rng = np.random.default_rng(43)
    f, A, c = OUTLIERS[loss]
    sigma0 = 1.0
    with glf.Context(0) as ctx:
        g, _, _ = _grey_graph(ctx, "ld64")
        phi = _phi64(g)
        a_true = np.ones(m)
        a_true *= 30.0 / float((phi @ a_true).std())
        clean = phi @ a_true
        s = clean + rng.normal(0.0, sigma0, n)
        bad = rng.uniform(size=n) < f
        s[bad] += A * sigma0 * rng.choice([-1.0, 1.0], int(bad.sum()))
        s32 = s.astype(F32).reshape(1, n)
        s = s32.astype(np.float64)
        d_planes = _dev(ctx, s32.reshape(1, h, width))
        plain = g.fit(d_planes).cpu().numpy().reshape(n).astype(np.float64)
        fit, info = g.fit_robust(d_planes, loss=loss, c=c, max_iter=30, return_info=True)
        robust = fit.cpu().numpy().reshape(n).astype(np.float64)
        weights = info["weights"].cpu().numpy().reshape(n)
        g.close()
    wv, pen = np.ones(n), np.zeros(m)
    its = info["iterations"]
    a64, _, weffs = _ref_irls(phi, s, wv, pen, info["sigma"], loss, c, its)
    rms = lambda z: float(np.sqrt(np.mean((z[~bad] - clean[~bad]) ** 2)))  # noqa: E731
    ref_plain, ref_robust = rms(phi @ a64[0][0]), rms(phi @ a64[-1][0])
    ref_out, ref_in = float((weffs[-1][bad] < 0.1).mean()), float((weffs[-1][~bad] > 0.5).mean())
    got_out, got_in = float((weights[bad] < 0.1).mean()), float((weights[~bad] > 0.5).mean())
    print("%s: sigma %.3f, %d iterations (converged %d); RMS error on the clean pixels: plain %.4f (reference %.4f), robust %.4f "
          "(reference %.4f)" % (loss, info["sigma"][0], its, info["converged"], rms(plain), ref_plain, rms(robust), ref_robust))
    print("%s: corrupted pixels with w_eff < 0.1: %.3f (reference %.3f); clean pixels with w_eff > 0.5: %.3f (reference %.3f)" %
          (loss, got_out, ref_out, got_in, ref_in))
    assert ref_robust <= 0.25 * ref_plain and ref_out >= 0.9 and ref_in >= 0.9      # the input
    bound = _irls_bound(phi, s, wv, weffs[-1], pen, a64[-1])
    err = np.linalg.norm(info["coeffs"] - a64[-1], axis=1)
    print("%s: ||a - a64|| / bound %.3e" % (loss, float((err / bound).max())))
    assert np.all(err <= bound)
    assert got_out >= 0.9 and got_in >= 0.9
    assert rms(robust) <= 0.25 * rms(plain)


# ---- 7. the estimated scale ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,rows", [("ld32", 1000), ("ld128", 0), ("tiny", 4096)])
def test_estimated_scale(shape, rows):
    """stats.sigma = glf.robust_scale of the f64 residuals of the plain fit at the rows floor(i N / n_s), n_s = min(sample_rows, N)
    (0: 4096), over the sampled pixels of positive weight. Both sides form the residuals in f64 from the same f32 values."""
    width, h = SHAPES[shape][:2]
    n = width * h
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        m = g.info["m"]
        w = _weight("mask", n)
        d_w = _dev_weight(ctx, w, h, width)
        G, b = g.normal_equations(d_w, d_sig)
        pen = np.full(m, 0.01 * np.trace(G) / m)
        a0 = glf.fit_coeffs(G, b, pen)
        _, info = g.fit_robust(d_sig, d_w, penalty=pen, sample_rows=rows, max_iter=1, return_info=True)
        phi32 = g.phi.cpu().numpy()[:, :m]
        g.close()
    ns = min(rows if rows else 4096, n)
    px = (np.arange(ns, dtype=np.int64) * n) // ns
    res = s[:, px] - a0 @ phi32[px].astype(np.float64).T
    want = np.array([glf.robust_scale(res[k], w[px]) for k in range(3)])
    print("%s: sigma %s, want %s" % (shape, info["sigma"], want))
    assert np.all(np.abs(info["sigma"] - want) <= 2.0 ** -20 * want)


# ---- 8. refusals on a live context ---------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_context():
    lib = glf._lib
    width, h, _, _, m, _ = SHAPES["ld32"]
    n = width * h
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld32")
        a = np.zeros((3, m))
        G, b = np.full((m, m), -7.0), np.full((3, m), -7.0)
        lo, ma = C.c_double(-7.0), C.c_double(-7.0)
        wout = torch.full((h, width), -7.0, device=ctx.device)
        rout = torch.full((3, h, width), -7.0, device=ctx.device)
        fit = torch.full((3, h, width), -7.0, device=ctx.device)
        P = C.c_void_p(d_sig.data_ptr())
        torch.cuda.synchronize()

        def loss_of(size=None, kind=0, c=1.0, sigma=(1.0, 1.0, 1.0, 1.0)):
            rl = glf.RobustLoss(struct_size=C.sizeof(glf.RobustLoss) if size is None else size, kind=kind, c=c)
            for k in range(4):
                rl.sigma[k] = sigma[k]
            return rl

        def step(gh, rl, nplanes, planes, ha, hG, hb):
            return lib.glf_graph_robust_step(gh, C.byref(rl) if rl is not None else None, None, C.c_int(nplanes), planes, glf._ptr(ha), glf._ptr(hG),
                                             glf._ptr(hb), C.byref(lo), C.byref(ma), C.c_void_p(wout.data_ptr()), C.c_void_p(rout.data_ptr()))

        nan, inf = float("nan"), float("inf")
        bad_a = a.copy()
        bad_a[2, m - 1] = nan
        bad_losses = [loss_of(size=8), loss_of(kind=3), loss_of(kind=-1), loss_of(c=-1.0), loss_of(c=nan), loss_of(c=inf),
                      loss_of(sigma=(1.0, 0.0, 1.0, 1.0)), loss_of(sigma=(1.0, 1.0, -1.0, 1.0)), loss_of(sigma=(nan, 1.0, 1.0, 1.0)),
                      loss_of(sigma=(1.0, 1.0, inf, 1.0))]
        ok = loss_of()
        cases = [(None, ok, 3, P, a, G, b), (g._g, None, 3, P, a, G, b), (g._g, ok, 3, None, a, G, b), (g._g, ok, 3, P, None, G, b),
                 (g._g, ok, 3, P, a, None, b), (g._g, ok, 3, P, a, G, None), (g._g, ok, 0, P, a, G, b), (g._g, ok, 5, P, a, G, b),
                 (g._g, ok, 3, P, bad_a, G, b)] + [(g._g, rl, 3, P, a, G, b) for rl in bad_losses]
        for i, args in enumerate(cases):
            assert step(*args) == glf.ERR_INVALID, i
        ctx.synchronize()
        assert np.all(G == -7.0) and np.all(b == -7.0) and lo.value == ma.value == -7.0
        assert bool((wout == -7.0).all()) and bool((rout == -7.0).all())
        # a sigma past nplanes is not read; c = 0 is the default
        assert step(g._g, loss_of(c=0.0, sigma=(1.0, nan, nan, nan)), 1, P, a[:1], G, b) == glf.OK
        assert np.all(G != -7.0) and bool((wout != -7.0).all()) and bool((rout[0] != -7.0).all()) and bool((rout[1:] == -7.0).all())
        wout.fill_(-7.0)
        torch.cuda.synchronize()

        def drive(gh, opt, nplanes, planes, ha, st):
            return lib.glf_graph_fit_robust(gh, C.byref(opt) if opt is not None else None, None, C.c_int(nplanes), planes, glf._ptr(ha),
                                            C.c_void_p(fit.data_ptr()), C.c_void_p(wout.data_ptr()), C.byref(st) if st is not None else None)

        def opt_of(rl=None, size=None, est=0, tol=0.0, penalty=None):
            return glf.RobustOptions(struct_size=C.sizeof(glf.RobustOptions) if size is None else size, loss=rl if rl is not None else loss_of(),
                                     penalty=penalty.ctypes.data if penalty is not None else None, tol=tol, estimate_sigma=est)

        st = glf.RobustStats(struct_size=C.sizeof(glf.RobustStats))
        bad_st = glf.RobustStats(struct_size=12)
        ha = np.full((3, m), -7.0)
        neg_pen, nan_pen = np.full(m, -1.0), np.full(m, nan)
        dcases = [(None, opt_of(), 3, P, ha, st), (g._g, None, 3, P, ha, st), (g._g, opt_of(), 3, None, ha, st), (g._g, opt_of(), 3, P, None, st),
                  (g._g, opt_of(), 0, P, ha, st), (g._g, opt_of(), 5, P, ha, st), (g._g, opt_of(size=16), 3, P, ha, st), (g._g, opt_of(), 3, P, ha, bad_st),
                  (g._g, opt_of(est=2), 3, P, ha, st), (g._g, opt_of(est=-1), 3, P, ha, st), (g._g, opt_of(tol=-1.0), 3, P, ha, st),
                  (g._g, opt_of(tol=nan), 3, P, ha, st), (g._g, opt_of(penalty=neg_pen), 3, P, ha, st), (g._g, opt_of(penalty=nan_pen), 3, P, ha, st)]
        dcases += [(g._g, opt_of(rl=rl), 3, P, ha, st) for rl in bad_losses]
        dcases += [(g._g, opt_of(rl=rl, est=1), 3, P, ha, st) for rl in bad_losses[:6]]
        for i, args in enumerate(dcases):
            assert drive(*args) == glf.ERR_INVALID, i
        ctx.synchronize()
        assert np.all(ha == -7.0) and st.iterations == 0 and bool((fit == -7.0).all()) and bool((wout == -7.0).all())
        # with estimate_sigma the given scales are not read
        assert drive(g._g, opt_of(rl=loss_of(sigma=(nan, -1.0, 0.0, inf)), est=1), 3, P, ha, st) == glf.OK
        assert st.iterations >= 1 and np.all(ha != -7.0) and bool((fit != -7.0).all())
        # the Python layer's own checks
        with pytest.raises(ValueError):
            g.robust_step(d_sig, a[:2], "huber")
        with pytest.raises(ValueError):
            g.robust_step(d_sig, a, "l1")
        with pytest.raises(ValueError):
            g.fit_robust(d_sig, penalty=np.zeros(m + 1))
        with pytest.raises(glf.GlfError):
            g.robust_step(d_sig, a, "huber", sigma=0.0)
        with pytest.raises(glf.GlfError):
            g.fit_robust(d_sig, sigma=-1.0)
        # a constant plane in the span of nothing: the plain fit's residuals on a zero plane are zero, the scale cannot be estimated
        with pytest.raises(glf.GlfError) as ei:
            g.fit_robust(torch.zeros((1, h, width), device=ctx.device))
        assert "pass sigma" in str(ei.value)
        first = g.robust_step(d_sig, a, "huber", sigma=2.0)
        handle = g._g
        g.close()
        # a closed handle: the Python object refuses (its handle is NULL), and the library refuses NULL
        assert not g._g
        with pytest.raises(glf.GlfError):
            g.robust_step(d_sig, a, "huber")
        with pytest.raises(glf.GlfError):
            g.fit_robust(d_sig, sigma=1.0)
        assert handle and np.isfinite(first[2])


# ---- 9. the work buffers on a debug pool ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ld32", "ld256"])
def test_robust_fit_on_a_debug_pool(monkeypatch, shape):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    rng = np.random.default_rng(47)
    width, h = SHAPES[shape][:2]
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        a, sigma, _ = _start(g, d_sig, rng)
        d_w = _dev_weight(ctx, _weight("uniform", width * h), h, width)
        first = g.robust_step(d_sig, a, "cauchy", sigma=sigma, weight=d_w)         # (the weights go to a pool buffer)
        fit, info = g.fit_robust(d_sig, d_w, loss="huber", ridge=0.1, return_info=True)
        ctx.image_processing(ctx.to_device(glf.synth_image(96, 80, seed=4)), glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.1))
        second = g.robust_step(d_sig, a, "cauchy", sigma=sigma, weight=d_w, want_weights=True, want_residuals=True)
        fit2 = g.fit_robust(d_sig, d_w, loss="huber", ridge=0.1)
        _same(second[0], first[0])
        _same(second[1], first[1])
        assert second[2:4] == first[2:4]
        assert torch.equal(fit.view(torch.int32), fit2.view(torch.int32))
        assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all() and bool(torch.isfinite(fit).all())
        assert bool(torch.isfinite(second[4]).all()) and bool(torch.isfinite(second[5]).all()) and np.isfinite(info["objective"]).all()
        assert ctx.debug_violations() == 0
        g.close()
        assert ctx.debug_violations() == 0
