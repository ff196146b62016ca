"""Joint filtering under a colour or a 16-bit guide (glf_image_processing_rgb_signals / glf_image_processing_u16_signals): float
planes go through the graph filter of the colour / 16-bit image, in the two passes over Phi the plain call makes.

The guide's outputs (image, float z, eigenvalues, every non-timing statistic) must be bit-identical to the plain _rgb / _u16 call on
the same context, on the entry-by-entry route and on the PIX_BAND route. Each plane s must come out as (1 - ysub) s + gain Phi w_s,
w_s = f(Pi) Phi^T s (sharpening: the Gram-matrix weights), checked in fp64 numpy (tests/rgb_ref.py, tests/u16_ref.py) on the run's
own Phi and eigenvalues, which the capture call on the same context returns.

Tolerance. A plane's correction z - (1 - ysub) s is held to ||got - want|| <= 1e-5 ||want|| + 2^-24 ||z||: the project's CORR_TOL
plus the resolution of the float output itself (test_fused_band_path_at_2048's rule). The second term is needed: at 61 x 47 with 100
samples and 8 eigenpairs a float32 z alone resolves the correction of the depth-like plane (level ~1000, correction rms 1.3) to
1.3e-5 only, the two planes of test_gpu_signals._planes to 3.4e-7 and 1.8e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_pix_band import FMTS, MODES, _bits, _route  # noqa: E402
from test_gpu_signals import _planes  # noqa: E402

CORR_TOL = 1e-5
fmt_param = pytest.mark.parametrize("fmt", list(FMTS))
SMALL = dict(w=61, h=47, ns=100, m=8)


def _test_planes(h, w, seed=0):
    """The two planes of test_gpu_signals (signed noise; smooth and positive) and a depth-like one: a disc 400 above a floor of
    1000 under sigma = 15 noise."""
    a, b = _planes(h, w, seed)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    depth = 1000.0 + 400.0 * disc + np.random.default_rng(seed + 100).normal(0.0, 15.0, (h, w))
    return np.stack([a, b, depth.astype(np.float32)]).astype(np.float32)


def _run(f, ctx, img, sig, opt):
    fn = ctx.image_processing_u16_signals if f.u16 else ctx.image_processing_rgb_signals
    d_sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32)).to(ctx.device)
    out, zf, so, info = fn(f.dev(ctx, img), d_sig, opt, want_float=True)
    return out.cpu().numpy(), zf.cpu().numpy(), so.cpu().numpy(), info


def _assert_guide_equal(got, plain, what=""):
    """(out, zf, info) of a signals call against the plain call's: bit for bit, and every statistic that is not a time."""
    (out, zf, info), (out1, zf1, info1) = got, plain
    np.testing.assert_array_equal(out, out1, err_msg=what)
    np.testing.assert_array_equal(_bits(zf), _bits(zf1), err_msg=what)
    np.testing.assert_array_equal(info["eigvals"], info1["eigvals"], err_msg=what)
    assert _route(info) == _route(info1), what
    for key, v in info1.items():
        if "ms" not in key and key not in ("eigvals", "capture"):
            assert info[key] == v, (what, key, info[key], v)


def _ysub(mode):
    return 1.0 if mode >= glf.FILTER_SMOOTH else 0.0


def _want_corr(f, phi, lam, mode, gain, sig):
    """gain Phi w_s in fp64 for each plane: [nsig, N]."""
    g = gain if mode == glf.FILTER_REFERENCE else 1.0
    s = sig.reshape(sig.shape[0], -1).astype(np.float64)
    return np.stack([g * (phi @ f.ref.weights(phi, lam, mode, phi.T @ s[k])) for k in range(s.shape[0])])


def _assert_corr(got_z, s, want, mode, what):
    """||got - want|| <= CORR_TOL ||want|| + 2^-24 ||z|| with z = (1 - ysub) s + want in fp64."""
    s = np.ravel(s).astype(np.float64)
    got = np.ravel(got_z).astype(np.float64) - (1.0 - _ysub(mode)) * s
    z = (1.0 - _ysub(mode)) * s + np.ravel(want)
    err, bound = float(np.linalg.norm(got - np.ravel(want))), CORR_TOL * float(np.linalg.norm(want)) + 2.0 ** -24 * float(np.linalg.norm(z))
    print("%s: |got - want| %.3e <= %.3e (rel %.2e of the correction)" % (what, err, bound, err / float(np.linalg.norm(want))))
    assert err <= bound, (what, err, bound)


def _captured(f, ctx, img, opt, m):
    """The plain call with its by-products: ((out, zf, info), Phi [N, m] fp64, eigenvalues)."""
    out, zf, info = f.whole(ctx, img, opt, capture=True)
    phi = info["capture"]["phi"].cpu().numpy()[:, :m].astype(np.float64)
    del info["capture"]
    return (out, zf, info), phi, np.asarray(info["eigvals"], dtype=np.float64)


# ---- 1. the guide keeps its bits ------------------------------------------------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("sampling", [glf.SAMPLING_UNIFORM, glf.SAMPLING_RANDOM])
def test_guide_bit_identical_to_plain_call(fmt, sampling):
    f = FMTS[fmt]
    w, h, ns, m = (SMALL[k] for k in ("w", "h", "ns", "m"))
    img, sig = f.image(h, w, seed=3), _test_planes(h, w)
    with glf.Context(0) as ctx:
        for name, mode in MODES.items():
            opt = f.options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=mode, sampling=sampling)
            plain = f.whole(ctx, img, opt)
            out, zf, so, info = _run(f, ctx, img, sig, opt)
            _assert_guide_equal((out, zf, info), plain, name)
            assert _route(info) == (0, 0, 0)
            assert np.isfinite(so).all(), name


# ---- 2. / 3. the planes against fp64, and a plane that is a guide channel -----------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("mode", list(MODES))
def test_planes_against_fp64(fmt, mode):
    f = FMTS[fmt]
    w, h, ns, m = (SMALL[k] for k in ("w", "h", "ns", "m"))
    img = f.image(h, w, seed=3)
    chan = f.planes(img)[-1].reshape(1, h, w).astype(np.float32)            # the 16-bit image / the blue channel as a plane
    sig = np.concatenate([_test_planes(h, w), chan])
    opt = f.options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode])
    with glf.Context(0) as ctx:
        plain, phi, lam = _captured(f, ctx, img, opt, m)
        out, zf, so, info = _run(f, ctx, img, sig, opt)
    np.testing.assert_array_equal(info["eigvals"], plain[2]["eigvals"])
    _assert_guide_equal((out, zf, info), plain, mode)
    want = _want_corr(f, phi, lam, MODES[mode], float(opt.gain), sig)
    for k in range(sig.shape[0]):
        _assert_corr(so[k], sig[k], want[k], MODES[mode], "%s %s plane %d" % (fmt, mode, k))
    # the plane that is the guide's last channel comes out as that channel's float z
    zch = zf.reshape(-1, h * w)[-1].astype(np.float64)
    s = sig[-1].reshape(-1).astype(np.float64)
    _assert_corr(so[-1], s, zch - (1.0 - _ysub(MODES[mode])) * s, MODES[mode], "%s %s plane = channel against zf" % (fmt, mode))


# ---- 4. independence and linearity -------------------------------------------------------------------------------------------------------

@fmt_param
def test_planes_independent_and_linear(fmt):
    f = FMTS[fmt]
    w, h, ns, m = (SMALL[k] for k in ("w", "h", "ns", "m"))
    img = f.image(h, w, seed=3)
    s1, s2 = _planes(h, w, 7)
    depth = _test_planes(h, w, 7)[2]
    chan = f.planes(img)[0].reshape(h, w).astype(np.float32)
    a, b = 0.75, -2.5
    opt = f.options(num_samples=ns, num_eigvals=m, epsilon=1e-3)
    with glf.Context(0) as ctx:
        four = _run(f, ctx, img, np.stack([s1, s2, depth, chan]), opt)[2]
        two = _run(f, ctx, img, np.stack([s2, s1]), opt)[2]
        ones = [_run(f, ctx, img, s[None], opt)[2][0] for s in (s1, s2, depth, chan)]
        comb = (a * s1.astype(np.float64) + b * s2).astype(np.float32)
        lin = _run(f, ctx, img, comb[None], opt)[2][0]
    for k in range(4):
        np.testing.assert_array_equal(_bits(four[k]), _bits(ones[k]), err_msg="plane %d of 4 against alone" % k)
    np.testing.assert_array_equal(_bits(two[0]), _bits(ones[1]))
    np.testing.assert_array_equal(_bits(two[1]), _bits(ones[0]))
    corr = lambda z, s: z.astype(np.float64) - s   # noqa: E731
    want = a * corr(four[0], s1) + b * corr(four[1], s2)
    r = float(np.linalg.norm(corr(lin, comb) - want) / np.linalg.norm(want))
    print("linearity (%s): rel %.2e" % (fmt, r))
    assert r <= 1e-5, r


# ---- 5. the PIX_BAND route -----------------------------------------------------------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("mode", list(MODES))
def test_pix_band_route(fmt, mode):
    f = FMTS[fmt]
    w, h, ns, m = 96, 80, 120, 8
    img, sig = f.image(h, w, seed=3), _test_planes(h, w, 2)
    opt = f.options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode])
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1", NYS_PATH="band", MV_PATH="band")
        plain, phi, lam = _captured(f, ctx, img, opt, m)
        out, zf, so, info = _run(f, ctx, img, sig, opt)
    assert _route(info) == (4, 4, 0) and _route(plain[2]) == (4, 4, 0)
    _assert_guide_equal((out, zf, info), plain, mode)
    want = _want_corr(f, phi, lam, MODES[mode], float(opt.gain), sig)
    for k in range(sig.shape[0]):
        _assert_corr(so[k], sig[k], want[k], MODES[mode], "PIX_BAND %s %s plane %d" % (fmt, mode, k))


# ---- 6. the wider row strides and the grid-strided launch ----------------------------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("w,h,ns,m,ld", [(96, 80, 300, 99, 128), (96, 80, 300, 130, 256), (640, 416, 300, 16, 32)])
def test_leading_dimensions_and_grid_stride(fmt, w, h, ns, m, ld):
    """ld = 128 and 256, and at ld = 32 more pixels (266 240) than the 8192 blocks x 32 pixels of one sweep of the grid: the planes at
    64 sampled pixels against s + gain Phi[px] . w, with w in fp64 from the captured Phi."""
    f = FMTS[fmt]
    img, sig = f.image(h, w, seed=5), _test_planes(h, w, 4)
    opt = f.options(num_samples=ns, num_eigvals=m, epsilon=0.05)
    pix = np.sort(np.random.default_rng(1).choice(w * h, 64, replace=False))
    pix[-1] = w * h - 1                                                        # (the last pixel: the end of the strided sweep)
    with glf.Context(0) as ctx:
        out1, zf1, info1 = f.whole(ctx, img, opt, capture=True)
        cap = info1.pop("capture")
        assert cap["ld"] == ld
        phi = cap["phi"][:, :m].double()
        s = torch.from_numpy(sig.reshape(sig.shape[0], -1)).to(phi.device).double()
        c = (phi.T @ s.T).cpu().numpy()                                       # (m, nsig) fp64
        rows = phi[torch.from_numpy(pix).to(phi.device)].cpu().numpy()
        del phi, cap
        out, zf, so, info = _run(f, ctx, img, sig, opt)
    if w * h > 8192 * 32:
        assert ld == 32
    _assert_guide_equal((out, zf, info), (out1, zf1, info1))
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    for k in range(sig.shape[0]):
        want = float(opt.gain) * (rows @ (lam * c[:, k]))
        _assert_corr(so[k].reshape(-1)[pix], sig[k].reshape(-1)[pix], want, glf.FILTER_REFERENCE, "%s ld %d plane %d" % (fmt, ld, k))


# ---- 7. the debug pool -------------------------------------------------------------------------------------------------------------------

@fmt_param
def test_debug_pool_run(fmt, monkeypatch):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    f = FMTS[fmt]
    img = f.image(72, 90, seed=8)
    sig = np.concatenate([_test_planes(72, 90, 8), f.planes(img)[0].reshape(1, 72, 90).astype(np.float32)])
    for mode in ("reference", "sharpen"):
        opt = f.options(num_samples=80, num_eigvals=8, epsilon=0.05, filter_mode=MODES[mode])
        with glf.Context(0) as ctx:
            out, zf, so, info = _run(f, ctx, img, sig, opt)
            assert ctx.debug_violations() == 0
        assert so.shape == (4, 72, 90)
        assert np.isfinite(zf).all() and np.isfinite(so).all() and np.isfinite(info["eigvals"]).all()


# ---- 8. errors with a live context ---------------------------------------------------------------------------------------------------------

@fmt_param
def test_invalid_and_unsupported_with_a_live_context(fmt):
    f = FMTS[fmt]
    w, h = 40, 32
    img = f.image(h, w, seed=1)
    g = glf.synth_image(96, 80, seed=4)
    gopt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05)
    with glf.Context(0) as fresh:
        out0, zf0, _ = fresh.image_processing(fresh.to_device(g), gopt, want_float=True)
        out0, zf0 = out0.cpu().numpy(), zf0.cpu().numpy()
    C = glf.C
    name = "glf_image_processing_u16_signals" if f.u16 else "glf_image_processing_rgb_signals"
    other = glf.KERNEL_BILATERAL_RGB if f.u16 else glf.KERNEL_BILATERAL_U16
    with glf.Context(0) as ctx:
        d = f.dev(ctx, img)
        sig = torch.zeros((1, h, w), dtype=torch.float32, device=ctx.device)
        fn = ctx.image_processing_u16_signals if f.u16 else ctx.image_processing_rgb_signals
        out = torch.zeros(img.shape, dtype=torch.int16 if f.u16 else torch.uint8, device=ctx.device)
        opt = f.options(num_samples=30, num_eigvals=4)
        for nsig, ps, po in ((0, sig.data_ptr(), sig.data_ptr()), (5, sig.data_ptr(), sig.data_ptr()),
                             (1, None, sig.data_ptr()), (1, sig.data_ptr(), None)):
            rc = getattr(glf._lib, name)(ctx._ctx, C.byref(opt), C.c_void_p(d.data_ptr()), w, h, nsig, C.c_void_p(ps), C.c_void_p(po),
                                         C.c_void_p(out.data_ptr()), None, None, None)
            assert rc == glf.ERR_INVALID, (nsig, ps, po)
        for kernel in (glf.KERNEL_PHOTOMETRIC, glf.KERNEL_SPATIAL, glf.KERNEL_NLM, other):
            with pytest.raises(glf.GlfError) as e:
                fn(d, sig, f.options(num_samples=30, num_eigvals=4, kernel=kernel))
            assert e.value.status == glf.ERR_UNSUPPORTED, kernel
        with pytest.raises(glf.GlfError) as e:               # more than 256 eigenpairs
            fn(d, sig, f.options(num_samples=400, num_eigvals=300))
        assert e.value.status == glf.ERR_UNSUPPORTED
        _, _, so, info = fn(d, sig, f.options(num_samples=30, num_eigvals=4, kernel=f.kernel))   # the context still works
        assert info["m"] == 4 and torch.isfinite(so).all()
        out1, zf1, _ = ctx.image_processing(ctx.to_device(g), gopt, want_float=True)           # and a grey call is a fresh context's
        np.testing.assert_array_equal(out1.cpu().numpy(), out0)
        np.testing.assert_array_equal(_bits(zf1.cpu().numpy()), _bits(zf0))
