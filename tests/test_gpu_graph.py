"""The graph handle (glf_graph_* / glf.Context.graph): the eigenbasis of an image built once, then projections c = Phi^T s and
syntheses out = ident s + Phi a on it (k_graph_synthesize: v_mfma_f32_32x32x2_f32, one pass over Phi for up to 32 outputs).

Shapes (uniform sampler; epsilon = 0.1, nothing here depends on convergence): 61 x 47 = 2867 = 89 * 32 + 19 pixels, so the last
32-pixel tile is partial, at every row stride -- 100 samples asked (108 realised) with m = 8 (ld 32) and m = 40 (ld 64), 200 asked
(300 realised) with m = 100 (ld 128) and m = 200 (ld 256) -- and 16 x 10 (12 asked, 15 realised, m = 4): 5 tiles, fewer than the
waves of two workgroups. At those sizes every wave takes at most one tile; 509 x 515 (8192 tiles, the last of 23 pixels) has more
tiles than waves can be resident, so the kernel's grid-strided loop iterates (test_synthesize_many_tiles_per_wave, every ld).

Bounds. Projection: |got - want| <= N 2^-51 sum_px |Phi[px][j] s[px]| per entry, the f64 summation bound of both sides (the
products are exact in f64). Synthesis: |got - want| <= (ld + 4) 2^-24 (|ident s| + sum_j |Phi[px][j] a_j|) per pixel, the f32
bound of an ld-term sum plus the roundings of (float)a, of the identity product and of the final add. The library's own filters
through the handle: the project's rule ||got - want|| <= 1e-5 ||want|| + 2^-24 ||z|| on the correction against fp64 (CORR_TOL of
tests/test_gpu_pix_signals.py), and twice that against the plain call's float z (both approximate the same fp64 value)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import rgb_ref  # noqa: E402
import test_gpu_f32 as tf32  # noqa: E402
import test_gpu_rgbf32 as trgbf32  # noqa: E402
from test_gpu_pix_band import MODES, _bits  # noqa: E402
from test_gpu_pix_signals import CORR_TOL, _test_planes  # noqa: E402
from test_gpu_rgb import _rgb_image  # noqa: E402
from test_gpu_u16 import _u16_image  # noqa: E402

C = glf.C
W, H = 61, 47
# name: (width, height, num_samples, realised p, m, ld)
SHAPES = {"ld32": (W, H, 100, 108, 8, 32), "ld64": (W, H, 100, 108, 40, 64), "ld128": (W, H, 200, 300, 100, 128),
          "ld256": (W, H, 200, 300, 200, 256), "tiny": (16, 10, 12, 15, 4, 32)}
shape_param = pytest.mark.parametrize("shape", list(SHAPES))
# the statistics of a call that are times (everything else must equal the capture call's)
TIMING_KEYS = ("ms_affinity", "ms_laplacian", "ms_eigen", "ms_nystroem", "ms_filter", "ms_total", "nystroem_kernel_ms", "nystroem_rowpass_ms",
               "nystroem_colpass_ms", "matvec_ms")


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _opt(shape, **kw):
    w, h, ns, p, m, ld = SHAPES[shape]
    return glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1, **kw)


def _grey_graph(ctx, shape, seed=3):
    """(graph, planes numpy [3, N] float64, device planes) on the synthetic grey image of a shape."""
    w, h, ns, p, m, ld = SHAPES[shape]
    assert glf.Sampling(w, h, ns).size == p                                     # the realised count the shape table states
    g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=seed)), _opt(shape))
    assert (g.info["p"], g.info["m"], g.info["ld"]) == (p, m, ld)
    sig = _test_planes(h, w)
    return g, sig.reshape(3, -1).astype(np.float64), _dev(ctx, sig)


def _phi64(g):
    return g.phi.cpu().numpy()[:, :g.info["m"]].astype(np.float64)


def _assert_synth(got, want, bound, what):
    err = np.abs(np.ravel(got).astype(np.float64) - np.ravel(want))
    worst = float((err / np.maximum(np.ravel(bound), 1e-300)).max())
    print("%s: max |got - want| / bound %.3f (max err %.3e)" % (what, worst, float(err.max())))
    assert np.all(err <= np.ravel(bound)), (what, worst)


def _synth_want(phi, ld, a, ident, plane, s):
    """(want, bound) of one output in fp64: ident s_plane + Phi a, and (ld + 4) 2^-24 (|ident s| + |Phi| |a|)."""
    idt = np.zeros(phi.shape[0]) if plane < 0 else float(ident) * s[plane]
    return idt + phi @ a, (ld + 4) * 2.0 ** -24 * (np.abs(idt) + np.abs(phi) @ np.abs(a))


# ---- 1. build is the capture call ----------------------------------------------------------------------------------------------------

def _fmt_cases():
    """name: (image, h_val, the plain call returning its info dict with capture=True)."""
    return {
        "u8": (glf.synth_image(W, H, seed=3), 30.0, lambda ctx, d, opt: ctx.image_processing(d, opt, want_float=True, capture=True)[-1]),
        "rgb8": (_rgb_image(H, W, 3), 30.0, lambda ctx, d, opt: ctx.image_processing_rgb(d, opt, want_float=True, capture=True)[-1]),
        "u16": (_u16_image(H, W, 3), 30.0 * 257.0, lambda ctx, d, opt: ctx.image_processing_u16(d, opt, want_float=True, capture=True)[-1]),
        "f32": (tf32._f32_image(H, W, 3), tf32.H_VAL, lambda ctx, d, opt: ctx.image_processing_f32(d, opt, capture=True)[-1]),
        "rgbf32": (trgbf32._f32_image(H, W, 3), trgbf32.H_VAL, lambda ctx, d, opt: ctx.image_processing_rgbf32(d, opt, capture=True)[-1]),
    }


def _assert_build_is_capture(g, info, pix, w, h):
    cap = info.pop("capture")
    np.testing.assert_array_equal(g.eigenvalues, info["eigvals"])
    np.testing.assert_array_equal(_bits(g.phi.cpu().numpy()), _bits(cap["phi"].cpu().numpy()))
    assert set(TIMING_KEYS) <= set(info)
    for key, v in info.items():
        if key not in TIMING_KEYS and key != "eigvals":
            assert g.stats[key] == v, (key, g.stats[key], v)
    assert g.info == dict(pix=pix, width=w, height=h, p=info["p"], m=info["m"], ld=cap["ld"], phi_bytes=4 * w * h * cap["ld"])
    assert tuple(g.phi.shape) == (w * h, cap["ld"]) and g.phi.dtype == torch.float32


@pytest.mark.parametrize("fmt", ["u8", "rgb8", "u16", "f32", "rgbf32"])
def test_build_is_the_capture_call(fmt):
    img, h_val, plain = _fmt_cases()[fmt]
    opt = glf.default_options(num_samples=100, num_eigvals=8, epsilon=0.1, h_val=h_val, filter_mode=glf.FILTER_SMOOTH)
    pix = ["u8", "rgb8", "u16", "f32", "rgbf32"].index(fmt)
    with glf.Context(0) as ctx:
        d = _dev(ctx, img)
        info = plain(ctx, d, opt)
        with ctx.graph(d, opt) as g:
            _assert_build_is_capture(g, info, pix, W, H)
            assert (g.info["p"], g.info["m"], g.info["ld"]) == (108, 8, 32)


@pytest.mark.parametrize("fmt", ["u8", "rgb8"])
def test_build_on_the_forced_band_form(fmt):
    w, h = 96, 80
    img = glf.synth_image(w, h, seed=3) if fmt == "u8" else _rgb_image(h, w, 3)
    plain = _fmt_cases()[fmt][2]
    opt = glf.default_options(num_samples=120, num_eigvals=8, epsilon=0.1)
    with glf.Context(0) as ctx:
        ctx.set_tuning(NYS_PATH="band", MV_PATH="band", **({} if fmt == "u8" else dict(PIX_BAND="1")))
        d = _dev(ctx, img)
        info = plain(ctx, d, opt)
        with ctx.graph(d, opt) as g:
            assert g.stats["nystroem_path"] == 4 and g.stats["filter_fused"] == 0
            _assert_build_is_capture(g, info, 0 if fmt == "u8" else 1, w, h)


# ---- 2. project against fp64 ---------------------------------------------------------------------------------------------------------

@shape_param
def test_project_against_fp64(shape):
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        phi = _phi64(g)
        four = torch.cat([d_sig, d_sig[:1]]).contiguous()
        got = {1: g.project(d_sig[2:3].contiguous()), 3: g.project(d_sig), 4: g.project(four)}
        g.close()
    n = phi.shape[0]
    rows = {1: [2], 3: [0, 1, 2], 4: [0, 1, 2, 0]}
    for nplanes, c in got.items():
        assert c.shape == (nplanes, phi.shape[1])
        for k, src in enumerate(rows[nplanes]):
            want = phi.T @ s[src]
            bound = n * 2.0 ** -51 * (np.abs(phi).T @ np.abs(s[src]))
            err = np.abs(c[k] - want)
            print("%s nplanes %d plane %d: max err / bound %.3e" % (shape, nplanes, k, float((err / bound).max())))
            assert np.all(err <= bound), (shape, nplanes, k)
    np.testing.assert_array_equal(got[4][3], got[4][0])                          # (the same plane twice: the same bits)
    np.testing.assert_array_equal(got[3], got[4][:3])


# ---- 3. synthesize against fp64 ------------------------------------------------------------------------------------------------------

def _outputs(nout, lam, c, rng):
    """Coefficients at the scale of lam c, identity factors from {0, 1, -0.5} and a plane map with -1, a repeated plane and every
    plane (nout = 1: plane 2)."""
    plane = np.array(([2] if nout == 1 else [-1, 0, 1, 2, 2] + [k % 3 for k in range(nout - 5)])[:nout], dtype=np.int32)
    ident = np.array([(0.0, 1.0, -0.5)[(k + 2) % 3] for k in range(nout)], dtype=np.float32)
    a = np.stack([lam * c[rng.integers(0, 3)] * rng.uniform(-1.5, 1.5, lam.size) for _ in range(nout)])
    return a, ident, plane


@shape_param
def test_synthesize_against_fp64(shape):
    ld = SHAPES[shape][5]
    rng = np.random.default_rng(11)
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, shape)
        phi, lam = _phi64(g), g.eigenvalues
        c = phi.T @ s.T                                                          # [m, 3]
        cases = [_outputs(nout, lam, c.T, rng) for nout in (1, 5, 32)]
        got = [g.synthesize(a, ident, plane, d_sig).cpu().numpy() for a, ident, plane in cases]
        free = g.synthesize(cases[1][0])                                         # no identity term at all: planes not needed
        g.close()
    for (a, ident, plane), z in zip(cases, got):
        assert z.shape == (a.shape[0], SHAPES[shape][1], SHAPES[shape][0]) and np.isfinite(z).all()
        for j in range(a.shape[0]):
            want, bound = _synth_want(phi, ld, a[j], ident[j], int(plane[j]), s)
            _assert_synth(z[j], want, bound, "%s nout %d output %d" % (shape, a.shape[0], j))
    for j in range(5):
        want, bound = _synth_want(phi, ld, cases[1][0][j], 0.0, -1, s)
        _assert_synth(free[j].cpu().numpy(), want, bound, "%s no identity output %d" % (shape, j))


# ---- 3b. the grid-strided loop: more tiles than resident waves -------------------------------------------------------------------

@pytest.mark.parametrize("m,ld", [(8, 32), (40, 64), (100, 128), (200, 256)])
def test_synthesize_many_tiles_per_wave(m, ld):
    """509 x 515 = 262 135 pixels = 8191 tiles of 32 and one of 23: more than the 4 waves x 7 workgroups x CUs that can be resident
    at the smallest LDS footprint, so every wave runs the tile loop more than once -- the prefetch of the next tile under the
    MFMAs, the fresh accumulator and the reuse of the wave's LDS image. Every pixel of all 32 outputs against fp64 (torch, on the
    device) at the bound of test 3, and three outputs against their 1-output calls bit for bit."""
    w, h = 509, 515
    n = w * h
    rng = np.random.default_rng(ld)
    with glf.Context(0) as ctx:
        assert (n + 31) // 32 > 4 * 7 * ctx.device_info()["num_cus"]
        assert glf.Sampling(w, h, 300).size == 324
        g = ctx.graph(ctx.to_device(glf.synth_image(w, h, seed=3)), glf.default_options(num_samples=300, num_eigvals=m, epsilon=0.1))
        assert (g.info["p"], g.info["m"], g.info["ld"]) == (324, m, ld)
        sig = _test_planes(h, w)
        d_sig = _dev(ctx, sig)
        phi = g.phi[:, :m].double()
        s = d_sig.reshape(3, n).double()
        c = (phi.T @ s.T).T.cpu().numpy()
        a, ident, plane = _outputs(32, g.eigenvalues, c, rng)
        got = g.synthesize(a, ident, plane, d_sig)
        ones = {j: g.synthesize(a[j:j + 1], ident[j:j + 1], plane[j:j + 1], d_sig)[0].cpu().numpy() for j in (0, 13, 31)}
        ta = torch.from_numpy(a).to(ctx.device)
        idt = torch.stack([torch.zeros(n, dtype=torch.float64, device=ctx.device) if plane[j] < 0 else float(ident[j]) * s[plane[j]]
                           for j in range(32)])
        want = idt + ta @ phi.T
        bound = (ld + 4) * 2.0 ** -24 * (idt.abs() + ta.abs() @ phi.abs().T)
        err = (got.reshape(32, n).double() - want).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        ok = bool(torch.all(err <= bound)) and bool(torch.isfinite(got).all())
        got = got.cpu().numpy()
        g.close()
    print("ld %d, %d tiles: max |got - want| / bound %.3f" % (ld, (n + 31) // 32, worst))
    assert ok, (ld, worst)
    for j, z in ones.items():
        np.testing.assert_array_equal(_bits(got[j]), _bits(z), err_msg="output %d of 32 against alone" % j)


# ---- 4. independence -----------------------------------------------------------------------------------------------------------------

def test_outputs_do_not_depend_on_their_neighbours():
    rng = np.random.default_rng(5)
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld64")
        c = (_phi64(g).T @ s.T).T
        a, ident, plane = _outputs(32, g.eigenvalues, c, rng)
        full = g.synthesize(a, ident, plane, d_sig).cpu().numpy()
        again = g.synthesize(a, ident, plane, d_sig).cpu().numpy()
        ones = [g.synthesize(a[j:j + 1], ident[j:j + 1], plane[j:j + 1], d_sig).cpu().numpy()[0] for j in range(32)]
        g.close()
    np.testing.assert_array_equal(_bits(full), _bits(again))
    for j in range(32):
        np.testing.assert_array_equal(_bits(full[j]), _bits(ones[j]), err_msg="output %d of 32 against alone" % j)


# ---- 5. the library's own filters through the handle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u8", "rgb8", "f32"])
@pytest.mark.parametrize("mode", list(MODES))
def test_library_filters_through_the_handle(fmt, mode):
    img, h_val, _ = _fmt_cases()[fmt]
    opt = glf.default_options(num_samples=100, num_eigvals=8, epsilon=0.1, h_val=h_val, filter_mode=MODES[mode])
    x = (img.reshape(-1, 3).T if fmt == "rgb8" else img.reshape(1, -1)).astype(np.float64)           # the guide's channels [nch, N]
    nch = x.shape[0]
    with glf.Context(0) as ctx:
        d = _dev(ctx, img)
        if fmt == "u8":
            zplain = ctx.image_processing(d, opt, want_float=True)[1].cpu().numpy()
        elif fmt == "rgb8":
            zplain = ctx.image_processing_rgb(d, opt, want_float=True)[1].cpu().numpy()
        else:
            zplain = ctx.image_processing_f32(d, opt)[0].cpu().numpy()
        with ctx.graph(d, opt) as g:
            planes = _dev(ctx, x.reshape(nch, H, W).astype(np.float32))
            c = g.project(planes)
            a, ident = glf.filter_coeffs(opt, g.eigenvalues, c, gram=g.gram() if mode == "sharpen" else None)
            got = g.synthesize(a, np.full(nch, ident, dtype=np.float32), np.arange(nch, dtype=np.int32), planes).cpu().numpy()
            phi, lam = _phi64(g), g.eigenvalues.copy()
    keep = 1.0 if MODES[mode] < glf.FILTER_SMOOTH else 0.0
    assert ident == keep
    gain = float(opt.gain) if mode == "reference" else 1.0
    zplain = zplain.reshape(nch, -1).astype(np.float64)
    for k in range(nch):
        want = gain * (phi @ rgb_ref.weights(phi, lam, MODES[mode], phi.T @ x[k]))
        z = keep * x[k] + want
        bound = CORR_TOL * float(np.linalg.norm(want)) + 2.0 ** -24 * float(np.linalg.norm(z))
        corr = got[k].reshape(-1).astype(np.float64) - keep * x[k]
        e64, eplain = float(np.linalg.norm(corr - want)), float(np.linalg.norm(corr - (zplain[k] - keep * x[k])))
        print("%s %s channel %d: |corr - fp64| %.3e <= %.3e, |corr - plain call| %.3e <= %.3e" % (fmt, mode, k, e64, bound, eplain, 2 * bound))
        assert e64 <= bound and eplain <= 2.0 * bound, (fmt, mode, k)


# ---- 6. a bank -------------------------------------------------------------------------------------------------------------------------

def test_a_bank_of_responses_in_one_synthesize():
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld64")
        phi, lam = _phi64(g), g.eigenvalues
        two = d_sig[1:3].contiguous()
        weights = np.stack([0.5 * lam, 3.0 * lam, 10.0 * lam, 1.0 - lam, -(lam + 5.0)])
        ident = np.array([1.0, 1.0, 1.0, 0.0, 1.0], dtype=np.float32)
        c = g.project(two)
        out = g.apply(two, weights, ident).cpu().numpy()
        g.close()
    assert out.shape == (5, 2, H, W)
    for r in range(5):
        for k in range(2):
            want, bound = _synth_want(phi, 64, weights[r] * c[k], ident[r], k, s[1:3])
            _assert_synth(out[r, k], want, bound, "bank response %d plane %d" % (r, k))


# ---- 7. the handle outlives other work on its context ------------------------------------------------------------------------------

def test_handle_outlives_other_calls_on_a_debug_pool(monkeypatch):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    rng = np.random.default_rng(2)
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld32")
        a, ident, plane = _outputs(5, g.eigenvalues, (_phi64(g).T @ s.T).T, rng)
        first = g.synthesize(a, ident, plane, d_sig).cpu().numpy()
        phi_before = g.phi.cpu().numpy().copy()
        ctx.image_processing(ctx.to_device(glf.synth_image(96, 80, seed=4)), glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.1))
        ctx.image_processing_rgb(_dev(ctx, _rgb_image(72, 90, 8)), glf.default_options(num_samples=80, num_eigvals=8, epsilon=0.1))
        with ctx.graph(_dev(ctx, _rgb_image(40, 32, 1)), glf.default_options(num_samples=30, num_eigvals=4, epsilon=0.1)) as other:
            assert other.info["m"] == 4
        second = g.synthesize(a, ident, plane, d_sig).cpu().numpy()
        np.testing.assert_array_equal(_bits(g.phi.cpu().numpy()), _bits(phi_before))
        np.testing.assert_array_equal(_bits(second), _bits(first))
        assert ctx.debug_violations() == 0
        cached = ctx.cached_bytes()
        g.close()
        assert ctx.cached_bytes() == cached                                      # Phi goes back to the driver, not into the pool
        assert ctx.debug_violations() == 0


# ---- 8. refusals on a live context ---------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_context():
    lib = glf._lib
    rng = np.random.default_rng(3)
    with glf.Context(0) as ctx:
        g, s, d_sig = _grey_graph(ctx, "ld32")
        m, n = g.info["m"], W * H
        a, ident, plane = _outputs(5, g.eigenvalues, (_phi64(g).T @ s.T).T, rng)
        first = g.synthesize(a, ident, plane, d_sig).cpu().numpy()
        cbuf = np.zeros((5, m))
        out = torch.zeros((33, n), dtype=torch.float32, device=ctx.device)
        P, O = C.c_void_p(d_sig.data_ptr()), C.c_void_p(out.data_ptr())
        for nplanes, planes, hc in ((0, P, glf._ptr(cbuf)), (5, P, glf._ptr(cbuf)), (-1, P, glf._ptr(cbuf)), (3, None, glf._ptr(cbuf)), (3, P, None)):
            assert lib.glf_graph_project(g._g, nplanes, planes, hc) == glf.ERR_INVALID, (nplanes, planes, hc)
        A = np.zeros((33, m))
        idn, pl = np.zeros(33, dtype=np.float32), np.zeros(33, dtype=np.int32)
        bad_pl = pl.copy()
        bad_pl[2] = 3                                                            # plane[j] = nplanes
        low_pl = pl.copy()
        low_pl[1] = -2
        for nout, pa, pi, pp, npl, dp, do in ((0, A, idn, pl, 3, P, O), (33, A, idn, pl, 3, P, O), (5, None, idn, pl, 3, P, O),
                                              (5, A, idn, None, 3, P, O), (5, A, idn, pl, 3, None, O), (5, A, idn, pl, 3, P, None),
                                              (5, A, None, pl, 3, P, O), (5, A, idn, bad_pl, 3, P, O), (5, A, idn, low_pl, 3, P, O),
                                              (5, A, idn, pl, 0, P, O), (5, A, idn, pl, -1, P, O)):
            rc = lib.glf_graph_synthesize(g._g, nout, glf._ptr(pa), glf._ptr(pi), glf._ptr(pp), npl, dp, do)
            assert rc == glf.ERR_INVALID, (nout, npl)
        gi = glf.GraphInfo(struct_size=C.sizeof(glf.GraphInfo) + 8)
        assert lib.glf_graph_get_info(g._g, C.byref(gi)) == glf.ERR_INVALID
        assert lib.glf_graph_get_info(g._g, None) == glf.ERR_INVALID and lib.glf_graph_eigenvalues(g._g, None) == glf.ERR_INVALID
        assert lib.glf_graph_gram(g._g, None) == glf.ERR_INVALID
        d = ctx.to_device(glf.synth_image(W, H, seed=3))
        with pytest.raises(glf.GlfError) as e:                                   # more than 256 eigenpairs
            ctx.graph(d, glf.default_options(num_samples=400, num_eigvals=300, epsilon=0.1))
        assert e.value.status == glf.ERR_UNSUPPORTED
        bad = glf.default_options()
        bad.struct_size += 4
        handle = C.c_void_p(1)
        assert lib.glf_graph_build(ctx._ctx, C.byref(bad), 0, C.c_void_p(d.data_ptr()), W, H, C.byref(handle), None) == glf.ERR_INVALID
        assert not handle.value
        handle = C.c_void_p(1)
        assert lib.glf_graph_build(ctx._ctx, None, 5, C.c_void_p(d.data_ptr()), W, H, C.byref(handle), None) == glf.ERR_INVALID and not handle.value
        for fimg in (tf32._f32_image(H, W, 3), trgbf32._f32_image(H, W, 3)):    # a float image with one NaN: refused, no handle
            fimg = fimg.copy()
            fimg.reshape(-1)[1234] = np.nan
            with pytest.raises(glf.GlfError) as e:
                ctx.graph(_dev(ctx, fimg), glf.default_options(num_samples=100, num_eigvals=8, epsilon=0.1))
            assert e.value.status == glf.ERR_INVALID and "NaN" in str(e.value)
        with pytest.raises(ValueError):
            ctx.graph(torch.zeros((H, W), dtype=torch.float64, device=ctx.device))
        with glf.Multi(2, devices=[0, 0], backend=glf.MULTI_LOOPBACK) as world:  # a context that carries a communicator
            handle = C.c_void_p(1)
            rc = lib.glf_graph_build(C.c_void_p(lib.glf_multi_ctx(world._w, 0)), None, 0, C.c_void_p(d.data_ptr()), W, H, C.byref(handle), None)
            assert rc == glf.ERR_UNSUPPORTED and not handle.value
        # nothing faulted, and the next valid calls on the context and on the handle succeed
        again = g.synthesize(a, ident, plane, d_sig).cpu().numpy()
        np.testing.assert_array_equal(_bits(again), _bits(first))
        with ctx.graph(d, _opt("ld32")) as g2:
            np.testing.assert_array_equal(g2.eigenvalues, g.eigenvalues)
        g.close()
        g.close()                                                                # (closing twice is harmless)
