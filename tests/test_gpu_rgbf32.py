"""Float colour filtering (GLF_KERNEL_BILATERAL_RGBF32, glf_image_processing_rgbf32): the graph is built from the differences of three
float channels in the image's own units (negative and fractional included) and each channel goes through its filter; the output is
the float z, interleaved as the image.

Checked against the fp64 numpy restatement in tests/rgb_ref.py, which casts the image to float64 and so takes a float [H, W, 3]
image unchanged: the stage kernels, the whole path in every filter mode on both samplers, bit-equality with the 8-bit colour call on
integer values, exact covariance under a power-of-two scale, the grey image replicated into three channels, the band form behind
PIX_BAND, joint filtering, the refusals (NaN / Inf, kernel mismatches, m > 256), the context's bookkeeping and sampled rows at
1024 x 256.

Tolerances: those of tests/test_gpu_rgb.py / tests/test_gpu_f32.py. Each of the three float differences is rounded once, its square
once, and the two fmas once each; all terms are positive, so dist2 carries at most ~5 x 2^-24 relative error and an entry moves by at
most K t ln2 x 3e-7 <= 1.1e-7 (x e^-x <= 1/e), a factor 9 inside 1e-6: K_A and D_A within 1e-6 of their maxima, alpha within 1e-6,
eigenpair residuals <= 2e-2 max(lam, 1e-3) against the fp64 L_A, Phi and the corrections within 1e-5 relative L2."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import rgb_ref as ref  # noqa: E402

MODES = {"reference": glf.FILTER_REFERENCE, "poc": glf.FILTER_POC, "smooth": glf.FILTER_SMOOTH, "sharpen": glf.FILTER_SHARPEN}
H_LOC = 40.0
H_VAL = 30.0 / 4.0                                  # the colour suite's bandwidth in the float test image's units
H_VAL8 = 30.0
K96 = glf.KERNEL_BILATERAL_RGBF32


def _colour_pattern(h, w, seed=0):
    """The 8-bit colour suite's pattern before it is rounded: smooth colour ramps, a disc of another colour and noise (float64)."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([60 + 120 * c / max(1, w - 1), 200 - 100 * r / max(1, h - 1), 90 + 40 * np.sin(c / 7.0)], axis=2)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    img[disc] = [210, 40, 160]
    img += rng.normal(0.0, 6.0, img.shape)
    return img


def _grey_f32_image(h, w, seed=0):
    """The float grey suite's image: signed fractional values, about -35 .. +34 with noise sigma 1.5."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 9000.0 + 30000.0 * c / max(1, w - 1) + 12000.0 * np.sin(r / 9.0)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    img[disc] = 58000.0
    img += rng.normal(0.0, 1500.0, img.shape)
    return ((img - 30000.0) / 1000.0).astype(np.float32)


def _f32_image(h, w, seed=0):
    """Three differently shaped channels of signed fractional values: the colour suite's pattern, not rounded, shifted by -128 and
    divided by 4 (about -32 .. +28 with noise sigma 1.5; at H_VAL = 30 / 4 its graph is the colour suite's). float32 [h, w, 3]."""
    img = np.ascontiguousarray((_colour_pattern(h, w, seed) - 128.0) / 4.0, dtype=np.float32)
    assert img.min() < -5.0 and img.max() > 5.0 and np.any(img != np.rint(img))      # negative and non-integer values
    return img


def _u8_image(h, w, seed=0):
    """The colour suite's 8-bit test image."""
    return np.clip(np.rint(_colour_pattern(h, w, seed)), 0, 255).astype(np.uint8)


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _route(info):
    return info["nystroem_path"], info["matvec_path"], info["filter_fused"]


def _dev(ctx, img):
    return torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)


def _whole(ctx, img, opt, capture=False):
    """(z float32 numpy [H, W, 3], info) of the float colour call."""
    z, info = ctx.image_processing_rgbf32(_dev(ctx, np.asarray(img, dtype=np.float32)), opt, capture=capture)
    return z.cpu().numpy(), info


def _whole8(ctx, rgb, opt, capture=False):
    out, zf, info = ctx.image_processing_rgb(_dev(ctx, np.asarray(rgb, dtype=np.uint8)), opt, want_float=True, capture=capture)
    return out.cpu().numpy(), zf.cpu().numpy(), info


def _residuals_ok(LA, phi_A, lam):
    for j in range(lam.size):   # the residual the eigen-solve's own stopping rule allows
        v = phi_A[:, j] / np.linalg.norm(phi_A[:, j])
        assert np.linalg.norm(LA @ v - lam[j] * v) <= 2e-2 * max(lam[j], 1e-3), (j, lam[j])


def _read_rows(ctx, mat, rows, m):
    """Rows `rows` of a dense device matrix, the first m columns."""
    out = np.empty((len(rows), m))
    full = np.empty((1, mat.ld), dtype=np.float32)
    for k, r in enumerate(rows):
        glf._lib.glf_memcpy_d2h(ctx._ctx, full.ctypes.data_as(glf.C.c_void_p), glf.C.c_void_p(mat.data + 4 * int(r) * mat.ld),
                                glf.C.c_size_t(full.nbytes))
        out[k] = full[0, :m]
    return out


# ---- the stages and the whole path against fp64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(48, 40), (97, 61), (64, 64)])
def test_stages_against_numpy(w, h):
    img = _f32_image(h, w, seed=w)
    idx = glf.Sampling(w, h, 120)
    m = 8
    with glf.Context(0) as ctx:
        K_A, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=True, kernel=K96, h_loc=H_LOC, h_val=H_VAL)
        ka, deg = ctx.mat_to_numpy(K_A).astype(np.float64), ctx.degree_of(K_B)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        vecs, vals, _ = ctx.InversePowerIteration(L_A, m, epsilon=1e-3)
        lam = ctx.mat_to_numpy(vals).astype(np.float64)
        phi_A = ctx.mat_to_numpy(vecs)[:len(idx)].astype(np.float64)
        pinv = ctx.InverseDiagMat(vals)
        phi_sf = ctx.Nystroem(L_B, vecs, pinv)
        phi_r = ctx.Permutation(phi_sf, idx)
        phi = ctx.mat_to_numpy(phi_r).astype(np.float64)
        ctx.destroy(K_A, K_B, L_A, vecs, vals, pinv, phi_sf, phi_r)
    KA, D, alpha_ref, LA = ref.laplacian(img, idx, H_LOC, H_VAL)
    print("rgbf32 stages %dx%d: max |K_A - ref| %.2e, max |D_A - ref| / max D %.2e, alpha rel %.2e" %
          (w, h, float(np.abs(ka - KA).max()), float(np.abs(deg - D).max() / D.max()), abs(alpha - alpha_ref) / alpha_ref))
    assert float(np.abs(ka - KA).max()) <= 1e-6 * float(np.abs(KA).max())
    assert float(np.abs(deg - D).max()) <= 1e-6 * float(D.max())
    assert abs(alpha - alpha_ref) <= 1e-6 * alpha_ref
    _residuals_ok(LA, phi_A, lam)
    want = ref.phi_rows(img, idx, np.arange(w * h), phi_A, lam, alpha, H_LOC, H_VAL)
    print("rgbf32 stages %dx%d: Phi rel-L2 %.2e" % (w, h, _rel(phi, want)))
    assert _rel(phi, want) <= 1e-5


@pytest.mark.parametrize("sampling", [glf.SAMPLING_UNIFORM, glf.SAMPLING_RANDOM])
@pytest.mark.parametrize("mode", list(MODES))
def test_whole_path_against_numpy(mode, sampling):
    """Every filter mode on both samplers, from the run's own by-products (glf_image_processing_rgbf32_capture)."""
    w, h, ns, m = 61, 47, 100, 8
    img = _f32_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], sampling=sampling, h_val=H_VAL)
    idx = glf.Sampling(w, h, ns) if sampling == glf.SAMPLING_UNIFORM else glf.RandomSampling(w, h, ns, seed=int(opt.sampling_seed))
    with glf.Context(0) as ctx:
        z, info = _whole(ctx, img, opt, capture=True)
        cap = info["capture"]
        phi_A = cap["phi_A"].cpu().numpy()[:len(idx), :m].astype(np.float64)
        phi = cap["phi"].cpu().numpy()[:, :m].astype(np.float64)
    assert z.dtype == np.float32 and z.shape == (h, w, 3)
    assert _route(info) == (0, 0, 0)
    assert info["contraction"] == glf.CONTRACT_F32_MFMA
    assert info["p"] == len(idx) and info["m"] == m
    assert 0 < info["degree_evaluated"] <= float(len(idx)) * w * h
    _, D, alpha, LA = ref.laplacian(img, idx, H_LOC, H_VAL)
    np.testing.assert_allclose(cap["degree"], D, rtol=1e-6)
    assert abs(info["alpha"] - alpha) <= 1e-6 * alpha
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    _residuals_ok(LA, phi_A, lam)
    want_phi = ref.phi_rows(img, idx, np.arange(w * h), phi_A, lam, info["alpha"], H_LOC, H_VAL)
    assert _rel(phi, want_phi) <= 1e-5
    ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
    x = img.reshape(-1, 3).T.astype(np.float64)
    corr = z.reshape(-1, 3).T.astype(np.float64) - (1.0 - ysub) * x
    want = ref.corrections(img, phi, lam, MODES[mode], float(opt.gain))
    for k in range(3):
        err = _rel(corr[k], want[k])
        print("rgbf32 whole path %s sampling %d channel %d: rel-L2 of the correction %.2e" % (mode, sampling, k, err))
        assert err <= 1e-5, (k, err)


# ---- the same template source on the same f32 values: the 8-bit colour call's bits -----------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_equals_the_u8_colour_call_on_integer_values(mode):
    """x = an 8-bit colour image: the float call on x.astype(float32) and the 8-bit call on x compare the same f32 values in the same
    operation order -- D_A, the eigenvalues, the iteration count and the route are equal, and z (interleaved) is the 8-bit call's
    planar float z, channel by channel, bit for bit."""
    w, h, ns, m = 61, 47, 100, 8
    x = _u8_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], h_val=H_VAL8)
    with glf.Context(0) as ctx:
        z, info = _whole(ctx, x.astype(np.float32), opt, capture=True)
        _, zf8, info8 = _whole8(ctx, x, opt, capture=True)
    d = float(np.abs(z.transpose(2, 0, 1).astype(np.float64) - zf8).max())
    print("rgbf32 against u8 colour (%s): max |z - zf8| %.3e, max rel eigenvalue difference %.3e" %
          (mode, d, float(np.abs(np.asarray(info["eigvals"]) / np.asarray(info8["eigvals"]) - 1.0).max())))
    np.testing.assert_array_equal(info["capture"]["degree"], info8["capture"]["degree"])
    np.testing.assert_array_equal(info["eigvals"], info8["eigvals"])
    assert info["outer_its"] == info8["outer_its"] and _route(info) == _route(info8)
    for k in range(3):
        np.testing.assert_array_equal(_bits(z[:, :, k]), _bits(zf8[k]), err_msg="channel %d" % k)


@pytest.mark.parametrize("mode", list(MODES))
def test_power_of_two_scale_covariance(mode):
    """x 2^-8 (values in [0, 1)) at h_val 2^-8: s_val scales by exactly 2^16, dist2 by exactly 2^-16, and every sum downstream is
    linear in x, so the eigenvalues and alpha are those of the 8-bit colour call on x and z = 2^-8 zf_rgb, bit for bit. (The 8-bit
    entry point cannot take this image: every pixel rounds to 0.)"""
    w, h, ns, m = 61, 47, 100, 8
    x = _u8_image(h, w, seed=3)
    s = np.float32(2.0 ** -8)
    xs = x.astype(np.float32) * s
    assert xs.max() < 1.0 and np.array_equal(xs.astype(np.float64) * 256.0, x.astype(np.float64))      # the scaling is exact
    kw = dict(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode])
    with glf.Context(0) as ctx:
        _, zf8, info8 = _whole8(ctx, x, glf.default_options(h_val=H_VAL8, **kw))
        zs, infos = _whole(ctx, xs, glf.default_options(h_val=H_VAL8 * 2.0 ** -8, **kw))
    np.testing.assert_array_equal(infos["eigvals"], info8["eigvals"])
    assert infos["alpha"] == info8["alpha"] and infos["outer_its"] == info8["outer_its"]
    want = zf8 * s
    assert np.array_equal(want.astype(np.float64) * 256.0, zf8.astype(np.float64))                      # (no underflow in the product)
    for k in range(3):
        np.testing.assert_array_equal(_bits(zs[:, :, k]), _bits(want[k]), err_msg="channel %d" % k)


def test_grey_replicated_is_the_float_grey_graph():
    """R = G = B = v (a float grey image) at h_val sqrt(3) is the float grey graph at h_val: D_A within 1e-6, the eigenvalues within
    1e-5, each channel's correction within 1e-5 relative L2 of the float grey call's (the bounds of the 8-bit colour suite's test)."""
    w, h, ns, m = 80, 64, 120, 8
    hv = 30.0 * 257.0 / 1000.0
    v = _grey_f32_image(h, w, seed=5)
    rgb = np.repeat(v[:, :, None], 3, axis=2).copy()
    idx = glf.Sampling(w, h, ns)
    for mode in ("reference", "smooth"):
        with glf.Context(0) as ctx:
            opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.05, filter_mode=MODES[mode], h_val=hv)
            zg, info_g = ctx.image_processing_f32(_dev(ctx, v), opt)
            zg = zg.cpu().numpy().astype(np.float64)
            opt_c = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.05, filter_mode=MODES[mode], h_val=hv * math.sqrt(3.0))
            zc, info_c = _whole(ctx, rgb, opt_c)
            _, KB_c = ctx.ComputeAffinityMatrices(_dev(ctx, rgb), idx, want_KA=False, kernel=K96, h_val=hv * math.sqrt(3.0))
            _, KB_g = ctx.ComputeAffinityMatrices(_dev(ctx, v), idx, want_KA=False, kernel=glf.KERNEL_BILATERAL_F32, h_val=hv)
            deg_c, deg_g = ctx.degree_of(KB_c), ctx.degree_of(KB_g)
            ctx.destroy(KB_c, KB_g)
        np.testing.assert_allclose(deg_c, deg_g, rtol=1e-6)
        np.testing.assert_allclose(info_c["eigvals"], info_g["eigvals"], rtol=1e-5)
        ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
        cg = zg - (1.0 - ysub) * v
        for k in range(3):
            ck = zc[:, :, k].astype(np.float64) - (1.0 - ysub) * v
            print("rgbf32 grey replicated %s channel %d: rel-L2 of the correction against the float grey call %.2e" % (mode, k, _rel(ck, cg)))
            assert _rel(ck, cg) <= 1e-5, (mode, k, _rel(ck, cg))


# ---- the band form behind PIX_BAND -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,ns", [(128, 96, 150), (77, 200, 60)])
def test_nystroem_stage_band_against_numpy_and_entrywise(w, h, ns):
    m = 8
    img = _f32_image(h, w, seed=w)
    idx = glf.Sampling(w, h, ns)
    _, _, _, LA = ref.laplacian(img, idx, H_LOC, H_VAL)
    vals, vecs = np.linalg.eigh(LA)                      # LAPACK eigenpairs of the fp64 L_A, the m smallest
    lam, phi_A = vals[:m], vecs[:, :m]
    got = {}
    with glf.Context(0) as ctx:
        _, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=False, kernel=K96, h_loc=H_LOC, h_val=H_VAL)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        d_vecs, d_vals = ctx.dense_from_numpy(phi_A), ctx.diag_from_numpy(lam)
        pinv = ctx.InverseDiagMat(d_vals)
        for key in ("band", "entrywise"):
            ctx.reset_tuning()
            if key == "band":
                ctx.set_tuning(PIX_BAND="1", NYS_PATH="band")
            phi_sf = ctx.Nystroem(L_B, d_vecs, pinv)
            phi_r = ctx.Permutation(phi_sf, idx)
            got[key] = ctx.mat_to_numpy(phi_r).astype(np.float64)
            ctx.destroy(phi_sf, phi_r)
        ctx.destroy(K_B, L_A, d_vecs, d_vals, pinv)
    want = ref.phi_rows(img, idx, np.arange(w * h), phi_A, lam, alpha, H_LOC, H_VAL)
    e_band, e_entry = _rel(got["band"], want), _rel(got["entrywise"], want)
    d = float(np.abs(got["band"] - got["entrywise"]).max() / np.abs(got["entrywise"]).max())
    print("rgbf32 %dx%d: Phi rel-L2 band %.2e entrywise %.2e, max |band - entrywise| / max |Phi| %.2e" % (w, h, e_band, e_entry, d))
    assert e_band <= 1e-5 and e_entry <= 1e-5
    assert d <= 2e-5                                     # (forms of different arithmetic: the suite's bound between them)
    assert np.any(got["band"] != got["entrywise"])      # (another arithmetic: the key did select another kernel)


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_path_small_forced_band(mode):
    """Route (4, 4, 0): the eigenvalues within 1e-5 of the key-off run's, Phi and the corrections within 1e-5 of numpy."""
    w, h, ns, m = 96, 80, 120, 8
    img = _f32_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], h_val=H_VAL)
    idx = glf.Sampling(w, h, ns)
    with glf.Context(0) as ctx:
        _, info_off = _whole(ctx, img, opt)
        ctx.set_tuning(PIX_BAND="1", NYS_PATH="band", MV_PATH="band")
        z, info = _whole(ctx, img, opt, capture=True)
        cap = info["capture"]
        phi_A = cap["phi_A"].cpu().numpy()[:len(idx), :m].astype(np.float64)
        phi = cap["phi"].cpu().numpy()[:, :m].astype(np.float64)
    assert _route(info_off) == (0, 0, 0) and _route(info) == (4, 4, 0)
    assert info["contraction"] == glf.CONTRACT_F16_SPLIT
    assert info["p"] == len(idx) and info["m"] == m and info["nystroem_evaluated"] > 0
    _, D, alpha, LA = ref.laplacian(img, idx, H_LOC, H_VAL)
    np.testing.assert_allclose(cap["degree"], D, rtol=1e-6)
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    _residuals_ok(LA, phi_A, lam)
    np.testing.assert_allclose(lam, info_off["eigvals"], rtol=1e-5)
    want_phi = ref.phi_rows(img, idx, np.arange(w * h), phi_A, lam, info["alpha"], H_LOC, H_VAL)
    e_phi = _rel(phi, want_phi)
    ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
    x = img.reshape(-1, 3).T.astype(np.float64)
    corr = z.reshape(-1, 3).T.astype(np.float64) - (1.0 - ysub) * x
    want = ref.corrections(img, phi, lam, MODES[mode], float(opt.gain))
    errs = [_rel(corr[k], want[k]) for k in range(3)]
    print("rgbf32 band %s: Phi rel-L2 %.2e, correction rel-L2 %.2e %.2e %.2e" % (mode, e_phi, errs[0], errs[1], errs[2]))
    assert e_phi <= 1e-5
    assert max(errs) <= 1e-5, errs


@pytest.mark.parametrize("mode", list(MODES))
def test_band_route_equals_the_u8_colour_band_route_on_integer_values(mode):
    """x = an 8-bit colour image at 96 x 80, the same key and the same route (4, 4, 0) for both calls: the float call's band kernels
    compare the same f32 values in the same operation order as the 8-bit colour call's -- D_A, the eigenvalues and z bit for bit."""
    w, h, ns, m = 96, 80, 120, 8
    x = _u8_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], h_val=H_VAL8)
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1", NYS_PATH="band", MV_PATH="band")
        z, info = _whole(ctx, x.astype(np.float32), opt, capture=True)
        _, zf8, info8 = _whole8(ctx, x, opt, capture=True)
    assert _route(info) == (4, 4, 0) and _route(info8) == (4, 4, 0)
    np.testing.assert_array_equal(info["capture"]["degree"], info8["capture"]["degree"])
    np.testing.assert_array_equal(info["eigvals"], info8["eigvals"])
    assert info["outer_its"] == info8["outer_its"] and info["nystroem_evaluated"] == info8["nystroem_evaluated"]
    for k in range(3):
        np.testing.assert_array_equal(_bits(z[:, :, k]), _bits(zf8[k]), err_msg="channel %d" % k)


# 1056 x 256 at h_loc = 10 (radius 53 px): wide enough, and the band narrow enough, for the automatic band form (the key alone takes
# it there), so a decline is the condition's doing and the exact-zero skips have something to skip
DECL_W, DECL_H = 1056, 256
DECL_KW = dict(num_samples=600, num_eigvals=8, epsilon=0.05, h_loc=10.0, h_val=H_VAL)


@pytest.mark.parametrize("case,okw", [("random-sampler", dict(sampling=glf.SAMPLING_RANDOM)), ("m-99", dict(num_eigvals=99))])
def test_declines_are_the_entrywise_route_bit_for_bit(case, okw):
    img = _f32_image(DECL_H, DECL_W, seed=6)
    kw = dict(DECL_KW)
    kw.update(okw)
    opt = glf.default_options(**kw)
    res = []
    for key in (None, "1"):
        with glf.Context(0) as ctx:
            ctx.set_tuning(PIX_BAND=key)
            res.append(_whole(ctx, img, opt))
    (z0, info0), (z1, info1) = res
    assert _route(info0) == (0, 0, 0) and _route(info1) == (0, 0, 0), case
    assert info1["contraction"] == glf.CONTRACT_F32_MFMA
    np.testing.assert_array_equal(_bits(z1), _bits(z0))
    np.testing.assert_array_equal(info1["eigvals"], info0["eigvals"])


def test_key_alone_takes_the_band_form_and_noskip_is_bit_identical():
    img = _f32_image(DECL_H, DECL_W, seed=6)
    opt = glf.default_options(**DECL_KW)
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1")
        _, info_a = _whole(ctx, img, opt)
        ctx.set_tuning(MV_PATH="band")
        z_b, info_b = _whole(ctx, img, opt)
        ctx.set_tuning(BAND_NOSKIP="1")
        z_c, info_c = _whole(ctx, img, opt)
    assert _route(info_a) == (4, 0, 0) and info_a["contraction"] == glf.CONTRACT_F16_SPLIT
    assert _route(info_b) == (4, 4, 0) and _route(info_c) == (4, 4, 0)
    print("rgbf32 band: nystroem_evaluated %.4e with the skips, %.4e without" % (info_b["nystroem_evaluated"], info_c["nystroem_evaluated"]))
    np.testing.assert_array_equal(_bits(z_c), _bits(z_b))
    np.testing.assert_array_equal(info_c["eigvals"], info_b["eigvals"])
    assert info_c["nystroem_evaluated"] > info_b["nystroem_evaluated"]


# ---- joint filtering ------------------------------------------------------------------------------------------------------------------------

def _test_planes(h, w, seed=0):
    """Signed noise; a smooth positive plane; a depth-like plane in metres: a disc 0.4 above a floor of 1.0 under sigma = 0.015."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 40.0, (h, w))
    b = np.linspace(-3.0, 7.0, h * w).reshape(h, w) ** 2
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    depth = 1.0 + 0.4 * disc + np.random.default_rng(seed + 100).normal(0.0, 0.015, (h, w))
    return np.stack([a, b, depth]).astype(np.float32)


def _signals(ctx, img, sig, opt):
    d_sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32)).to(ctx.device)
    z, so, info = ctx.image_processing_rgbf32_signals(_dev(ctx, img), d_sig, opt)
    return z.cpu().numpy(), so.cpu().numpy(), info


def _assert_guide_equal(z, info, z1, info1, what=""):
    np.testing.assert_array_equal(_bits(z), _bits(z1), err_msg=what)
    np.testing.assert_array_equal(info["eigvals"], info1["eigvals"], err_msg=what)
    for key, v in info1.items():
        if "ms" not in key and key not in ("eigvals", "capture"):
            assert info[key] == v, (what, key, info[key], v)


@pytest.mark.parametrize("band", [False, True])
@pytest.mark.parametrize("sampling", [glf.SAMPLING_UNIFORM, glf.SAMPLING_RANDOM])
def test_guide_bit_identical_to_plain_call(sampling, band):
    """The guide's z, eigenvalues and every non-timing statistic, key off (61 x 47) and on (96 x 80: the band suite's small shape;
    the grid sampler with the band routes forced, the random sampler with the key alone, where the band form declines)."""
    w, h, ns, m = (96, 80, 120, 8) if band else (61, 47, 100, 8)
    img, sig = _f32_image(h, w, seed=3), _test_planes(h, w)
    with glf.Context(0) as ctx:
        if band:
            ctx.set_tuning(PIX_BAND="1")
            if sampling == glf.SAMPLING_UNIFORM:
                ctx.set_tuning(NYS_PATH="band", MV_PATH="band")
        for name, mode in MODES.items():
            opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=mode, sampling=sampling, h_val=H_VAL)
            z1, info1 = _whole(ctx, img, opt)
            z, so, info = _signals(ctx, img, sig, opt)
            _assert_guide_equal(z, info, z1, info1, name)
            assert _route(info) == ((4, 4, 0) if band and sampling == glf.SAMPLING_UNIFORM else (0, 0, 0))
            assert np.isfinite(so).all(), name


@pytest.mark.parametrize("mode", list(MODES))
def test_planes_against_fp64(mode):
    """Plane s comes out as (1 - ysub) s + gain Phi w_s, w_s = f(Pi) Phi^T s in fp64 on the run's own Phi and eigenvalues: within
    1e-5 relative L2 of the correction. The correction is read back from the output, which the API stores in f32; numpy's output goes
    through the same storage before the corrections are compared (the float grey suite's rule: the bound is unchanged, and every
    error of the route still shows). The last plane is the guide's first channel and must come out as that channel's z to within one
    ulp of the float output."""
    w, h, ns, m = 61, 47, 100, 8
    img = _f32_image(h, w, seed=3)
    sig = np.concatenate([_test_planes(h, w), img[None, :, :, 0]])
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], h_val=H_VAL)
    with glf.Context(0) as ctx:
        z1, info1 = _whole(ctx, img, opt, capture=True)
        phi = info1["capture"]["phi"].cpu().numpy()[:, :m].astype(np.float64)
        del info1["capture"]
        z, so, info = _signals(ctx, img, sig, opt)
    _assert_guide_equal(z, info, z1, info1, mode)
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
    g = float(opt.gain) if MODES[mode] == glf.FILTER_REFERENCE else 1.0
    for k in range(sig.shape[0]):
        s = sig[k].reshape(-1).astype(np.float64)
        want = g * (phi @ ref.weights(phi, lam, MODES[mode], phi.T @ s))
        want_stored = ((1.0 - ysub) * s + want).astype(np.float32).astype(np.float64) - (1.0 - ysub) * s
        got = so[k].reshape(-1).astype(np.float64) - (1.0 - ysub) * s
        err = float(np.linalg.norm(got - want_stored) / np.linalg.norm(want))
        print("rgbf32 %s plane %d: rel-L2 of the correction %.2e (against numpy's before its f32 storage: %.2e)" % (mode, k, err, _rel(got, want)))
        assert err <= 1e-5, (k, err)
    assert _rel(so[-1], z[:, :, 0]) <= 2.0 ** -23          # (both are one f32 rounding of the same fp64 sum, formed by two statements)


def test_planes_independent_of_their_neighbours():
    w, h, ns, m = 61, 47, 100, 8
    img = _f32_image(h, w, seed=3)
    s1, s2, depth = _test_planes(h, w, 7)
    s4 = img[:, :, 1].copy()
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, h_val=H_VAL)
    with glf.Context(0) as ctx:
        four = _signals(ctx, img, np.stack([s1, s2, depth, s4]), opt)[1]
        two = _signals(ctx, img, np.stack([s2, s1]), opt)[1]
        ones = [_signals(ctx, img, s[None], opt)[1][0] for s in (s1, s2, depth, s4)]
    for k in range(4):
        np.testing.assert_array_equal(_bits(four[k]), _bits(ones[k]), err_msg="plane %d of 4 against alone" % k)
    np.testing.assert_array_equal(_bits(two[0]), _bits(ones[1]))
    np.testing.assert_array_equal(_bits(two[1]), _bits(ones[0]))


# ---- refusals and bookkeeping ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channel", [0, 1, 2])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_is_refused_and_nothing_is_written(bad, channel):
    w, h, ns = 61, 47, 100
    img = _f32_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=8, epsilon=0.05, h_val=H_VAL)
    idx = set(int(i) for i in glf.Sampling(w, h, ns))
    px = next(i for i in range(w * h - 1, 0, -1) if i not in idx)       # a pixel that is not a sample
    poisoned = img.copy()
    poisoned.reshape(-1, 3)[px, channel] = bad
    with glf.Context(0) as ctx:
        z0, info0 = _whole(ctx, img, opt)
        out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device=ctx.device)
        sig = torch.zeros((1, h, w), dtype=torch.float32, device=ctx.device)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_rgbf32(_dev(ctx, poisoned), opt, out=out)
        assert e.value.status == glf.ERR_INVALID and ("NaN" in str(e.value) or "Inf" in str(e.value))
        assert bool((out == 7.0).all())
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_rgbf32_signals(_dev(ctx, poisoned), sig, opt)
        assert e.value.status == glf.ERR_INVALID
        with pytest.raises(glf.GlfError) as e:
            ctx.ComputeAffinityMatrices(_dev(ctx, poisoned), glf.Sampling(w, h, ns), want_KA=False, kernel=K96, h_loc=H_LOC, h_val=H_VAL)
        assert e.value.status == glf.ERR_INVALID
        z1, info1 = _whole(ctx, img, opt)                                # the context still works, and gives the same bits
    np.testing.assert_array_equal(_bits(z1), _bits(z0))
    np.testing.assert_array_equal(info1["eigvals"], info0["eigvals"])


def test_invalid_and_unsupported_with_a_live_context():
    w, h = 40, 32
    img = _f32_image(h, w, seed=1)
    with glf.Context(0) as ctx:
        d = _dev(ctx, img)
        sig = torch.zeros((1, h, w), dtype=torch.float32, device=ctx.device)
        for kernel in (glf.KERNEL_PHOTOMETRIC, glf.KERNEL_SPATIAL, glf.KERNEL_NLM, glf.KERNEL_BILATERAL_RGB, glf.KERNEL_BILATERAL_U16,
                       glf.KERNEL_BILATERAL_F32):
            with pytest.raises(glf.GlfError) as e:
                ctx.image_processing_rgbf32(d, glf.default_options(num_samples=30, num_eigvals=4, kernel=kernel))
            assert e.value.status == glf.ERR_UNSUPPORTED, kernel
            with pytest.raises(glf.GlfError) as e:
                ctx.image_processing_rgbf32_signals(d, sig, glf.default_options(num_samples=30, num_eigvals=4, kernel=kernel))
            assert e.value.status == glf.ERR_UNSUPPORTED, kernel
        k7 = glf.default_options(num_samples=30, num_eigvals=4, kernel=K96, h_val=H_VAL)
        g = ctx.to_device(glf.synth_image(w, h, seed=1))
        with pytest.raises(glf.GlfError) as e:           # the other entry points never read their pixels as float triples
            ctx.image_processing(g, k7)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_signals(g, sig, k7)
        assert e.value.status == glf.ERR_UNSUPPORTED
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=ctx.device)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_rgb(rgb, k7)
        assert e.value.status == glf.ERR_UNSUPPORTED
        u16 = torch.zeros((h, w), dtype=torch.int16, device=ctx.device).view(torch.uint16)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_u16(u16, k7)
        assert e.value.status == glf.ERR_UNSUPPORTED
        f32 = torch.zeros((h, w), dtype=torch.float32, device=ctx.device)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_f32(f32, k7)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_f32_signals(f32, sig, k7)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:           # more than 256 eigenpairs
            ctx.image_processing_rgbf32(d, glf.default_options(num_samples=400, num_eigvals=300, h_val=H_VAL))
        assert e.value.status == glf.ERR_UNSUPPORTED
        C = glf.C
        for nsig in (0, 5):                              # nsig outside 1 .. 4
            out = torch.zeros((h, w, 3), dtype=torch.float32, device=ctx.device)
            planes = torch.zeros((5, h, w), dtype=torch.float32, device=ctx.device)
            rc = glf._lib.glf_image_processing_rgbf32_signals(ctx._ctx, None, C.c_void_p(d.data_ptr()), w, h, C.c_int(nsig),
                                                              C.c_void_p(planes.data_ptr()), C.c_void_p(planes.data_ptr()),
                                                              C.c_void_p(out.data_ptr()), None, None)
            assert rc == glf.ERR_INVALID, nsig
        out = torch.zeros((h, w, 3), dtype=torch.float32, device=ctx.device)
        rc = glf._lib.glf_image_processing_rgbf32(ctx._ctx, None, None, w, h, C.c_void_p(out.data_ptr()), None, None)
        assert rc == glf.ERR_INVALID
        rc = glf._lib.glf_image_processing_rgbf32(ctx._ctx, None, C.c_void_p(d.data_ptr()), w, h, None, None, None)
        assert rc == glf.ERR_INVALID
        z, info = ctx.image_processing_rgbf32(d, k7)     # kernel 7 is the format's own id; the context still works
        assert z.shape == (h, w, 3) and z.dtype == torch.float32 and info["m"] == 4 and bool(torch.isfinite(z).all())


def test_grey_rgb_and_f32_calls_after_a_float_colour_call_are_unchanged():
    g = glf.synth_image(96, 80, seed=4)
    x8 = _u8_image(80, 96, seed=2)
    v = _grey_f32_image(80, 96, seed=2)
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05)
    opt32 = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=30.0 * 257.0 / 1000.0)
    with glf.Context(0) as fresh:
        out0, zf0, _ = fresh.image_processing(fresh.to_device(g), opt, want_float=True)
        out0, zf0 = out0.cpu().numpy(), zf0.cpu().numpy()
    with glf.Context(0) as fresh:
        o8, z8, i8 = _whole8(fresh, x8, opt)
    with glf.Context(0) as fresh:
        z32, i32 = fresh.image_processing_f32(_dev(fresh, v), opt32)
        z32 = z32.cpu().numpy()
    with glf.Context(0) as ctx:
        _whole(ctx, _f32_image(80, 96, seed=2), glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=H_VAL))
        out1, zf1, _ = ctx.image_processing(ctx.to_device(g), opt, want_float=True)
        np.testing.assert_array_equal(out1.cpu().numpy(), out0)
        np.testing.assert_array_equal(_bits(zf1.cpu().numpy()), _bits(zf0))
        o8b, z8b, i8b = _whole8(ctx, x8, opt)
        z32b, i32b = ctx.image_processing_f32(_dev(ctx, v), opt32)
        z32b = z32b.cpu().numpy()
    np.testing.assert_array_equal(o8b, o8)
    np.testing.assert_array_equal(_bits(z8b), _bits(z8))
    np.testing.assert_array_equal(i8b["eigvals"], i8["eigvals"])
    np.testing.assert_array_equal(_bits(z32b), _bits(z32))
    np.testing.assert_array_equal(i32b["eigvals"], i32["eigvals"])


@pytest.mark.parametrize("band", [False, True])
def test_debug_pool_rgbf32_run(monkeypatch, band):
    """GLF_POOL_DEBUG=1 on each route, p no multiple of 64 (the value block behind the padded records, the wider LDS stage, the
    three-plane sample values of the band form)."""
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    img = _f32_image(72, 90, seed=8)
    sig = _test_planes(72, 90, 8)
    for mode in ("reference", "sharpen"):
        opt = glf.default_options(num_samples=80, num_eigvals=8, epsilon=0.05, filter_mode=MODES[mode], h_val=H_VAL)
        with glf.Context(0) as ctx:
            if band:
                ctx.set_tuning(PIX_BAND="1", NYS_PATH="band", MV_PATH="band")
            z, info = _whole(ctx, img, opt)
            z2, so, _ = _signals(ctx, img, sig, opt)
            assert ctx.debug_violations() == 0
        assert _route(info) == ((4, 4, 0) if band else (0, 0, 0)) and info["p"] % 64 != 0
        assert np.isfinite(z).all() and np.isfinite(so).all() and np.isfinite(info["eigvals"]).all()
        np.testing.assert_array_equal(_bits(z2), _bits(z))


# ---- 1024 x 256: sampled rows of the stage path --------------------------------------------------------------------------------------------

def test_1024_wide_sampled_rows_against_numpy():
    """At 1024 x 256 with h_loc = 10 (the width from which the key alone takes the band form) the stage path's Phi rows of sampled
    pixels against numpy's extension of its Phi_A, with the PIX_BAND key off and on (the same Phi_A and eigenvalues through both
    Nystroem kernels)."""
    w, h, m, h_loc = 1024, 256, 8, 10.0
    img = _f32_image(h, w, seed=11)
    idx = glf.Sampling(w, h, 640)
    with glf.Context(0) as ctx:
        _, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=False, kernel=K96, h_loc=h_loc, h_val=H_VAL)
        deg = ctx.degree_of(K_B)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        vecs, vals, _ = ctx.InversePowerIteration(L_A, m, epsilon=0.1)
        lam = ctx.mat_to_numpy(vals).astype(np.float64)
        phi_A = ctx.mat_to_numpy(vecs)[:len(idx)].astype(np.float64)
        pinv = ctx.InverseDiagMat(vals)
        pix = np.sort(np.random.default_rng(0).choice(w * h, 48, replace=False))
        rows = {}
        for key in (None, "1"):
            ctx.set_tuning(PIX_BAND=key)
            phi_sf = ctx.Nystroem(L_B, vecs, pinv)
            phi_r = ctx.Permutation(phi_sf, idx)
            rows[key] = _read_rows(ctx, phi_r, pix, m)
            ctx.destroy(phi_sf, phi_r)
        ctx.destroy(K_B, L_A, vecs, vals, pinv)
    sel = np.arange(0, len(idx), max(1, len(idx) // 24))
    np.testing.assert_allclose(deg[sel], ref.degree(img, idx[sel], h_loc, H_VAL, chunk=1 << 16), rtol=1e-6)
    want = ref.phi_rows(img, idx, pix, phi_A, lam, alpha, h_loc, H_VAL)
    print("rgbf32 1024 x 256 stage path: Phi rows rel-L2 %.2e (key off), %.2e (key on)" % (_rel(rows[None], want), _rel(rows["1"], want)))
    assert _rel(rows[None], want) <= 1e-5 and _rel(rows["1"], want) <= 1e-5
    assert np.any(rows[None] != rows["1"])                  # (the key selected the band kernel: another arithmetic)
