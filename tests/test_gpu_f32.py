"""32-bit float greyscale filtering (GLF_KERNEL_BILATERAL_F32, glf_image_processing_f32): the graph is built from float values in
the image's own units (negative and fractional included) and the image goes through its filter; the output is the float z.

Checked against the fp64 numpy restatement in tests/u16_ref.py, which is format-neutral (it casts the image to float64) and sees the
float32-rounded image the GPU sees: the stage kernels, the whole path in every filter mode on both samplers, bit-equality with the
16-bit call on integer values, exact covariance under a power-of-two scale, an edge below one 16-bit level, the band form behind
PIX_BAND, joint filtering, the refusals (NaN / Inf, kernel mismatches, m > 256), the context's bookkeeping and 2048^2 sampled rows.

Tolerances: those of tests/test_gpu_u16.py, because the arithmetic is the same chain. v_i - v_j of two floats is rounded once (2^-24
relative), its square once more, so the exponent carries ~3 x 2^-24 and an entry moves by at most K t ln2 x 1.8e-7 <= 7e-8 (x e^-x
<= 1/e), under the 1e-7 per entry the 16-bit analysis allows: K_A and D_A within 1e-6 of their maxima, alpha within 1e-6, eigenpair
residuals <= 2e-2 max(lam, 1e-3) against the fp64 L_A, Phi and the corrections within 1e-5 relative L2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import u16_ref as ref  # noqa: E402

MODES = {"reference": glf.FILTER_REFERENCE, "poc": glf.FILTER_POC, "smooth": glf.FILTER_SMOOTH, "sharpen": glf.FILTER_SHARPEN}
H_LOC, H_VAL = 40.0, 30.0 * 257.0 / 1000.0
H_VAL16 = 30.0 * 257.0
K32 = glf.KERNEL_BILATERAL_F32


def _pattern(h, w, seed=0):
    """The pattern of the 16-bit suite's test image before it is rounded: smooth ramps, a disc of another level and noise."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 9000.0 + 30000.0 * c / max(1, w - 1) + 12000.0 * np.sin(r / 9.0)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    img[disc] = 58000.0
    img += rng.normal(0.0, 1500.0, img.shape)
    return img


def _u16_image(h, w, seed=0):
    return np.clip(np.rint(_pattern(h, w, seed)), 0, 65535).astype(np.uint16)


def _f32_image(h, w, seed=0):
    """Signed fractional values: about -35 .. +34 with noise sigma 1.5."""
    return ((_pattern(h, w, seed) - 30000.0) / 1000.0).astype(np.float32)


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _route(info):
    return info["nystroem_path"], info["matvec_path"], info["filter_fused"]


def _dev(ctx, img):
    return torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)


def _whole(ctx, img, opt, capture=False):
    """(z float32 numpy, info) of the float call."""
    z, info = ctx.image_processing_f32(_dev(ctx, np.asarray(img, dtype=np.float32)), opt, capture=capture)
    return z.cpu().numpy(), info


def _whole16(ctx, img, opt, capture=False):
    out, zf, info = ctx.image_processing_u16(_dev(ctx, np.asarray(img, dtype=np.uint16)), opt, want_float=True, capture=capture)
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
    assert img.min() < -5.0 and img.max() > 5.0 and np.any(img != np.rint(img))
    idx = glf.Sampling(w, h, 120)
    m = 8
    with glf.Context(0) as ctx:
        K_A, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=True, kernel=K32, h_loc=H_LOC, h_val=H_VAL)
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
    print("f32 stages %dx%d: max |K_A - ref| %.2e, max |D_A - ref| / max D %.2e, alpha rel %.2e" %
          (w, h, float(np.abs(ka - KA).max()), float(np.abs(deg - D).max() / D.max()), abs(alpha - alpha_ref) / alpha_ref))
    assert float(np.abs(ka - KA).max()) <= 1e-6 * float(np.abs(KA).max())
    assert float(np.abs(deg - D).max()) <= 1e-6 * float(D.max())
    assert abs(alpha - alpha_ref) <= 1e-6 * alpha_ref
    _residuals_ok(LA, phi_A, lam)
    want = ref.phi_rows(img, idx, np.arange(w * h), phi_A, lam, alpha, H_LOC, H_VAL)
    print("f32 stages %dx%d: Phi rel-L2 %.2e" % (w, h, _rel(phi, want)))
    assert _rel(phi, want) <= 1e-5


@pytest.mark.parametrize("sampling", [glf.SAMPLING_UNIFORM, glf.SAMPLING_RANDOM])
@pytest.mark.parametrize("mode", list(MODES))
def test_whole_path_against_numpy(mode, sampling):
    """Every filter mode on both samplers, from the run's own by-products (glf_image_processing_f32_capture)."""
    w, h, ns, m = 61, 47, 100, 8
    img = _f32_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], sampling=sampling, h_val=H_VAL)
    idx = glf.Sampling(w, h, ns) if sampling == glf.SAMPLING_UNIFORM else glf.RandomSampling(w, h, ns, seed=int(opt.sampling_seed))
    with glf.Context(0) as ctx:
        z, info = _whole(ctx, img, opt, capture=True)
        cap = info["capture"]
        phi_A = cap["phi_A"].cpu().numpy()[:len(idx), :m].astype(np.float64)
        phi = cap["phi"].cpu().numpy()[:, :m].astype(np.float64)
    assert z.dtype == np.float32 and z.shape == (h, w)
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
    x = img.reshape(-1).astype(np.float64)
    corr = z.reshape(-1).astype(np.float64) - (1.0 - ysub) * x
    want = ref.correction(img, phi, lam, MODES[mode], float(opt.gain))
    err = _rel(corr, want)
    print("f32 whole path %s sampling %d: rel-L2 of the correction %.2e" % (mode, sampling, err))
    assert err <= 1e-5, err


# ---- the same template source on the same f32 values: the 16-bit call's bits ---------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_equals_the_u16_call_on_integer_values(mode):
    """x = a 16-bit image: the float call on x.astype(float32) and the 16-bit call on x run the same template source on the same f32
    values -- D_A, the eigenvalues and z (against the 16-bit call's float z) bit for bit."""
    w, h, ns, m = 61, 47, 100, 8
    x = _u16_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], h_val=H_VAL16)
    with glf.Context(0) as ctx:
        z, info = _whole(ctx, x.astype(np.float32), opt, capture=True)
        _, zf16, info16 = _whole16(ctx, x, opt, capture=True)
    d = float(np.abs(z.astype(np.float64) - zf16).max())
    print("f32 against u16 (%s): max |z - zf16| %.3e, max rel eigenvalue difference %.3e" %
          (mode, d, float(np.abs(np.asarray(info["eigvals"]) / np.asarray(info16["eigvals"]) - 1.0).max())))
    np.testing.assert_array_equal(info["capture"]["degree"], info16["capture"]["degree"])
    np.testing.assert_array_equal(info["eigvals"], info16["eigvals"])
    assert info["outer_its"] == info16["outer_its"] and _route(info) == _route(info16)
    np.testing.assert_array_equal(_bits(z), _bits(zf16))


@pytest.mark.parametrize("mode", list(MODES))
def test_power_of_two_scale_covariance(mode):
    """x 2^-16 (values in [0, 1)) at h_val 2^-16: s_val scales by exactly 2^32, dist2 by exactly 2^-32, and every sum downstream is
    linear in x, so the eigenvalues are those of the unscaled call and z = 2^-16 z_unscaled, bit for bit. (The 16-bit entry point
    cannot take this image: every pixel rounds to 0.)"""
    w, h, ns, m = 61, 47, 100, 8
    x = _u16_image(h, w, seed=3).astype(np.float32)
    s = np.float32(2.0 ** -16)
    xs = x * s
    assert xs.max() < 1.0 and np.array_equal(xs.astype(np.float64) * 65536.0, x.astype(np.float64))
    kw = dict(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode])
    with glf.Context(0) as ctx:
        z, info = _whole(ctx, x, glf.default_options(h_val=H_VAL16, **kw))
        zs, infos = _whole(ctx, xs, glf.default_options(h_val=H_VAL16 * 2.0 ** -16, **kw))
    np.testing.assert_array_equal(infos["eigvals"], info["eigvals"])
    assert infos["alpha"] == info["alpha"] and infos["outer_its"] == info["outer_its"]
    np.testing.assert_array_equal(_bits(zs), _bits(z * s))


# ---- an edge below one 16-bit level ---------------------------------------------------------------------------------------------------

def _edge_image(h, w, seed=0):
    """The 16-bit suite's edge image: two flat halves at 32 836 and 32 956 plus fixed-seed noise sigma = 15 clipped at +-4 sigma."""
    img = np.empty((h, w))
    img[:, : w // 2] = 32836.0
    img[:, w // 2:] = 32956.0
    img += np.clip(np.random.default_rng(seed).normal(0.0, 15.0, img.shape), -60.0, 60.0)
    return np.rint(img).astype(np.uint16)


def _step_noise(z, w):
    """(|mean of the right half - mean of the left half|, rms of z about its half's mean), over pixels at least 8 px from the boundary."""
    left, right = z[:, : w // 2 - 8], z[:, w // 2 + 8:]
    step = abs(float(right.mean()) - float(left.mean()))
    dev = np.concatenate([(left - left.mean()).ravel(), (right - right.mean()).ravel()])
    return step, float(np.sqrt(np.mean(dev ** 2)))


def test_sub_16bit_edge_kept_only_in_float():
    """The 16-bit suite's edge image times 2^-9: a step of 120 / 512 = 0.234 units under noise of 0.03, all of it between 64.0 and
    64.5. The float route keeps the step (by the two tests above this is the 16-bit route's measured 119.9 of 119.8, scaled
    exactly); the 16-bit route on rint(x) sees a constant image and must show at most 5 % of the float route's step (a margin
    taken from the 8-bit analogue, which measured 0.08 of 119.9)."""
    h, w = 64, 64
    x = (_edge_image(h, w).astype(np.float64) * 2.0 ** -9).astype(np.float32)
    x16 = np.rint(x).astype(np.uint16)
    assert (x16 == 64).all()
    s_in, n_in = _step_noise(x.astype(np.float64), w)
    opt = glf.default_options(num_samples=200, num_eigvals=16, epsilon=1e-3, h_val=60.0 * 2.0 ** -9)
    with glf.Context(0) as ctx:
        z, _ = _whole(ctx, x, opt)
        _, z16, _ = _whole16(ctx, x16, opt)
    s32, n32 = _step_noise(z.astype(np.float64), w)
    s16, _ = _step_noise(z16.astype(np.float64), w)
    print("sub-16-bit edge: input step %.4f noise %.4f; float route step %.4f noise %.4f (in the 16-bit suite's units: %.1f of %.1f); "
          "16-bit route step %.5f (%.3f %% of the float route's)" % (s_in, n_in, s32, n32, 512.0 * s32, 512.0 * s_in, s16, 100.0 * s16 / s32))
    assert abs(s32 - s_in) <= 0.1 * s_in
    assert s16 <= 0.05 * s32


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
        _, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=False, kernel=K32, h_loc=H_LOC, h_val=H_VAL)
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
    print("f32 %dx%d: Phi rel-L2 band %.2e entrywise %.2e, max |band - entrywise| / max |Phi| %.2e" % (w, h, e_band, e_entry, d))
    assert e_band <= 1e-5 and e_entry <= 1e-5
    assert d <= 2e-5                                     # (forms of different arithmetic: the suite's bound between them)
    assert np.any(got["band"] != got["entrywise"])      # (another arithmetic: the key did select another kernel)


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_path_small_forced_band(mode):
    """Route (4, 4, 0): the eigenvalues within 1e-5 of the key-off run's, Phi and the correction within 1e-5 of numpy."""
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
    x = img.reshape(-1).astype(np.float64)
    corr = z.reshape(-1).astype(np.float64) - (1.0 - ysub) * x
    want = ref.correction(img, phi, lam, MODES[mode], float(opt.gain))
    err = _rel(corr, want)
    print("f32 band %s: Phi rel-L2 %.2e, correction rel-L2 %.2e" % (mode, e_phi, err))
    assert e_phi <= 1e-5
    assert err <= 1e-5, err


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
    print("f32 band: nystroem_evaluated %.4e with the skips, %.4e without" % (info_b["nystroem_evaluated"], info_c["nystroem_evaluated"]))
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
    z, so, info = ctx.image_processing_f32_signals(_dev(ctx, img), d_sig, opt)
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
    1e-5 relative L2 of the correction. The correction is read back from z, which the API stores in f32; numpy's z goes through the
    same storage before the corrections are compared (test_whole_path_small_forced_band's rule in the band suite: the bound is
    unchanged, and every error of the route still shows). The last plane is the guide itself and must come out as the guide's z to within one ulp of the float output."""
    w, h, ns, m = 61, 47, 100, 8
    img = _f32_image(h, w, seed=3)
    sig = np.concatenate([_test_planes(h, w), img[None]])
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
        print("f32 %s plane %d: rel-L2 of the correction %.2e (against numpy's before its f32 storage: %.2e)" % (mode, k, err, _rel(got, want)))
        assert err <= 1e-5, (k, err)
    assert _rel(so[-1], z) <= 2.0 ** -23                # (both are one f32 rounding of the same fp64 sum, formed by two statements)


def test_planes_independent_of_their_neighbours():
    w, h, ns, m = 61, 47, 100, 8
    img = _f32_image(h, w, seed=3)
    s1, s2, depth = _test_planes(h, w, 7)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, h_val=H_VAL)
    with glf.Context(0) as ctx:
        four = _signals(ctx, img, np.stack([s1, s2, depth, img]), opt)[1]
        two = _signals(ctx, img, np.stack([s2, s1]), opt)[1]
        ones = [_signals(ctx, img, s[None], opt)[1][0] for s in (s1, s2, depth, img)]
    for k in range(4):
        np.testing.assert_array_equal(_bits(four[k]), _bits(ones[k]), err_msg="plane %d of 4 against alone" % k)
    np.testing.assert_array_equal(_bits(two[0]), _bits(ones[1]))
    np.testing.assert_array_equal(_bits(two[1]), _bits(ones[0]))


# ---- refusals and bookkeeping ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_is_refused_and_nothing_is_written(bad):
    w, h, ns = 61, 47, 100
    img = _f32_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=8, epsilon=0.05, h_val=H_VAL)
    idx = set(int(i) for i in glf.Sampling(w, h, ns))
    px = next(i for i in range(w * h - 1, 0, -1) if i not in idx)       # a pixel that is not a sample
    poisoned = img.copy()
    poisoned.reshape(-1)[px] = bad
    with glf.Context(0) as ctx:
        z0, info0 = _whole(ctx, img, opt)
        out = torch.full((h, w), 7.0, dtype=torch.float32, device=ctx.device)
        sig = torch.zeros((1, h, w), dtype=torch.float32, device=ctx.device)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_f32(_dev(ctx, poisoned), opt, out=out)
        assert e.value.status == glf.ERR_INVALID and ("NaN" in str(e.value) or "Inf" in str(e.value))
        assert bool((out == 7.0).all())
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_f32_signals(_dev(ctx, poisoned), sig, opt)
        assert e.value.status == glf.ERR_INVALID
        with pytest.raises(glf.GlfError) as e:
            ctx.ComputeAffinityMatrices(_dev(ctx, poisoned), glf.Sampling(w, h, ns), want_KA=False, kernel=K32, h_loc=H_LOC, h_val=H_VAL)
        assert e.value.status == glf.ERR_INVALID
        z1, info1 = _whole(ctx, img, opt)                                # the context still works, and gives the same bits
    np.testing.assert_array_equal(_bits(z1), _bits(z0))
    np.testing.assert_array_equal(info1["eigvals"], info0["eigvals"])
    with glf.Multi(2, devices=[0, 0], backend=glf.MULTI_LOOPBACK) as world:
        with pytest.raises(glf.GlfError) as e:
            world.image_processing_f32(poisoned, opt)
        assert e.value.status == glf.ERR_INVALID
        zm, _ = world.image_processing_f32(img, opt)                     # the world is still usable
    assert np.isfinite(zm).all()


def test_invalid_and_unsupported_with_a_live_context():
    w, h = 40, 32
    img = _f32_image(h, w, seed=1)
    with glf.Context(0) as ctx:
        d = _dev(ctx, img)
        sig = torch.zeros((1, h, w), dtype=torch.float32, device=ctx.device)
        for kernel in (glf.KERNEL_PHOTOMETRIC, glf.KERNEL_SPATIAL, glf.KERNEL_NLM, glf.KERNEL_BILATERAL_RGB, glf.KERNEL_BILATERAL_U16):
            with pytest.raises(glf.GlfError) as e:
                ctx.image_processing_f32(d, glf.default_options(num_samples=30, num_eigvals=4, kernel=kernel))
            assert e.value.status == glf.ERR_UNSUPPORTED, kernel
            with pytest.raises(glf.GlfError) as e:
                ctx.image_processing_f32_signals(d, sig, glf.default_options(num_samples=30, num_eigvals=4, kernel=kernel))
            assert e.value.status == glf.ERR_UNSUPPORTED, kernel
        f32_opt = glf.default_options(num_samples=30, num_eigvals=4, kernel=K32, h_val=H_VAL)
        g = ctx.to_device(glf.synth_image(w, h, seed=1))
        with pytest.raises(glf.GlfError) as e:           # the other entry points never read their pixels as floats
            ctx.image_processing(g, f32_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_signals(g, sig, f32_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=ctx.device)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_rgb(rgb, f32_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        u16 = torch.zeros((h, w), dtype=torch.int16, device=ctx.device).view(torch.uint16)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_u16(u16, f32_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_u16_signals(u16, sig, f32_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:           # more than 256 eigenpairs
            ctx.image_processing_f32(d, glf.default_options(num_samples=400, num_eigvals=300, h_val=H_VAL))
        assert e.value.status == glf.ERR_UNSUPPORTED
        C = glf.C
        out = torch.zeros((h, w), dtype=torch.float32, device=ctx.device)
        rc = glf._lib.glf_image_processing_f32(ctx._ctx, None, None, w, h, C.c_void_p(out.data_ptr()), None, None)
        assert rc == glf.ERR_INVALID
        rc = glf._lib.glf_image_processing_f32(ctx._ctx, None, C.c_void_p(d.data_ptr()), w, h, None, None, None)
        assert rc == glf.ERR_INVALID
        z, info = ctx.image_processing_f32(d, f32_opt)   # kernel 6 is the float kernel's own id; the context still works
        assert z.shape == (h, w) and z.dtype == torch.float32 and info["m"] == 4 and bool(torch.isfinite(z).all())


def test_grey_and_u16_calls_after_an_f32_call_are_unchanged():
    g = glf.synth_image(96, 80, seed=4)
    x16 = _u16_image(80, 96, seed=2)
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05)
    opt16 = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=H_VAL16)
    with glf.Context(0) as fresh:
        out0, zf0, _ = fresh.image_processing(fresh.to_device(g), opt, want_float=True)
        out0, zf0 = out0.cpu().numpy(), zf0.cpu().numpy()
    with glf.Context(0) as fresh:
        o16, z16, i16 = _whole16(fresh, x16, opt16)
    with glf.Context(0) as ctx:
        _whole(ctx, _f32_image(80, 96, seed=2), glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=H_VAL))
        out1, zf1, _ = ctx.image_processing(ctx.to_device(g), opt, want_float=True)
        np.testing.assert_array_equal(out1.cpu().numpy(), out0)
        np.testing.assert_array_equal(_bits(zf1.cpu().numpy()), _bits(zf0))
        o16b, z16b, i16b = _whole16(ctx, x16, opt16)
    np.testing.assert_array_equal(o16b, o16)
    np.testing.assert_array_equal(_bits(z16b), _bits(z16))
    np.testing.assert_array_equal(i16b["eigvals"], i16["eigvals"])


@pytest.mark.parametrize("band", [False, True])
def test_debug_pool_f32_run(monkeypatch, band):
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
        assert _route(info) == ((4, 4, 0) if band else (0, 0, 0))
        assert np.isfinite(z).all() and np.isfinite(so).all() and np.isfinite(info["eigvals"]).all()
        np.testing.assert_array_equal(_bits(z2), _bits(z))


# ---- 2048^2: sampled rows of the stage path ------------------------------------------------------------------------------------------------

def test_2048_sampled_rows_against_numpy():
    """At 2048^2 (about 10 500 samples) the stage path's Phi rows of sampled pixels against numpy's extension of its Phi_A, with the
    PIX_BAND key off and on (the same Phi_A and eigenvalues through both Nystroem kernels)."""
    n, m = 2048, 16
    img = _f32_image(n, n, seed=11)
    idx = glf.Sampling(n, n, int(n * n * 0.0025))
    with glf.Context(0) as ctx:
        _, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=False, kernel=K32, h_loc=H_LOC, h_val=H_VAL)
        deg = ctx.degree_of(K_B)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        vecs, vals, _ = ctx.InversePowerIteration(L_A, m, epsilon=0.1)
        lam = ctx.mat_to_numpy(vals).astype(np.float64)
        phi_A = ctx.mat_to_numpy(vecs)[:len(idx)].astype(np.float64)
        pinv = ctx.InverseDiagMat(vals)
        pix = np.sort(np.random.default_rng(0).choice(n * n, 48, replace=False))
        rows = {}
        for key in (None, "1"):
            ctx.set_tuning(PIX_BAND=key)
            phi_sf = ctx.Nystroem(L_B, vecs, pinv)
            phi_r = ctx.Permutation(phi_sf, idx)
            rows[key] = _read_rows(ctx, phi_r, pix, m)
            ctx.destroy(phi_sf, phi_r)
        ctx.destroy(K_B, L_A, vecs, vals, pinv)
    sel = np.arange(0, len(idx), max(1, len(idx) // 24))
    np.testing.assert_allclose(deg[sel], ref.degree(img, idx[sel], H_LOC, H_VAL, chunk=1 << 20), rtol=1e-6)
    want = ref.phi_rows(img, idx, pix, phi_A, lam, alpha, H_LOC, H_VAL)
    print("f32 2048^2 stage path: Phi rows rel-L2 %.2e (key off), %.2e (key on)" % (_rel(rows[None], want), _rel(rows["1"], want)))
    assert _rel(rows[None], want) <= 1e-5 and _rel(rows["1"], want) <= 1e-5
    assert np.any(rows[None] != rows["1"])                  # (the key selected the band kernel: another arithmetic)
