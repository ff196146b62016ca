"""16-bit greyscale filtering (GLF_KERNEL_BILATERAL_U16, glf_image_processing_u16): the graph is built from the 16-bit values and
the image goes through its filter.

Checked against the fp64 numpy restatement in tests/u16_ref.py: the stage kernels (K_A, D_A, the Nystroem extension), the whole
path in every filter mode on both samplers, the 8-bit equivalence (257 g at h_val 257 is the graph of g at h_val), an edge smaller
than one 8-bit level that only the 16-bit route keeps, 2048^2 sampled rows, the context's bookkeeping and the declines.

Tolerances. The only arithmetic the 16-bit kernel adds to the 8-bit one is the f32 rounding of dv^2 (up to 32 bits): the exponent's
relative error is ~2^-23 and every kernel entry stays within ~1e-7 of the fp64 value (entrywise.hip), so K_A and D_A are held to 1e-6 of
their maxima like the 8-bit and colour kernels, and Phi and the corrections to the 1e-5 relative L2 the colour tests use."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import u16_ref as ref  # noqa: E402

MODES = {"reference": glf.FILTER_REFERENCE, "poc": glf.FILTER_POC, "smooth": glf.FILTER_SMOOTH, "sharpen": glf.FILTER_SHARPEN}
H_LOC, H_VAL = 40.0, 30.0 * 257.0


def _u16_image(h, w, seed=0):
    """A 16-bit test image: smooth ramps, a disc of another level and noise, over most of 0..65535."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 9000.0 + 30000.0 * c / max(1, w - 1) + 12000.0 * np.sin(r / 9.0)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    img[disc] = 58000.0
    img += rng.normal(0.0, 1500.0, img.shape)
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16)


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def _dev(ctx, img16):
    return torch.from_numpy(np.ascontiguousarray(img16, dtype=np.uint16)).to(ctx.device)


def _stages(ctx, img, idx, m, epsilon=0.1):
    """The stage entry points on the 16-bit kernel: (K_A, D_A, alpha, eigvals, phi_A [p, m], Phi raster [N, m])."""
    K_A, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=True, kernel=glf.KERNEL_BILATERAL_U16, h_loc=H_LOC, h_val=H_VAL)
    ka, deg = ctx.mat_to_numpy(K_A).astype(np.float64), ctx.degree_of(K_B)
    L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
    vecs, vals, _ = ctx.InversePowerIteration(L_A, m, epsilon=epsilon)
    lam = ctx.mat_to_numpy(vals).astype(np.float64)
    phi_A = ctx.mat_to_numpy(vecs)[:len(idx)].astype(np.float64)
    pinv = ctx.InverseDiagMat(vals)
    phi_sf = ctx.Nystroem(L_B, vecs, pinv)
    phi_r = ctx.Permutation(phi_sf, idx)
    phi = ctx.mat_to_numpy(phi_r).astype(np.float64)
    ctx.destroy(K_A, K_B, L_A, vecs, vals, pinv, phi_sf, phi_r)
    return ka, deg, alpha, lam, phi_A, phi


@pytest.mark.parametrize("w,h", [(48, 40), (97, 61), (64, 64)])
def test_stages_against_numpy(w, h):
    img = _u16_image(h, w, seed=w)
    idx = glf.Sampling(w, h, 120)
    with glf.Context(0) as ctx:
        ka, deg, alpha, lam, phi_A, phi = _stages(ctx, img, idx, 8, epsilon=1e-3)
    KA, D, alpha_ref, LA = ref.laplacian(img, idx, H_LOC, H_VAL)
    assert float(np.abs(ka - KA).max()) <= 1e-6 * float(np.abs(KA).max())
    assert float(np.abs(deg - D).max()) <= 1e-6 * float(D.max())
    assert abs(alpha - alpha_ref) <= 1e-6 * alpha_ref
    # eigenpairs of the fp64 L_A: the residual the eigen-solve's own stopping rule allows
    for j in range(lam.size):
        v = phi_A[:, j] / np.linalg.norm(phi_A[:, j])
        assert np.linalg.norm(LA @ v - lam[j] * v) <= 2e-2 * max(lam[j], 1e-3), (j, lam[j])
    # Phi against the numpy extension of the GPU's own Phi_A
    want = ref.phi_rows(img, idx, np.arange(w * h), phi_A, lam, alpha, H_LOC, H_VAL)
    assert _rel(phi, want) <= 1e-5


def _whole(ctx, img, opt, capture=False):
    out, zf, info = ctx.image_processing_u16(_dev(ctx, img), opt, want_float=True, capture=capture)
    return out.cpu().numpy(), zf.cpu().numpy().astype(np.float64), info


@pytest.mark.parametrize("sampling", [glf.SAMPLING_UNIFORM, glf.SAMPLING_RANDOM])
@pytest.mark.parametrize("mode", list(MODES))
def test_whole_path_against_numpy(mode, sampling):
    """Every filter mode on both samplers, from the run's own by-products (glf_image_processing_u16_capture): D_A against the fp64
    restatement, the eigenpairs against the fp64 L_A, Phi against numpy's extension of the run's Phi_A, and the correction
    z - (1 - ysub) x against numpy's from the run's Phi and eigenvalues."""
    w, h, ns, m = 61, 47, 100, 8
    img = _u16_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], sampling=sampling, h_val=H_VAL)
    idx = glf.Sampling(w, h, ns) if sampling == glf.SAMPLING_UNIFORM else glf.RandomSampling(w, h, ns, seed=int(opt.sampling_seed))
    with glf.Context(0) as ctx:
        out, zf, info = _whole(ctx, img, opt, capture=True)
        cap = info["capture"]
        phi_A = cap["phi_A"].cpu().numpy()[:len(idx), :m].astype(np.float64)
        phi = cap["phi"].cpu().numpy()[:, :m].astype(np.float64)
    assert (info["nystroem_path"], info["matvec_path"], info["filter_fused"]) == (0, 0, 0)
    assert info["contraction"] == glf.CONTRACT_F32_MFMA
    assert info["p"] == len(idx) and info["m"] == m
    assert 0 < info["degree_evaluated"] <= float(len(idx)) * w * h
    _, D, alpha, LA = ref.laplacian(img, idx, H_LOC, H_VAL)
    np.testing.assert_allclose(cap["degree"], D, rtol=1e-6)
    assert abs(info["alpha"] - alpha) <= 1e-6 * alpha
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    for j in range(m):   # the residual the eigen-solve's own stopping rule allows (as test_stages_against_numpy)
        v = phi_A[:, j] / np.linalg.norm(phi_A[:, j])
        assert np.linalg.norm(LA @ v - lam[j] * v) <= 2e-2 * max(lam[j], 1e-3), (j, lam[j])
    want_phi = ref.phi_rows(img, idx, np.arange(w * h), phi_A, lam, info["alpha"], H_LOC, H_VAL)
    assert _rel(phi, want_phi) <= 1e-5
    ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
    x = img.reshape(-1).astype(np.float64)
    corr = zf.reshape(-1) - (1.0 - ysub) * x
    want = ref.correction(img, phi, lam, MODES[mode], float(opt.gain))
    err = _rel(corr, want)
    print("u16 whole path %s sampling %d: rel-L2 of the correction %.2e" % (mode, sampling, err))
    assert err <= 1e-5, err
    # the u16 output is the clamped truncation x + floor(c) (the grey d_out's rule at 16 bits): the float z = x + c rounds a small
    # negative c up to x, so a pixel may sit one level below the truncation of its float z, never further
    zt = np.clip(np.floor(zf), 0, 65535)
    d = out.astype(np.int64) - zt
    assert d.max() <= 0 and d.min() >= -1


def test_8bit_equivalence():
    """img16 = 257 g at h_val 257 is the graph of g at h_val: the degree, the eigenvalues and the correction, on the same arithmetic
    (f32 contraction, the direct paths forced for the 8-bit call)."""
    w, h, ns, m = 80, 64, 120, 8
    g = glf.synth_image(w, h, seed=5)
    img16 = g.astype(np.uint16) * 257
    idx = glf.Sampling(w, h, ns)
    for mode in ("reference", "smooth"):
        with glf.Context(0) as ctx:
            ctx.set_contraction(glf.CONTRACT_F32_MFMA)
            ctx.set_tuning(NYS_PATH="direct", DEG_PATH="direct", MV_PATH="dense")
            opt8 = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.05, filter_mode=MODES[mode], h_val=30.0)
            _, zf8, info8 = ctx.image_processing(ctx.to_device(g), opt8, want_float=True)
            zf8 = zf8.cpu().numpy().astype(np.float64)
            opt16 = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.05, filter_mode=MODES[mode], h_val=30.0 * 257.0)
            _, zf16, info16 = _whole(ctx, img16, opt16)
            _, KB16 = ctx.ComputeAffinityMatrices(_dev(ctx, img16), idx, want_KA=False, kernel=glf.KERNEL_BILATERAL_U16, h_val=30.0 * 257.0)
            _, KB8 = ctx.ComputeAffinityMatrices(ctx.to_device(g), idx, want_KA=False, kernel=glf.KERNEL_BILATERAL, h_val=30.0)
            deg16, deg8 = ctx.degree_of(KB16), ctx.degree_of(KB8)
            ctx.destroy(KB16, KB8)
        np.testing.assert_allclose(deg16, deg8, rtol=1e-6)
        assert info16["outer_its"] == info8["outer_its"]
        np.testing.assert_allclose(info16["eigvals"], info8["eigvals"], rtol=1e-5)
        ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
        c8 = zf8 - (1.0 - ysub) * g
        c16 = (zf16 - (1.0 - ysub) * img16) / 257.0
        err = _rel(c16, c8)
        # the corrections are read back from z stored in f32: half an ulp of each z (the 16-bit z in 8-bit units) is in both,
        # whatever the arithmetic before it (measured: reference filter 1.05e-5 against a storage bound of 2.8e-5, smooth filter
        # 9.1e-6 against 9e-8)
        floor = float(np.linalg.norm(0.5 * np.spacing(zf16.astype(np.float32)).astype(np.float64) / 257.0 +
                                     0.5 * np.spacing(zf8.astype(np.float32)).astype(np.float64)) / np.linalg.norm(c8))
        print("8-bit equivalence %s: rel-L2 of the correction %.2e (f32 storage of z: %.2e)" % (mode, err, floor))
        assert err <= 1e-5 + floor, (mode, err, floor)


def _edge_image(h, w, seed=0):
    """Two flat halves at 32 836 and 32 956 (a 120-unit step) plus fixed-seed noise sigma = 15 clipped at +-4 sigma: every pixel
    rounds to 8-bit level 128 (127.5 * 257 = 32 767.5 and 128.5 * 257 = 33 024.5 are 4.6 sigma away)."""
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


def test_sub_8bit_edge_kept_only_at_16_bits():
    """A 120-unit step under sigma = 15 noise: below one 8-bit level, so quantising to 8 bits leaves a constant image and the step is
    lost before the graph is built. The 16-bit route must keep it; the 8-bit route on round(img / 257) at h_val / 257, scaled back by
    257, must show a step of at most 5 % of the 16-bit route's (its input is constant: its step is ~0).

    Changed from the planned smooth-filter denoising check (step-to-noise ratio at least twice the input's 120 / 15 = 8), because no
    filter of this library denoises this image at m = 16, h_val = 60: in the fp64 numpy restatement (tests/u16_ref.py, the same
    samples, exact eigenvectors) the smooth and sharpening filters (z = Phi f(Pi) Phi^T y, no y term) return z of mean 0 with step
    0.00 and rms 0.49 / 0.30 (the Nystroem-extended basis does not carry the image's level), the reference and PoC filters step 119.8
    with rms 15.9 / 16.8 (ratio 7.5 / 7.1, the input's 8.0). The check therefore runs the library's default reference filter and asks
    for the step alone: within 10 % of the input's on the 16-bit route. On the GPU at epsilon = 0.05 that route measured step 113.9
    with rms 277 about the halves' means: the image's level (32 896) cancels in c = Phi^T y, so the eigen-solve's stopping rule shows
    in z at the size of one 8-bit level; the check runs at epsilon = 1e-3. Measured there: 16-bit route step 119.9 (output 119.5)
    with rms 17.8; 8-bit route step 0.08 (output 1.34)."""
    h, w = 64, 64
    img = _edge_image(h, w)
    g8 = np.rint(img / 257.0).astype(np.uint8)
    assert (g8 == 128).all()
    s_in, n_in = _step_noise(img.astype(np.float64), w)
    opt16 = glf.default_options(num_samples=200, num_eigvals=16, epsilon=1e-3, h_val=60.0)
    opt8 = glf.default_options(num_samples=200, num_eigvals=16, epsilon=1e-3, h_val=60.0 / 257.0)
    with glf.Context(0) as ctx:
        out16, z16, _ = _whole(ctx, img, opt16)
        out8, z8, _ = ctx.image_processing(ctx.to_device(g8), opt8, want_float=True)
        out8, z8 = out8.cpu().numpy(), z8.cpu().numpy().astype(np.float64) * 257.0
    s16, n16 = _step_noise(z16, w)
    s8, _ = _step_noise(z8, w)
    so16, _ = _step_noise(out16.astype(np.float64), w)
    so8, _ = _step_noise(out8.astype(np.float64) * 257.0, w)
    print("sub-8-bit edge: input step %.1f noise %.2f (ratio %.2f); 16-bit route step %.1f noise %.2f (ratio %.2f), output step %.1f; "
          "8-bit route step %.2f, output step %.2f" % (s_in, n_in, s_in / n_in, s16, n16, s16 / n16, so16, s8, so8))
    assert abs(s16 - s_in) <= 0.1 * s_in and abs(so16 - s_in) <= 0.1 * s_in
    assert s8 <= 0.05 * s16 and so8 <= 0.05 * so16


def test_2048_sampled_rows_against_numpy():
    """At 2048^2 (about 10 500 samples) the stage path's Phi rows of sampled pixels against numpy's extension of its Phi_A."""
    n = 2048
    img = _u16_image(n, n, seed=11)
    idx = glf.Sampling(n, n, int(n * n * 0.0025))
    with glf.Context(0) as ctx:
        _, K_B = ctx.ComputeAffinityMatrices(_dev(ctx, img), idx, want_KA=False, kernel=glf.KERNEL_BILATERAL_U16, h_loc=H_LOC, h_val=H_VAL)
        deg = ctx.degree_of(K_B)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        vecs, vals, _ = ctx.InversePowerIteration(L_A, 16, epsilon=0.1)
        lam = ctx.mat_to_numpy(vals).astype(np.float64)
        phi_A = ctx.mat_to_numpy(vecs)[:len(idx)].astype(np.float64)
        pinv = ctx.InverseDiagMat(vals)
        phi_sf = ctx.Nystroem(L_B, vecs, pinv)
        phi_r = ctx.Permutation(phi_sf, idx)
        rng = np.random.default_rng(0)
        pix = np.sort(rng.choice(n * n, 48, replace=False))
        rows = np.empty((pix.size, 16))
        full = np.empty((1, phi_r.ld), dtype=np.float32)
        for k, px in enumerate(pix):
            glf._lib.glf_memcpy_d2h(ctx._ctx, full.ctypes.data_as(glf.C.c_void_p), glf.C.c_void_p(phi_r.data + 4 * int(px) * phi_r.ld),
                                    glf.C.c_size_t(full.nbytes))
            rows[k] = full[0, :16]
        ctx.destroy(K_B, L_A, vecs, vals, pinv, phi_sf, phi_r)
    sel = np.arange(0, len(idx), max(1, len(idx) // 24))
    np.testing.assert_allclose(deg[sel], ref.degree(img, idx[sel], H_LOC, H_VAL, chunk=1 << 20), rtol=1e-6)
    want = ref.phi_rows(img, idx, pix, phi_A, lam, alpha, H_LOC, H_VAL)
    assert _rel(rows, want) <= 1e-5


def test_grey_call_after_u16_call_is_unchanged():
    g = glf.synth_image(96, 80, seed=4)
    img = _u16_image(80, 96, seed=2)
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05)
    with glf.Context(0) as fresh:
        out0, zf0, _ = fresh.image_processing(fresh.to_device(g), opt, want_float=True)
        out0, zf0 = out0.cpu().numpy(), zf0.cpu().numpy()
    with glf.Context(0) as ctx:
        _whole(ctx, img, glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=H_VAL))
        out1, zf1, _ = ctx.image_processing(ctx.to_device(g), opt, want_float=True)
        np.testing.assert_array_equal(out1.cpu().numpy(), out0)
        np.testing.assert_array_equal(zf1.cpu().numpy().view(np.int32), zf0.view(np.int32))


def test_debug_pool_u16_run(monkeypatch):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    img = _u16_image(72, 90, seed=8)
    for mode in ("reference", "sharpen"):
        opt = glf.default_options(num_samples=80, num_eigvals=8, epsilon=0.05, filter_mode=MODES[mode], h_val=H_VAL)
        with glf.Context(0) as ctx:
            out, zf, info = _whole(ctx, img, opt)
            assert ctx.debug_violations() == 0
        assert np.isfinite(zf).all() and np.isfinite(info["eigvals"]).all()


def test_forced_factored_forms_decline_the_u16_kernel():
    """Forcing the grid / rank / band tuning (and the split-f16 contraction) still runs the entry-by-entry route: paths (0, 0, 0), the
    f32 contraction, and the same outputs as the default tuning."""
    img = _u16_image(64, 72, seed=6)
    opt = glf.default_options(num_samples=100, num_eigvals=8, epsilon=0.05, h_val=H_VAL)
    with glf.Context(0) as ctx:
        ctx.set_contraction(glf.CONTRACT_F16_SPLIT)
        out0, zf0, _ = _whole(ctx, img, opt)
    for tune in (dict(NYS_PATH="grid", DEG_PATH="grid", MV_PATH="grid"), dict(NYS_PATH="rank", DEG_PATH="grid", MV_PATH="rank"),
                 dict(NYS_PATH="band", DEG_PATH="grid", MV_PATH="band")):
        with glf.Context(0) as ctx:
            ctx.set_contraction(glf.CONTRACT_F16_SPLIT)
            ctx.set_tuning(**tune)
            out, zf, info = _whole(ctx, img, opt)
        assert (info["nystroem_path"], info["matvec_path"], info["filter_fused"]) == (0, 0, 0), tune
        assert info["contraction"] == glf.CONTRACT_F32_MFMA
        np.testing.assert_array_equal(out, out0)
        np.testing.assert_array_equal(zf, zf0)


def test_invalid_and_unsupported_with_a_live_context():
    img = _u16_image(32, 40, seed=1)
    with glf.Context(0) as ctx:
        d = _dev(ctx, img)
        for kernel in (glf.KERNEL_PHOTOMETRIC, glf.KERNEL_SPATIAL, glf.KERNEL_NLM, glf.KERNEL_BILATERAL_RGB):
            with pytest.raises(glf.GlfError) as e:
                ctx.image_processing_u16(d, glf.default_options(num_samples=30, num_eigvals=4, kernel=kernel))
            assert e.value.status == glf.ERR_UNSUPPORTED
        g = ctx.to_device((img >> 8).astype(np.uint8))
        u16_opt = glf.default_options(num_samples=30, num_eigvals=4, kernel=glf.KERNEL_BILATERAL_U16)
        with pytest.raises(glf.GlfError) as e:           # the 8-bit entry points never read 16-bit values as bytes
            ctx.image_processing(g, u16_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_signals(g, torch.zeros((1, 32, 40), dtype=torch.float32, device=ctx.device), u16_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        rgb = torch.from_numpy(np.zeros((32, 40, 3), dtype=np.uint8)).to(ctx.device)
        with pytest.raises(glf.GlfError) as e:
            ctx.image_processing_rgb(rgb, u16_opt)
        assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:           # more than 256 eigenpairs
            ctx.image_processing_u16(d, glf.default_options(num_samples=400, num_eigvals=300))
        assert e.value.status == glf.ERR_UNSUPPORTED
        C = glf.C
        out = torch.zeros((32, 40), dtype=torch.int16, device=ctx.device)
        rc = glf._lib.glf_image_processing_u16(ctx._ctx, None, None, 40, 32, C.c_void_p(out.data_ptr()), None, None, None)
        assert rc == glf.ERR_INVALID
        rc = glf._lib.glf_image_processing_u16(ctx._ctx, None, C.c_void_p(d.data_ptr()), 40, 32, None, None, None, None)
        assert rc == glf.ERR_INVALID
        o, _, info = ctx.image_processing_u16(d, u16_opt)
        assert o.shape == (32, 40) and o.dtype == torch.uint16 and info["m"] == 4
