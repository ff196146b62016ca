"""Colour-guided filtering (GLF_KERNEL_BILATERAL_RGB, glf_image_processing_rgb): the graph is built from the RGB differences and
R, G, B go through its filter.

Checked against the fp64 numpy restatement in tests/rgb_ref.py: the stage kernels (K_A, D_A, the Nystroem extension), the whole
path in every filter mode on both samplers, the grey equivalence (R = G = B = g at h_val sqrt(3) is the grey graph at h_val),
the isoluminant edge that the luma graph cannot see, 2048^2 sampled rows, and the context's bookkeeping."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import rgb_ref as ref  # noqa: E402

MODES = {"reference": glf.FILTER_REFERENCE, "poc": glf.FILTER_POC, "smooth": glf.FILTER_SMOOTH, "sharpen": glf.FILTER_SHARPEN}
H_LOC, H_VAL = 40.0, 30.0


def _rgb_image(h, w, seed=0):
    """A colour test image: smooth colour ramps, a disc of another colour and noise."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([60 + 120 * c / max(1, w - 1), 200 - 100 * r / max(1, h - 1), 90 + 40 * np.sin(c / 7.0)], axis=2)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    img[disc] = [210, 40, 160]
    img += rng.normal(0.0, 6.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def _stages(ctx, rgb, idx, m, epsilon=0.1):
    """The stage entry points on the colour kernel: (K_A, D_A, alpha, eigvals, phi_A [p, m], Phi raster [N, m])."""
    d_rgb = torch.from_numpy(rgb).to(ctx.device)
    K_A, K_B = ctx.ComputeAffinityMatrices(d_rgb, idx, want_KA=True, kernel=glf.KERNEL_BILATERAL_RGB, h_loc=H_LOC, h_val=H_VAL)
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
    rgb = _rgb_image(h, w, seed=w)
    idx = glf.Sampling(w, h, 120)
    with glf.Context(0) as ctx:
        ka, deg, alpha, lam, phi_A, phi = _stages(ctx, rgb, idx, 8, epsilon=1e-3)
    KA, D, alpha_ref, LA = ref.laplacian(rgb, idx, H_LOC, H_VAL)
    assert float(np.abs(ka - KA).max()) <= 1e-6 * float(np.abs(KA).max())
    assert float(np.abs(deg - D).max()) <= 1e-6 * float(D.max())
    assert abs(alpha - alpha_ref) <= 1e-6 * alpha_ref
    # eigenpairs of the fp64 L_A: the residual the eigen-solve's own stopping rule allows
    for j in range(lam.size):
        v = phi_A[:, j] / np.linalg.norm(phi_A[:, j])
        assert np.linalg.norm(LA @ v - lam[j] * v) <= 2e-2 * max(lam[j], 1e-3), (j, lam[j])
    # Phi against the numpy extension of the GPU's own Phi_A
    want = ref.phi_rows(rgb, idx, np.arange(w * h), phi_A, lam, alpha, H_LOC, H_VAL)
    assert _rel(phi, want) <= 1e-5


def _whole(ctx, rgb, opt):
    out, zf, info = ctx.image_processing_rgb(torch.from_numpy(rgb).to(ctx.device), opt, want_float=True)
    return out.cpu().numpy(), zf.cpu().numpy().astype(np.float64), info


@pytest.mark.parametrize("sampling", [glf.SAMPLING_UNIFORM, glf.SAMPLING_RANDOM])
@pytest.mark.parametrize("mode", list(MODES))
def test_whole_path_against_numpy(mode, sampling):
    """Every filter mode on both samplers, from the run's own by-products (glf_image_processing_rgb_capture): D_A against the fp64
    restatement, the eigenpairs against the fp64 L_A, Phi against numpy's extension of the run's Phi_A, and each channel's correction
    z_c - (1 - ysub) x_c against numpy's from the run's Phi and eigenvalues."""
    w, h, ns, m = 61, 47, 100, 8
    rgb = _rgb_image(h, w, seed=3)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], sampling=sampling)
    idx = glf.Sampling(w, h, ns) if sampling == glf.SAMPLING_UNIFORM else glf.RandomSampling(w, h, ns, seed=int(opt.sampling_seed))
    with glf.Context(0) as ctx:
        out, zf, info = ctx.image_processing_rgb(torch.from_numpy(rgb).to(ctx.device), opt, want_float=True, capture=True)
        out, zf = out.cpu().numpy(), zf.cpu().numpy().astype(np.float64)
        cap = info["capture"]
        phi_A = cap["phi_A"].cpu().numpy()[:len(idx), :m].astype(np.float64)
        phi = cap["phi"].cpu().numpy()[:, :m].astype(np.float64)
    assert (info["nystroem_path"], info["matvec_path"], info["filter_fused"]) == (0, 0, 0)
    assert info["p"] == len(idx) and info["m"] == m
    _, D, alpha, LA = ref.laplacian(rgb, idx, H_LOC, H_VAL)
    np.testing.assert_allclose(cap["degree"], D, rtol=1e-6)
    assert abs(info["alpha"] - alpha) <= 1e-6 * alpha
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    for j in range(m):   # the residual the eigen-solve's own stopping rule allows (as test_stages_against_numpy)
        v = phi_A[:, j] / np.linalg.norm(phi_A[:, j])
        assert np.linalg.norm(LA @ v - lam[j] * v) <= 2e-2 * max(lam[j], 1e-3), (j, lam[j])
    want_phi = ref.phi_rows(rgb, idx, np.arange(w * h), phi_A, lam, info["alpha"], H_LOC, H_VAL)
    assert _rel(phi, want_phi) <= 1e-5
    ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
    x = rgb.reshape(-1, 3).T.astype(np.float64)
    corr = zf.reshape(3, -1) - (1.0 - ysub) * x
    want = ref.corrections(rgb, phi, lam, MODES[mode], float(opt.gain))
    for k in range(3):
        err = _rel(corr[k], want[k])
        print("rgb whole path %s sampling %d channel %d: rel-L2 of the correction %.2e" % (mode, sampling, k, err))
        assert err <= 1e-5, (k, err)
    # the u8 output is the clamped truncation x + floor(c) (the grey d_out's rule): the float z = x + c rounds a small negative c
    # up to x, so a pixel may sit one level below the truncation of its float z, never further
    zt = np.clip(np.floor(zf.reshape(3, h, w).transpose(1, 2, 0)), 0, 255)
    d = out.astype(np.int64) - zt
    assert d.max() <= 0 and d.min() >= -1


def test_grey_equivalence():
    """R = G = B = g at h_val sqrt(3) is the grey graph at h_val: degree, eigenvalues, each channel's z and the u8 output."""
    w, h, ns, m = 80, 64, 120, 8
    g = glf.synth_image(w, h, seed=5)
    rgb = np.repeat(g[:, :, None], 3, axis=2).copy()
    idx = glf.Sampling(w, h, ns)
    for mode in ("reference", "smooth"):
        with glf.Context(0) as ctx:
            ctx.set_contraction(glf.CONTRACT_F32_MFMA)   # both on the entry-by-entry kernels with the f32 contraction
            ctx.set_tuning(NYS_PATH="direct", DEG_PATH="direct", MV_PATH="dense")
            opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.05, filter_mode=MODES[mode], h_val=H_VAL)
            out_g, zf_g, info_g = ctx.image_processing(ctx.to_device(g), opt, want_float=True)
            out_g, zf_g = out_g.cpu().numpy(), zf_g.cpu().numpy().astype(np.float64)
            opt_c = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.05, filter_mode=MODES[mode], h_val=H_VAL * math.sqrt(3.0))
            out_c, zf_c, info_c = _whole(ctx, rgb, opt_c)
            d_rgb, d_g = torch.from_numpy(rgb).to(ctx.device), ctx.to_device(g)
            _, KB_c = ctx.ComputeAffinityMatrices(d_rgb, idx, want_KA=False, kernel=glf.KERNEL_BILATERAL_RGB, h_val=H_VAL * math.sqrt(3.0))
            _, KB_g = ctx.ComputeAffinityMatrices(d_g, idx, want_KA=False, kernel=glf.KERNEL_BILATERAL, h_val=H_VAL)
            deg_c, deg_g = ctx.degree_of(KB_c), ctx.degree_of(KB_g)
            ctx.destroy(KB_c, KB_g)
        np.testing.assert_allclose(deg_c, deg_g, rtol=1e-6)
        assert info_c["outer_its"] == info_g["outer_its"]
        np.testing.assert_allclose(info_c["eigvals"], info_g["eigvals"], rtol=1e-5)
        ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
        cg = zf_g - (1.0 - ysub) * g
        for k in range(3):
            ck = zf_c[k] - (1.0 - ysub) * g
            assert _rel(ck, cg) <= 1e-5, (mode, k, _rel(ck, cg))
            assert np.mean(out_c[:, :, k] != out_g) < 1e-3


def _isoluminant(h, w, seed=0):
    """Two colour halves of equal BT.601 luma (a red-ish and a green-blue), plus noise."""
    a = np.array([200.0, 70.0, 90.0])
    ya = 0.299 * a[0] + 0.587 * a[1] + 0.114 * a[2]
    b = np.array([40.0, 0.0, 150.0])
    b[1] = (ya - 0.299 * b[0] - 0.114 * b[2]) / 0.587
    img = np.empty((h, w, 3))
    img[:, : w // 2] = a
    img[:, w // 2:] = b
    img += np.random.default_rng(seed).normal(0.0, 2.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _step(z):
    """Sharpness of the colour step: |mean colour of the column left of the boundary - of the column right of it| over the same
    distance between the mean colours of the outer eighths (1: a sharp step; a blur across the boundary makes it small)."""
    w = z.shape[1]
    near = z[:, w // 2 - 1].mean(axis=0) - z[:, w // 2].mean(axis=0)
    far = z[:, : w // 8].mean(axis=(0, 1)) - z[:, w - w // 8:].mean(axis=(0, 1))
    return float(np.linalg.norm(near) / np.linalg.norm(far))


def test_isoluminant_edge_kept_by_the_colour_graph():
    """The luma graph cannot see an edge between two colours of equal luma: filtering the chroma through it (-color -chroma)
    flattens the colour step; the colour graph keeps it (smooth filter, float outputs). Measured sharpness (step at the boundary
    over the step between the outer eighths): input 0.998, luma graph + chroma 0.136, colour graph 4.02 (the smooth filter pulls
    the outer eighths together, the boundary step stays)."""
    h, w = 48, 64
    rgb = _isoluminant(h, w)
    Y = np.array([[0.299, 0.587, 0.114], [-0.14714119, -0.28886916, 0.43601035], [0.61497538, -0.51496512, -0.10001026]])
    yuv = rgb.astype(np.float64) @ Y.T
    luma = np.clip(np.floor(yuv[:, :, 0] + 0.5), 0, 255).astype(np.uint8)
    assert int(luma[:, : w // 2].mean().round()) == int(luma[:, w // 2:].mean().round())
    opt = glf.default_options(num_samples=200, num_eigvals=16, epsilon=0.05, filter_mode=glf.FILTER_SMOOTH)
    with glf.Context(0) as ctx:
        uv = torch.from_numpy(np.ascontiguousarray(yuv[:, :, 1:].transpose(2, 0, 1), dtype=np.float32)).to(ctx.device)
        _, zf, so, _ = ctx.image_processing_signals(ctx.to_device(luma), uv, opt, want_float=True)
        zy, so = zf.cpu().numpy().astype(np.float64), so.cpu().numpy().astype(np.float64)
        _, zc, info = _whole(ctx, rgb, opt)
    luma_rgb = np.stack([zy, so[0], so[1]], axis=2) @ np.linalg.inv(Y).T
    s_in, s_luma, s_rgb = _step(rgb.astype(np.float64)), _step(luma_rgb), _step(zc.transpose(1, 2, 0))
    print("isoluminant step sharpness: input %.3f, luma graph + chroma %.3f, colour graph %.3f" % (s_in, s_luma, s_rgb))
    assert s_rgb > 0.7 * s_in
    assert s_luma < 0.5 * s_rgb


def test_2048_sampled_rows_against_numpy():
    """At 2048^2 (about 10 500 samples) the stage path's Phi rows of sampled pixels against numpy's extension of its Phi_A."""
    n = 2048
    rgb = _rgb_image(n, n, seed=11)
    idx = glf.Sampling(n, n, int(n * n * 0.0025))
    with glf.Context(0) as ctx:
        d_rgb = torch.from_numpy(rgb).to(ctx.device)
        _, K_B = ctx.ComputeAffinityMatrices(d_rgb, idx, want_KA=False, kernel=glf.KERNEL_BILATERAL_RGB, h_loc=H_LOC, h_val=H_VAL)
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
        for k, px in enumerate(pix):
            col = np.empty(16, dtype=np.float32)
            full = np.empty((1, phi_r.ld), dtype=np.float32)
            glf._lib.glf_memcpy_d2h(ctx._ctx, full.ctypes.data_as(glf.C.c_void_p), glf.C.c_void_p(phi_r.data + 4 * int(px) * phi_r.ld),
                                    glf.C.c_size_t(full.nbytes))
            col[:] = full[0, :16]
            rows[k] = col
        ctx.destroy(K_B, L_A, vecs, vals, pinv, phi_sf, phi_r)
    # the degree of a few samples and the extension of the sampled rows, in fp64
    sel = np.arange(0, len(idx), max(1, len(idx) // 24))
    np.testing.assert_allclose(deg[sel], ref.degree(rgb, idx[sel], H_LOC, H_VAL, chunk=1 << 20), rtol=1e-6)
    want = ref.phi_rows(rgb, idx, pix, phi_A, lam, alpha, H_LOC, H_VAL)
    assert _rel(rows, want) <= 1e-5


def test_grey_call_after_colour_call_is_unchanged():
    g = glf.synth_image(96, 80, seed=4)
    rgb = _rgb_image(80, 96, seed=2)
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05)
    with glf.Context(0) as fresh:
        out0, zf0, _ = fresh.image_processing(fresh.to_device(g), opt, want_float=True)
        out0, zf0 = out0.cpu().numpy(), zf0.cpu().numpy()
    with glf.Context(0) as ctx:
        _whole(ctx, rgb, opt)
        out1, zf1, _ = ctx.image_processing(ctx.to_device(g), opt, want_float=True)
        np.testing.assert_array_equal(out1.cpu().numpy(), out0)
        np.testing.assert_array_equal(zf1.cpu().numpy().view(np.int32), zf0.view(np.int32))


def test_debug_pool_colour_run(monkeypatch):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    rgb = _rgb_image(72, 90, seed=8)
    for mode in ("reference", "sharpen"):
        opt = glf.default_options(num_samples=80, num_eigvals=8, epsilon=0.05, filter_mode=MODES[mode])
        with glf.Context(0) as ctx:
            out, zf, info = _whole(ctx, rgb, opt)
            assert ctx.debug_violations() == 0
        assert np.isfinite(zf).all() and np.isfinite(info["eigvals"]).all()


def test_invalid_and_unsupported_with_a_live_context():
    rgb = _rgb_image(32, 40, seed=1)
    with glf.Context(0) as ctx:
        d = torch.from_numpy(rgb).to(ctx.device)
        for kernel in (glf.KERNEL_PHOTOMETRIC, glf.KERNEL_SPATIAL, glf.KERNEL_NLM):
            with pytest.raises(glf.GlfError) as e:
                ctx.image_processing_rgb(d, glf.default_options(num_samples=30, num_eigvals=4, kernel=kernel))
            assert e.value.status == glf.ERR_UNSUPPORTED
        with pytest.raises(glf.GlfError) as e:           # the grey entry point never reads RGB bytes as grey
            ctx.image_processing(ctx.to_device(rgb[:, :, 0].copy()), glf.default_options(num_samples=30, num_eigvals=4,
                                                                                          kernel=glf.KERNEL_BILATERAL_RGB))
        assert e.value.status == glf.ERR_UNSUPPORTED
        C = glf.C
        out = torch.zeros_like(d)
        rc = glf._lib.glf_image_processing_rgb(ctx._ctx, None, None, 40, 32, C.c_void_p(out.data_ptr()), None, None, None)
        assert rc == glf.ERR_INVALID
        rc = glf._lib.glf_image_processing_rgb(ctx._ctx, None, C.c_void_p(d.data_ptr()), 40, 32, None, None, None, None)
        assert rc == glf.ERR_INVALID
        o, _, info = ctx.image_processing_rgb(d, glf.default_options(num_samples=30, num_eigvals=4, kernel=glf.KERNEL_BILATERAL_RGB))
        assert o.shape == (32, 40, 3) and info["m"] == 4
