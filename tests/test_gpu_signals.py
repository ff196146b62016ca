"""Joint filtering (glf_image_processing_signals): float planes go through the guide image's graph filter.

The guide's outputs (u8 image, float z, eigenvalues) must be bit-identical to the plain glf_image_processing call on every
path; each plane s must come out as (1 - ysub) s + gain Phi w_s, w_s = f(Pi) Phi^T s, checked against the fp64 oracle's
Phi built from the GPU's own eigenpairs. A plane's result does not depend on the other planes, and the operator is linear."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import oracle as orc  # noqa: E402

from test_gpu_multi import _env_paths  # noqa: E402

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
YUV_FROM_RGB = np.array([[0.299, 0.587, 0.114], [-0.14714119, -0.28886916, 0.43601035], [0.61497538, -0.51496512, -0.10001026]])
MODES = {"reference": glf.FILTER_REFERENCE, "poc": glf.FILTER_POC, "smooth": glf.FILTER_SMOOTH, "sharpen": glf.FILTER_SHARPEN}
# rel-L2 of the planes' correction z - (1 - ysub) s against the fp64 oracle fed the GPU's eigenpairs
CORR_TOL = 1e-5


def _planes(h, w, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 40.0, (h, w))                                  # signed
    b = np.linspace(-3.0, 7.0, h * w).reshape(h, w) ** 2               # smooth, positive
    return np.stack([a, b]).astype(np.float32)


def _run(ctx, img, opt, sig):
    d_img = ctx.to_device(img)
    d_sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32)).to(ctx.device)
    out, zf, so, info = ctx.image_processing_signals(d_img, d_sig, opt, want_float=True)
    return out.cpu().numpy(), zf.cpu().numpy(), so.cpu().numpy(), info


def _expected_corr(img, opt, info, phi_A, sig):
    """The fp64 correction z - (1 - ysub) s of each plane: gain Phi f(Pi) Phi^T s with Phi = the oracle's Nystroem extension of
    the GPU's Phi_A (raster order)."""
    h, w = img.shape
    idx = glf.Sampling(w, h, int(opt.num_samples))
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    m = lam.size
    phi = orc.permutation(orc.nystroem(img, idx, info["alpha"], phi_A[:, :m].T.astype(np.float64), lam), idx)   # (m, N)
    mode = int(opt.filter_mode)
    f = {glf.FILTER_REFERENCE: lam, glf.FILTER_POC: -(lam + 5.0), glf.FILTER_SMOOTH: 1.0 - lam}[mode]
    gain = float(opt.gain) if mode == glf.FILTER_REFERENCE else 1.0
    s = sig.reshape(sig.shape[0], -1).astype(np.float64)
    return (gain * ((f[:, None] * (phi @ s.T)).T @ phi)).reshape(sig.shape)


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


@pytest.mark.parametrize("paths", ["direct", "grid", "rank", "band"])
def test_guide_outputs_bit_identical_to_plain_call(paths, monkeypatch):
    _env_paths(monkeypatch, paths)
    img = glf.synth_image(96, 80, seed=4)
    sig = _planes(80, 96)
    with glf.Context(0) as ctx:
        for name, mode in MODES.items():
            opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, filter_mode=mode)
            out1, zf1, info1 = ctx.image_processing(ctx.to_device(img), opt, want_float=True)
            out, zf, so, info = _run(ctx, img, opt, sig)
            np.testing.assert_array_equal(out, out1.cpu().numpy(), err_msg=name)
            np.testing.assert_array_equal(zf.view(np.int32), zf1.cpu().numpy().view(np.int32), err_msg=name)
            np.testing.assert_array_equal(info["eigvals"], info1["eigvals"], err_msg=name)
            assert info["filter_fused"] == info1["filter_fused"]
            assert np.isfinite(so).all(), name


def _luma_chroma():
    rgb = glf.read_png_rgb(__import__("os").path.join(ROOT, "tests", "golden", "pixel_mountains.png")).astype(np.float64)
    yuv = rgb @ YUV_FROM_RGB.T
    luma = np.clip(np.floor(yuv[:, :, 0] + 0.5), 0, 255).astype(np.uint8)
    return luma, yuv


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", ["mountains", "synth"])
def test_planes_against_fp64_oracle(case, fused):
    if case == "mountains":
        img, yuv = _luma_chroma()
        h, w = img.shape
        sig = np.stack([yuv[:, :, 1], yuv[:, :, 2], _planes(h, w, 3)[0]]).astype(np.float32)
        ns, m = 300, 16
    else:
        img = glf.synth_image(96, 80, seed=4)
        h, w = img.shape
        sig = np.concatenate([_planes(h, w, 5), img[None].astype(np.float32)])
        ns, m = 60, 8
    with glf.Context(0) as ctx:
        ctx.set_tuning(MV_PATH="band", NYS_PATH="band", DEG_PATH="grid", NO_FUSED_FILTER=None if fused else "1")
        for mode in (glf.FILTER_REFERENCE, glf.FILTER_SMOOTH, glf.FILTER_POC):
            opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1, filter_mode=mode)
            _, _, cinfo = ctx.image_processing(ctx.to_device(img), opt, capture=True)
            out, zf, so, info = _run(ctx, img, opt, sig)
            assert info["filter_fused"] == (1 if fused else 0)
            np.testing.assert_array_equal(info["eigvals"], cinfo["eigvals"])
            ref = _expected_corr(img, opt, info, cinfo["capture"]["phi_A"].cpu().numpy(), sig)
            ysub = 1.0 if mode == glf.FILTER_SMOOTH else 0.0
            corr = so.astype(np.float64) - (1.0 - ysub) * sig
            for k in range(sig.shape[0]):
                r = _rel(corr[k], ref[k])
                print("oracle %s fused=%s mode=%d plane %d: rel-L2 of the correction %.2e" % (case, fused, mode, k, r))
                assert r <= CORR_TOL, (k, r)
            if case == "synth":   # s = the image: the guide's own float z
                zcorr = zf.astype(np.float64) - (1.0 - ysub) * img
                r = _rel(corr[-1], zcorr)
                print("s = image, fused=%s mode=%d: rel-L2 against the guide's correction %.2e" % (fused, mode, r))
                assert r <= CORR_TOL, r


def test_planes_independent_and_linear():
    img = glf.synth_image(96, 80, seed=4)
    s1, s2 = _planes(80, 96, 7)
    a, b = 0.75, -2.5
    with glf.Context(0) as ctx:
        for paths in ("band", "direct"):
            ctx.set_tuning(NYS_PATH=paths, DEG_PATH="direct" if paths == "direct" else "grid",
                           MV_PATH={"direct": "dense", "band": "band"}[paths])
            opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05)
            _, _, both, _ = _run(ctx, img, opt, np.stack([s1, s2]))
            _, _, one, _ = _run(ctx, img, opt, s1[None])
            _, _, two, _ = _run(ctx, img, opt, s2[None])
            np.testing.assert_array_equal(both[0].view(np.int32), one[0].view(np.int32))
            np.testing.assert_array_equal(both[1].view(np.int32), two[0].view(np.int32))
            comb = (a * s1.astype(np.float64) + b * s2).astype(np.float32)
            _, _, lin, _ = _run(ctx, img, opt, comb[None])
            corr = lambda z, s: z.astype(np.float64) - s
            r = _rel(corr(lin[0], comb), a * corr(both[0], s1) + b * corr(both[1], s2))
            print("linearity (%s): rel %.2e" % (paths, r))
            assert r <= 1e-5, r


def test_fused_band_path_at_2048():
    """The default path at scale: the guide bit-identical to the plain call. The planes: Phi's sampled rows (the captured run's,
    the same contraction the planes use) against the fp64 oracle rows fed the GPU's Phi_A (test_gpu_large's PHI_TOL), and each
    plane's correction on those rows against gain Phi_rows (f(Pi) c_s) with c_s = Phi^T s in fp64 over the captured Phi."""
    size, m = 2048, 64
    img = glf.synth_image(size, size, seed=0)
    ns = int(size * size * 0.005)
    sig = _planes(size, size, 11)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1)
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        out1, zf1, info1 = ctx.image_processing(d_img, opt, want_float=True)
        out, zf, so, info = _run(ctx, img, opt, sig)
        assert info["filter_fused"] == 1 and info1["filter_fused"] == 1 and info["nystroem_path"] == 4
        np.testing.assert_array_equal(out, out1.cpu().numpy())
        np.testing.assert_array_equal(zf.view(np.int32), zf1.cpu().numpy().view(np.int32))
        np.testing.assert_array_equal(info["eigvals"], info1["eigvals"])
        del out1, zf1
        _, _, cinfo = ctx.image_processing(d_img, opt, capture=True)
        cap = cinfo["capture"]
        np.testing.assert_array_equal(cinfo["eigvals"], info["eigvals"])
        phi = cap["phi"][:, :m].double()                                        # [N, m] raster rows
        c = (phi.T @ torch.from_numpy(sig.reshape(2, -1)).to(phi.device).double().T).cpu().numpy()   # (m, 2)
        rows = (0, size // 2 + 3, size - 1)
        phi_rows = {r0: phi.view(size, size, m)[r0].cpu().numpy() for r0 in rows}
        del phi, cap
        torch.cuda.empty_cache()
        lam = np.asarray(info["eigvals"], dtype=np.float64)
        idx = glf.Sampling(size, size, ns)
        phi_A = cinfo["capture"]["phi_A"][:, :m].cpu().numpy().astype(np.float64).T
        for r0 in rows:
            ref_rows = orc.nystroem_rows(img, idx, info["alpha"], phi_A, lam, r0, r0 + 1)   # (m, w) fp64
            err = float(np.abs(phi_rows[r0].T - ref_rows).max() / np.abs(ref_rows).max())
            assert err <= 2e-5, (r0, err)
            got = so[:, r0, :].astype(np.float64) - sig[:, r0, :]
            for k in range(2):
                ref = float(opt.gain) * (phi_rows[r0] @ (lam * c[:, k]))
                ref_orc = float(opt.gain) * (ref_rows.T @ (lam * c[:, k]))
                r, r_orc = _rel(got[k], ref), _rel(got[k], ref_orc)
                # the float plane z resolves its correction to ulp(z) only: a zero-mean noise plane (|z| ~ 40) low-passed onto
                # 64 eigenvectors of 4M pixels has a correction of ~1e-2, so z's rounding (<= 2^-24 |z| per pixel) dominates
                rms = lambda a: float(np.sqrt(np.mean(np.square(a))))
                bound = CORR_TOL * rms(ref) + 2.0 ** -24 * rms(so[k, r0, :])
                bound_orc = CORR_TOL * rms(ref_orc) + 2.0 ** -24 * rms(so[k, r0, :])
                print("2048^2 row %d plane %d: Phi rows %.2e, correction rel %.2e (oracle rows %.2e), rms err %.2e <= %.2e, "
                      "against the oracle rows %.2e <= %.2e" % (r0, k, err, r, r_orc, rms(got[k] - ref), bound, rms(got[k] - ref_orc),
                                                                 bound_orc), flush=True)
                assert rms(got[k] - ref) <= bound, (r0, k, r)
                assert rms(got[k] - ref_orc) <= bound_orc, (r0, k, r_orc)     # the plane's rows against the fp64 oracle itself


def test_unsupported_and_invalid():
    img = glf.synth_image(64, 48, seed=1)
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        sig = torch.zeros((1, 48, 64), dtype=torch.float32, device=ctx.device)
        with pytest.raises(glf.GlfError) as e:   # the panel path (more than 256 eigenpairs)
            ctx.image_processing_signals(d_img, sig, glf.default_options(num_samples=400, num_eigvals=300))
        assert e.value.status == glf.ERR_UNSUPPORTED
        out = torch.zeros((48, 64), dtype=torch.uint8, device=ctx.device)
        opt = glf.default_options(num_samples=60, num_eigvals=8)
        lib = glf._lib
        for nsig, ps, po in ((0, sig.data_ptr(), sig.data_ptr()), (5, sig.data_ptr(), sig.data_ptr()),
                             (1, None, sig.data_ptr()), (1, sig.data_ptr(), None)):
            rc = lib.glf_image_processing_signals(ctx._ctx, glf.C.byref(opt), glf.C.c_void_p(d_img.data_ptr()), 64, 48, nsig,
                                                  glf.C.c_void_p(ps), glf.C.c_void_p(po), glf.C.c_void_p(out.data_ptr()), None, None, None)
            assert rc == glf.ERR_INVALID, (nsig, ps, po)
        # the context still works afterwards
        _, _, so, _ = ctx.image_processing_signals(d_img, sig, opt)
        assert torch.isfinite(so).all()
