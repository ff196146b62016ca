"""The band form of the 16-bit and colour bilateral kernels (tuning key PIX_BAND; k_band<.., PixGen::U16 | PixGen::Rgb>): the
Nystroem stage and the operator of the eigen-solve take the band form wherever the grey kernel would, with the photometric factor
generated per entry (dist2 of the pixel policy, one v_exp_f32) instead of gathered from the 256-level table.

References: the fp64 numpy restatements tests/u16_ref.py and tests/rgb_ref.py. Every tolerance is one the suite already holds for
the same comparison on another route: 1e-5 relative L2 for Phi and the corrections (test_stages_against_numpy /
test_whole_path_against_numpy of both format suites), 2e-5 of max |Phi| between forms of different arithmetic
(test_nystroem_paths_agree), rtol 1e-5 for eigenvalues between routes (the 8-bit / grey equivalence tests), rtol 1e-6 for D_A.
With the key off, or where the band form declines (random sampler, more than 64 eigenpairs, the f32 contraction, NYS_PATH grid /
rank / direct), the calls are the entry-by-entry route bit for bit; a grey call never sees the key."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import rgb_ref  # noqa: E402
import u16_ref  # noqa: E402
from test_gpu_rgb import _rgb_image  # noqa: E402
from test_gpu_u16 import _u16_image  # noqa: E402

MODES = {"reference": glf.FILTER_REFERENCE, "poc": glf.FILTER_POC, "smooth": glf.FILTER_SMOOTH, "sharpen": glf.FILTER_SHARPEN}
H_LOC = 40.0


class _Fmt:
    """What differs between the two formats in a test: the image, the reference module, the kernel, h_val, the entry point."""

    def __init__(self, name):
        self.name = name
        self.u16 = name == "u16"
        self.ref = u16_ref if self.u16 else rgb_ref
        self.kernel = glf.KERNEL_BILATERAL_U16 if self.u16 else glf.KERNEL_BILATERAL_RGB
        self.h_val = 30.0 * 257.0 if self.u16 else 30.0
        self.vmax = 65535 if self.u16 else 255

    def image(self, h, w, seed):
        return _u16_image(h, w, seed) if self.u16 else _rgb_image(h, w, seed)

    def dev(self, ctx, img):
        return torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)

    def options(self, **kw):
        return glf.default_options(h_val=self.h_val, **kw)

    def whole(self, ctx, img, opt, capture=False):
        fn = ctx.image_processing_u16 if self.u16 else ctx.image_processing_rgb
        out, zf, info = fn(self.dev(ctx, img), opt, want_float=True, capture=capture)
        return out.cpu().numpy(), zf.cpu().numpy(), info

    def planes(self, img):
        """The image's channels as float64 planes [nch, N]."""
        return img.reshape(1, -1).astype(np.float64) if self.u16 else img.reshape(-1, 3).T.astype(np.float64)

    def corrections(self, img, phi, lam, mode, gain):
        if self.u16:
            return self.ref.correction(img, phi, lam, mode, gain)[None, :]
        return np.asarray(self.ref.corrections(img, phi, lam, mode, gain))

    def phi_rows(self, img, idx, pixels, phi_A, lam, alpha, chunk=8192):
        pixels = np.asarray(pixels, dtype=np.int64)
        return np.concatenate([self.ref.phi_rows(img, idx, pixels[k:k + chunk], phi_A, lam, alpha, H_LOC, self.h_val)
                               for k in range(0, pixels.size, chunk)], axis=0)


FMTS = {"u16": _Fmt("u16"), "rgb": _Fmt("rgb")}
fmt_param = pytest.mark.parametrize("fmt", list(FMTS))


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def _route(info):
    return info["nystroem_path"], info["matvec_path"], info["filter_fused"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _read_rows(ctx, mat, rows, m):
    """Rows `rows` of a dense device matrix, the first m columns."""
    out = np.empty((len(rows), m))
    full = np.empty((1, mat.ld), dtype=np.float32)
    for k, r in enumerate(rows):
        glf._lib.glf_memcpy_d2h(ctx._ctx, full.ctypes.data_as(glf.C.c_void_p), glf.C.c_void_p(mat.data + 4 * int(r) * mat.ld),
                                glf.C.c_size_t(full.nbytes))
        out[k] = full[0, :m]
    return out


# ---- 1. the Nystroem stage, the same inputs through both routes -------------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("w,h,ns", [(128, 96, 150), (450, 300, 1350), (77, 200, 60)])
def test_nystroem_stage_band_against_numpy_and_entrywise(fmt, w, h, ns):
    f = FMTS[fmt]
    m = 8
    img = f.image(h, w, seed=w)
    idx = glf.Sampling(w, h, ns)
    _, _, _, LA = f.ref.laplacian(img, idx, H_LOC, f.h_val)
    vals, vecs = np.linalg.eigh(LA)                      # LAPACK eigenpairs of the fp64 L_A, the m smallest
    lam, phi_A = vals[:m], vecs[:, :m]
    got = {}
    with glf.Context(0) as ctx:
        _, K_B = ctx.ComputeAffinityMatrices(f.dev(ctx, img), idx, want_KA=False, kernel=f.kernel, h_loc=H_LOC, h_val=f.h_val)
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
    want = f.phi_rows(img, idx, np.arange(w * h), phi_A, lam, alpha)
    e_band, e_entry = _rel(got["band"], want), _rel(got["entrywise"], want)
    d = float(np.abs(got["band"] - got["entrywise"]).max() / np.abs(got["entrywise"]).max())
    print("%s %dx%d: Phi rel-L2 band %.2e entrywise %.2e, max |band - entrywise| / max |Phi| %.2e" % (fmt, w, h, e_band, e_entry, d))
    assert e_band <= 1e-5 and e_entry <= 1e-5
    assert d <= 2e-5
    assert np.any(got["band"] != got["entrywise"])      # (another arithmetic: the key did select another kernel)


# ---- 2. operator and whole path, small -------------------------------------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("mode", list(MODES))
def test_whole_path_small_forced_band(fmt, mode):
    """The checks of test_whole_path_against_numpy (both format suites) at their tolerances on the route (4, 4, 0), and the
    eigenvalues against the key-off run's.

    The correction is read back from z, which the API stores in f32. On this image that storage alone is 1.07e-5 relative L2 of the
    red plane's reference-filter correction (rms 0.31 levels under z of 60 - 250; computed from the fp64 restatement with LAPACK
    eigenpairs, no GPU involved; 7.9e-6 for the 16-bit image, 3 - 4e-6 at the 61 x 47 of the format suites), and the first run here
    measured 1.08e-5 there with Phi at 6.8e-9: the 1e-5 bound was being spent on the output format, whatever the route. numpy's
    z = x + c therefore goes through the same f32 storage before the corrections are compared; the bound is unchanged and every
    error of the route still shows (a deviation below one ulp of z moves the stored value with probability deviation / ulp)."""
    f = FMTS[fmt]
    w, h, ns, m = 96, 80, 120, 8
    img = f.image(h, w, seed=3)
    opt = f.options(num_samples=ns, num_eigvals=m, epsilon=1e-3, filter_mode=MODES[mode], sampling=glf.SAMPLING_UNIFORM)
    idx = glf.Sampling(w, h, ns)
    with glf.Context(0) as ctx:
        _, _, info_off = f.whole(ctx, img, opt)
        ctx.set_tuning(PIX_BAND="1", NYS_PATH="band", MV_PATH="band")
        out, zf, info = f.whole(ctx, img, opt, capture=True)
        cap = info["capture"]
        phi_A = cap["phi_A"].cpu().numpy()[:len(idx), :m].astype(np.float64)
        phi = cap["phi"].cpu().numpy()[:, :m].astype(np.float64)
    zf = zf.astype(np.float64)
    assert _route(info_off) == (0, 0, 0)
    assert _route(info) == (4, 4, 0)
    assert info["contraction"] == glf.CONTRACT_F16_SPLIT
    assert info["p"] == len(idx) and info["m"] == m and info["nystroem_evaluated"] > 0
    _, D, alpha, LA = f.ref.laplacian(img, idx, H_LOC, f.h_val)
    np.testing.assert_allclose(cap["degree"], D, rtol=1e-6)
    lam = np.asarray(info["eigvals"], dtype=np.float64)
    for j in range(m):
        v = phi_A[:, j] / np.linalg.norm(phi_A[:, j])
        assert np.linalg.norm(LA @ v - lam[j] * v) <= 2e-2 * max(lam[j], 1e-3), (j, lam[j])
    np.testing.assert_allclose(lam, info_off["eigvals"], rtol=1e-5)
    want_phi = f.phi_rows(img, idx, np.arange(w * h), phi_A, lam, info["alpha"])
    e_phi = _rel(phi, want_phi)
    print("%s %s: Phi rel-L2 %.2e" % (fmt, mode, e_phi))
    assert e_phi <= 1e-5
    ysub = 1.0 if MODES[mode] >= glf.FILTER_SMOOTH else 0.0
    x = f.planes(img)
    corr = zf.reshape(x.shape[0], -1) - (1.0 - ysub) * x
    want = f.corrections(img, phi, lam, MODES[mode], float(opt.gain))
    want_stored = ((1.0 - ysub) * x + want).astype(np.float32).astype(np.float64) - (1.0 - ysub) * x
    for k in range(x.shape[0]):
        err = float(np.linalg.norm(corr[k] - want_stored[k]) / np.linalg.norm(want[k]))
        print("%s %s plane %d: rel-L2 of the correction %.2e (against numpy's before its f32 storage: %.2e)" % (fmt, mode, k, err, _rel(corr[k], want[k])))
        assert err <= 1e-5, (k, err)
    # the output is the clamped truncation x + floor(c): at most one level below the truncation of the float z, never above
    zt = np.clip(np.floor(zf if f.u16 else zf.reshape(3, h, w).transpose(1, 2, 0)), 0, f.vmax)
    d = out.astype(np.int64) - zt
    assert d.max() <= 0 and d.min() >= -1


# ---- 3. the benchmark tile: 1024^2, 0.5 % (p = 5329), m = 64 --------------------------------------------------------------------

@fmt_param
def test_tile_1024_routes_rows_and_noskip(fmt):
    f = FMTS[fmt]
    n, m = 1024, 64
    img = f.image(n, n, seed=7)
    opt = f.options(num_samples=int(n * n * 0.005), num_eigvals=m, epsilon=0.1)
    idx = glf.Sampling(n, n, int(n * n * 0.005))
    g = glf.synth_image(n, n, seed=5)
    with glf.Context(0) as ctx:
        _, _, info_grey = ctx.image_processing(ctx.to_device(g), glf.default_options(num_samples=int(n * n * 0.005), num_eigvals=m, epsilon=0.1))
        ctx.set_tuning(PIX_BAND="1")
        _, _, info_a = f.whole(ctx, img, opt)                       # (a) default tuning plus the key
        ctx.set_tuning(MV_PATH="band")
        out_b, zf_b, info_b = f.whole(ctx, img, opt, capture=True)    # (b) the operator in band form as well
        phi_A = info_b["capture"]["phi_A"].cpu().numpy()[:len(idx), :m].astype(np.float64)
        rng = np.random.default_rng(0)
        pix = np.sort(np.concatenate([rng.choice(n * n, 48, replace=False), rng.choice(idx, 48, replace=False)])).astype(np.int64)
        rows = info_b["capture"]["phi"][torch.from_numpy(pix).to(ctx.device)].cpu().numpy()[:, :m].astype(np.float64)
        del info_b["capture"]
        ctx.set_tuning(BAND_NOSKIP="1")
        out_c, zf_c, info_c = f.whole(ctx, img, opt)
    assert info_a["p"] == 5329 == len(idx)
    assert info_a["nystroem_path"] == 4 and info_a["matvec_path"] == info_grey["matvec_path"] == 0 and info_a["filter_fused"] == 0
    assert _route(info_b) == (4, 4, 0) and info_b["contraction"] == glf.CONTRACT_F16_SPLIT
    lam = np.asarray(info_b["eigvals"], dtype=np.float64)
    want = f.phi_rows(img, idx, pix, phi_A, lam, info_b["alpha"])
    err = _rel(rows, want)
    print("%s 1024^2: Phi rows rel-L2 %.2e; nystroem_evaluated %.4e with the skips, %.4e without; stages (b) eigen %.2f nystroem %.2f ms"
          % (fmt, err, info_b["nystroem_evaluated"], info_c["nystroem_evaluated"], info_b["ms_eigen"], info_b["ms_nystroem"]))
    assert err <= 1e-5
    assert _route(info_c) == (4, 4, 0)
    np.testing.assert_array_equal(out_c, out_b)
    np.testing.assert_array_equal(_bits(zf_c), _bits(zf_b))
    np.testing.assert_array_equal(info_c["eigvals"], info_b["eigvals"])
    assert info_c["nystroem_evaluated"] > info_b["nystroem_evaluated"]


# ---- 4. / 6. 2048^2: sampled rows on the stage path, the automatic route, and L_A not stored ------------------------------------

@fmt_param
def test_2048_sampled_rows_stage_path_with_the_key(fmt):
    f = FMTS[fmt]
    n, m = 2048, 16
    img = f.image(n, n, seed=11)
    idx = glf.Sampling(n, n, int(n * n * 0.0025))
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1")
        _, K_B = ctx.ComputeAffinityMatrices(f.dev(ctx, img), idx, want_KA=False, kernel=f.kernel, h_loc=H_LOC, h_val=f.h_val)
        L_A, L_B, alpha = ctx.ComputeLaplacianMatrix(None, K_B)
        vecs, vals, _ = ctx.InversePowerIteration(L_A, m, epsilon=0.1)
        lam = ctx.mat_to_numpy(vals).astype(np.float64)
        phi_A = ctx.mat_to_numpy(vecs)[:len(idx)].astype(np.float64)
        pinv = ctx.InverseDiagMat(vals)
        phi_sf = ctx.Nystroem(L_B, vecs, pinv)
        phi_r = ctx.Permutation(phi_sf, idx)
        pix = np.sort(np.random.default_rng(0).choice(n * n, 48, replace=False))
        rows = _read_rows(ctx, phi_r, pix, m)
        ctx.reset_tuning()
        phi_sf0 = ctx.Nystroem(L_B, vecs, pinv)            # the key off: the entry-by-entry kernel on the same inputs
        phi_r0 = ctx.Permutation(phi_sf0, idx)
        rows0 = _read_rows(ctx, phi_r0, pix, m)
        ctx.destroy(K_B, L_A, vecs, vals, pinv, phi_sf, phi_r, phi_sf0, phi_r0)
    want = f.phi_rows(img, idx, pix, phi_A, lam, alpha)
    print("%s 2048^2 stage path: Phi rows rel-L2 %.2e (key on), %.2e (key off)" % (fmt, _rel(rows, want), _rel(rows0, want)))
    assert _rel(rows, want) <= 1e-5
    assert np.any(rows != rows0)                            # (the key selected the band kernel: another arithmetic)


@fmt_param
def test_2048_automatic_route_and_la_not_stored(fmt):
    """2048^2 at 0.5 % (20 971 samples asked for, the 146 x 146 grid of p = 21 316 realised): default tuning plus the key runs
    (4, 4, 0), and the context's pool -- every work buffer of the call, released and cached at its end -- stays below the 4 p^2
    bytes of a stored L_A (1.8 GB); the key-off call on a fresh context holds at least that."""
    f = FMTS[fmt]
    n = 2048
    img = f.image(n, n, seed=13)
    opt = f.options(num_samples=int(n * n * 0.005), num_eigvals=16, epsilon=0.1)
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1")
        _, zf_on, info_on = f.whole(ctx, img, opt)
        bytes_on = ctx.cached_bytes()
    with glf.Context(0) as ctx:
        _, zf_off, info_off = f.whole(ctx, img, opt)
        bytes_off = ctx.cached_bytes()
    p = info_on["p"]
    assert p == info_off["p"] == len(glf.Sampling(n, n, int(n * n * 0.005))) and p >= 16384
    assert _route(info_on) == (4, 4, 0) and _route(info_off) == (0, 0, 0)
    print("%s 2048^2: pool %.3f GB with the key, %.3f GB without (4 p^2 = %.3f GB); eigen + nystroem + laplacian %.1f ms against %.1f ms"
          % (fmt, bytes_on / 1e9, bytes_off / 1e9, 4.0 * p * p / 1e9, info_on["ms_eigen"] + info_on["ms_nystroem"] + info_on["ms_laplacian"],
             info_off["ms_eigen"] + info_off["ms_nystroem"] + info_off["ms_laplacian"]))
    assert bytes_on < 4 * p * p
    assert bytes_off >= 4 * p * p
    assert np.isfinite(zf_on).all() and np.isfinite(info_on["eigvals"]).all()


# ---- 5. the declines are today's behaviour -------------------------------------------------------------------------------------------

# 1056 x 256 at h_loc = 10 (radius 53 px): wide enough, and the band narrow enough, for the automatic band form -- the key alone
# takes it there (test_the_key_alone_...), so each decline below is the condition's doing
DECL_W, DECL_H = 1056, 256
DECL_KW = dict(num_samples=600, num_eigvals=8, epsilon=0.05, h_loc=10.0)

DECLINES = {
    "random-sampler": (dict(sampling=glf.SAMPLING_RANDOM), {}, None),
    "m-100": (dict(num_eigvals=100), {}, None),
    "f32-contraction": ({}, {}, glf.CONTRACT_F32_MFMA),
    "nys-grid": ({}, dict(NYS_PATH="grid", MV_PATH="dense"), None),
    "nys-rank": ({}, dict(NYS_PATH="rank", MV_PATH="dense"), None),
    "nys-direct": ({}, dict(NYS_PATH="direct", MV_PATH="dense"), None),
}


@fmt_param
@pytest.mark.parametrize("case", list(DECLINES))
def test_declines_are_the_entrywise_route_bit_for_bit(fmt, case):
    f = FMTS[fmt]
    okw, tune, contraction = DECLINES[case]
    img = f.image(DECL_H, DECL_W, seed=6)
    kw = dict(DECL_KW)
    kw.update(okw)
    opt = f.options(**kw)
    res = []
    for key in (None, "1"):
        with glf.Context(0) as ctx:
            if contraction is not None:
                ctx.set_contraction(contraction)
            ctx.set_tuning(PIX_BAND=key, **tune)
            res.append(f.whole(ctx, img, opt))
    (out0, zf0, info0), (out1, zf1, info1) = res
    assert _route(info0) == (0, 0, 0) and _route(info1) == (0, 0, 0), case
    assert info1["contraction"] == glf.CONTRACT_F32_MFMA
    np.testing.assert_array_equal(out1, out0)
    np.testing.assert_array_equal(_bits(zf1), _bits(zf0))
    np.testing.assert_array_equal(info1["eigvals"], info0["eigvals"])


@fmt_param
def test_the_key_alone_takes_the_band_nystroem_on_the_declines_image(fmt):
    """The counterpart of the declines: on the same image and options the key with nothing in its way does take the band form."""
    f = FMTS[fmt]
    img = f.image(DECL_H, DECL_W, seed=6)
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1")
        _, _, info = f.whole(ctx, img, f.options(**DECL_KW))
    assert _route(info) == (4, 0, 0) and info["contraction"] == glf.CONTRACT_F16_SPLIT


# ---- 7. grey is untouched ----------------------------------------------------------------------------------------------------------------

def test_grey_calls_never_see_the_key():
    n = 1024
    g = glf.synth_image(n, n, seed=5)
    opt = glf.default_options(num_samples=int(n * n * 0.005), num_eigvals=64, epsilon=0.1)

    def grey(ctx):
        out, zf, info = ctx.image_processing(ctx.to_device(g), opt, want_float=True)
        return out.cpu().numpy(), zf.cpu().numpy(), info

    with glf.Context(0) as ctx:
        out0, zf0, info0 = grey(ctx)
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1")
        first = grey(ctx)
        for f in FMTS.values():                              # a key-on 16-bit and colour call on the same context, then grey again
            _, _, info = f.whole(ctx, f.image(DECL_H, DECL_W, seed=2), f.options(**DECL_KW))
            assert info["nystroem_path"] == 4
        second = grey(ctx)
    for out, zf, info in (first, second):
        assert _route(info) == _route(info0)
        np.testing.assert_array_equal(out, out0)
        np.testing.assert_array_equal(_bits(zf), _bits(zf0))
        np.testing.assert_array_equal(info["eigvals"], info0["eigvals"])


# ---- 9. the debug pool ------------------------------------------------------------------------------------------------------------------

@fmt_param
def test_debug_pool_key_on_run(fmt, monkeypatch):
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    f = FMTS[fmt]
    img = f.image(72, 90, seed=8)
    opt = f.options(num_samples=80, num_eigvals=8, epsilon=0.05)
    with glf.Context(0) as ctx:
        ctx.set_tuning(PIX_BAND="1", NYS_PATH="band", MV_PATH="band")
        _, zf, info = f.whole(ctx, img, opt)
        assert ctx.debug_violations() == 0
    assert _route(info) == (4, 4, 0)
    assert np.isfinite(zf).all() and np.isfinite(info["eigvals"]).all()


def test_the_key_is_read_from_the_environment(monkeypatch):
    f = FMTS["u16"]
    monkeypatch.setenv("GLF_PIX_BAND", "1")
    monkeypatch.setenv("GLF_NYS_PATH", "band")
    monkeypatch.setenv("GLF_MV_PATH", "band")
    with glf.Context(0) as ctx:
        _, _, info = f.whole(ctx, f.image(72, 90, seed=8), f.options(num_samples=80, num_eigvals=8, epsilon=0.05))
    assert _route(info) == (4, 4, 0)
