"""The fused filter of the band form contracted with q = Psi w (k_band_vec, FILTER_FORM=vec: one column per plane instead of the
64 columns of Phi) on the shapes where its windows and masks can go wrong: a radius larger than the image (every window clipped by all
four borders, a last tile of 8 pixels, a last workgroup with waves without a row), m below the padded width of Psi, a narrow kernel
with a handful of samples per pixel, signal planes, the BAND_NOSKIP schedule, and an uneven row split over three ranks.

The correction z - (1 - ysub) y (and each plane's) is held to the project's rule ||got - want|| <= 1e-5 ||want|| + 2^-24 ||z|| twice:
against the fp64 oracle's Nystroem extension fed the run's own Phi_A, eigenvalues, alpha and c (a captured run of the same input),
and against the FILTER_FORM=phi run (k_band's epilogue). The 8-bit outputs of the two forms differ by at most 1 on at most 1e-4 of
the pixels; the oracle's correction must reach whole grey levels for that to say anything, which is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import oracle as orc  # noqa: E402

from conftest import psnr  # noqa: E402

CORR_TOL = 1e-5                       # (test_gpu_signals.py / test_gpu_pix_signals.py)
BAND = dict(NYS_PATH="band", MV_PATH="band", DEG_PATH="grid")
CLIPPED = dict(width=200, height=93, frac=0.02, h_loc=40.0, seed=7)      # radius 212 px > the image; 3 tiles + 8 px; 11 workgroups + 5 rows
NARROW = dict(width=512, height=384, frac=0.005, h_loc=6.0, seed=9)      # radius 32 px on a grid of pitch 14


def _image(width, height, frac, h_loc, seed):
    return glf.synth_image(width, height, seed=seed), int(width * height * frac)


def _planes(h, w, n, seed=3):
    rng = np.random.default_rng(seed)
    out = [rng.normal(0.0, 40.0, (h, w)), np.linspace(-3.0, 7.0, h * w).reshape(h, w) ** 2,
           np.cos(np.arange(h)[:, None] / 9.0) * np.arange(w)[None, :], rng.uniform(0.0, 255.0, (h, w))]
    return np.stack(out[:n]).astype(np.float32)


def _err(got, want):
    return float(np.linalg.norm((got - want).ravel())), float(np.linalg.norm(want.ravel()))


def _assert_rule(what, got, want, z):
    e, n = _err(got, want)
    bound = CORR_TOL * n + 2.0 ** -24 * float(np.linalg.norm(np.asarray(z, dtype=np.float64).ravel()))
    print("%s: ||got - want|| %.3e <= %.3e (||want|| %.3e)" % (what, e, bound, n), flush=True)
    assert e <= bound, (what, e, bound)


def _assert_stats(info):
    assert info["filter_fused"] == 1 and info["nystroem_path"] == 4
    assert info["nystroem_mfma_flops"] == 0 and info["nystroem_evaluated"] > 0
    assert info["rank_terms"] == 0, info["rank_terms"]   # k_band_vec ran, not the separable form (the default)


def _oracle_phi(img, ns, opt, cinfo):
    """fp64 Phi [m, N] in raster order (the sample pixels hold their rows of Phi_A) from the captured run's eigenpairs"""
    h, w = img.shape
    idx = glf.Sampling(w, h, ns)
    lam = np.asarray(cinfo["eigvals"], dtype=np.float64)
    prm = orc.default_params()
    prm.h_loc = float(opt.h_loc)
    phi_A = cinfo["capture"]["phi_A"].cpu().numpy()[:, :lam.size].astype(np.float64).T
    return orc.permutation(orc.nystroem(img, idx, cinfo["alpha"], phi_A, lam, prm=prm), idx), lam


def _pairs_inside(width, height, ns, h_loc):
    """(pixel, sample) pairs with dr^2 + dc^2 < D2 (band_plan.hpp's |dc| <= dcmax[dr]), counted exactly: what the kernel must at least
    evaluate. A window or a cap that lost a column at the circle's edge would pass every parity bound here, but not this count
    on the narrow kernel, where the schedule has little slack."""
    idx = glf.Sampling(width, height, ns).astype(np.int64)
    rows, cols = np.unique(idx // width), np.unique(idx % width)
    D2 = 40.5 / float(np.float32(1.4426950408889634 / (float(h_loc) * float(h_loc))))
    dr2 = (np.arange(height)[:, None] - rows[None, :]).astype(np.float64) ** 2          # [H, nr]
    dc2 = np.sort(((np.arange(width)[:, None] - cols[None, :]).astype(np.float64) ** 2).ravel())
    return int(np.searchsorted(dc2, (D2 - dr2).ravel(), side="left").sum())             # per (row, band row): the dc^2 < D2 - dr^2


def _guide_case(shape, m, mode=glf.FILTER_REFERENCE):
    img, ns = _image(**shape)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1, h_loc=shape["h_loc"], filter_mode=mode)
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        ctx.set_tuning(**BAND)
        _, _, cinfo = ctx.image_processing(d_img, opt, capture=True)
        res = {}
        for form in ("vec", "phi"):
            ctx.set_tuning(FILTER_FORM=form, **BAND)
            out, zf, info = ctx.image_processing(d_img, opt, want_float=True)
            res[form] = (out.cpu().numpy(), zf.cpu().numpy().astype(np.float64), info)
    (out_v, zf_v, info_v), (out_p, zf_p, info_p) = res["vec"], res["phi"]
    _assert_stats(info_v)
    pairs = _pairs_inside(shape["width"], shape["height"], ns, shape["h_loc"])
    print("nystroem_evaluated %.4e lane-entries for %.4e pairs inside the radius (%.3fx)" % (info_v["nystroem_evaluated"], pairs, info_v["nystroem_evaluated"] / pairs))
    assert info_v["nystroem_evaluated"] >= pairs
    assert info_p["filter_fused"] == 1 and info_p["nystroem_path"] == 4 and info_p["nystroem_mfma_flops"] > 0
    for info in (info_v, info_p):
        np.testing.assert_array_equal(info["eigvals"], cinfo["eigvals"])
        assert info["alpha"] == cinfo["alpha"]
    phi, lam = _oracle_phi(img, ns, opt, cinfo)
    f = {glf.FILTER_REFERENCE: lam, glf.FILTER_POC: -(lam + 5.0), glf.FILTER_SMOOTH: 1.0 - lam}[mode]
    gain = float(opt.gain) if mode == glf.FILTER_REFERENCE else 1.0
    ysub = 1.0 if mode == glf.FILTER_SMOOTH else 0.0
    c = np.asarray(cinfo["capture"]["c"], dtype=np.float64)[:lam.size]
    want = (gain * ((f * c) @ phi)).reshape(img.shape)                   # z - (1 - ysub) y
    assert np.abs(want - ysub * img).max() >= 1.0   # the filter moves pixels by whole grey levels: the 8-bit comparison below is not vacuous
    got_v, got_p = zf_v - (1.0 - ysub) * img, zf_p - (1.0 - ysub) * img
    _assert_rule("correction against the fp64 oracle", got_v, want, zf_v)
    _assert_rule("correction against FILTER_FORM=phi", got_v, got_p, zf_v)
    d = np.abs(out_v.astype(np.int32) - out_p.astype(np.int32))
    print("8-bit outputs: %d of %d pixels differ, max %d; %d changed by the filter" % ((d > 0).sum(), d.size, d.max(), (out_v != img).sum()))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-4
    assert (out_v != img).any()
    return info_v


@pytest.mark.parametrize("m", [20, 64])
def test_clipped_windows(m):
    """m = 20: ld = 32, and the 12 padded columns of Psi must not leak into q."""
    info = _guide_case(CLIPPED, m)
    assert info["m"] == m


def test_narrow_kernel():
    """h_loc = 6: a few samples inside the radius of a pixel, most lanes masked in most steps."""
    _guide_case(NARROW, 16)


@pytest.mark.parametrize("nsig", [1, 4])
def test_planes(nsig):
    img, ns = _image(**CLIPPED)
    h, w = img.shape
    sig = _planes(h, w, nsig)
    opt = glf.default_options(num_samples=ns, num_eigvals=20, epsilon=0.1)
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        d_sig = torch.from_numpy(sig).to(ctx.device)
        ctx.set_tuning(**BAND)
        _, _, cinfo = ctx.image_processing(d_img, opt, capture=True)
        res = {}
        for form in ("vec", "phi"):
            ctx.set_tuning(FILTER_FORM=form, **BAND)
            out, zf, so, info = ctx.image_processing_signals(d_img, d_sig, opt, want_float=True)
            res[form] = (out.cpu().numpy(), zf.cpu().numpy().astype(np.float64), so.cpu().numpy().astype(np.float64), info)
        ctx.set_tuning(FILTER_FORM="vec", **BAND)
        out1, zf1, _ = ctx.image_processing(d_img, opt, want_float=True)
    (out_v, zf_v, so_v, info_v), (out_p, zf_p, so_p, info_p) = res["vec"], res["phi"]
    _assert_stats(info_v)
    assert info_p["filter_fused"] == 1 and info_p["nystroem_mfma_flops"] > 0
    np.testing.assert_array_equal(info_v["eigvals"], cinfo["eigvals"])
    # the guide does not see the planes
    np.testing.assert_array_equal(out_v, out1.cpu().numpy())
    np.testing.assert_array_equal(zf_v.astype(np.float32).view(np.int32), zf1.cpu().numpy().view(np.int32))
    phi, lam = _oracle_phi(img, ns, opt, cinfo)
    s = sig.reshape(nsig, -1).astype(np.float64)
    want = (float(opt.gain) * ((lam[:, None] * (phi @ s.T)).T @ phi)).reshape(sig.shape)
    for k in range(nsig):
        _assert_rule("plane %d against the fp64 oracle" % k, so_v[k] - sig[k], want[k], so_v[k])
        _assert_rule("plane %d against FILTER_FORM=phi" % k, so_v[k] - sig[k], so_p[k] - sig[k], so_v[k])
    d = np.abs(out_v.astype(np.int32) - out_p.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-4


def _noskip_pair(form):
    """CLIPPED at m = 20 (a last workgroup whose waves have no row) under FILTER_FORM=form with BAND_NOSKIP unset and set: out and zf
    bit for bit the same, and more entries evaluated without the skips. Returns the two runs' infos."""
    img, ns = _image(**CLIPPED)
    opt = glf.default_options(num_samples=ns, num_eigvals=20, epsilon=0.1)
    res = {}
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        for noskip in (0, 1):
            ctx.set_tuning(FILTER_FORM=form, BAND_NOSKIP="1" if noskip else None, **BAND)
            out, zf, info = ctx.image_processing(d_img, opt, want_float=True)
            res[noskip] = (out.clone(), zf.clone(), info)
    (o0, z0, i0), (o1, z1, i1) = res[0], res[1]
    print("nystroem_evaluated: %.4e with the skips, %.4e without" % (i0["nystroem_evaluated"], i1["nystroem_evaluated"]))
    assert torch.equal(z0.view(torch.int32), z1.view(torch.int32))      # bit for bit
    assert torch.equal(o0, o1)
    np.testing.assert_array_equal(i0["eigvals"], i1["eigvals"])
    assert i0["alpha"] == i1["alpha"]
    assert i1["nystroem_evaluated"] > i0["nystroem_evaluated"]
    return i0, i1


def test_noskip_is_bit_identical():
    """BAND_NOSKIP: every wave walks every sample of its workgroup's range; the per-lane support still applies, so not a bit moves."""
    for info in _noskip_pair("vec"):
        _assert_stats(info)


def test_phi_noskip_is_bit_identical():
    """k_band's epilogue (FILTER_FORM=phi) under BAND_NOSKIP: every wave executes every unit of the workgroup's range. On this shape
    the radius exceeds the image, so no wave with an image row skips anything: what grows the count are the three waves of the last
    workgroup that have no row, which walk with Er15 = 0 and must store nothing (10 665 984 -> 11 010 048 entries)."""
    for info in _noskip_pair("phi"):
        assert info["filter_fused"] == 1 and info["nystroem_path"] == 4 and info["rank_terms"] == 0
        assert info["nystroem_mfma_flops"] > 0 and info["nystroem_evaluated"] > 0


def test_three_ranks_uneven_rows(monkeypatch):
    """93 rows over 3 ranks: 31 each, so every rank's last workgroup is short and the workgroups start at other rows than in one piece."""
    monkeypatch.setenv("GLF_NYS_PATH", "band")
    monkeypatch.setenv("GLF_DEG_PATH", "grid")
    monkeypatch.setenv("GLF_MV_PATH", "band")
    monkeypatch.setenv("GLF_FILTER_FORM", "vec")
    img, ns = _image(**CLIPPED)
    opt = glf.default_options(num_samples=ns, num_eigvals=20, epsilon=0.1)
    with glf.Context(0) as ctx:
        out1, zf1, info1 = ctx.image_processing(ctx.to_device(img), opt, want_float=True)
        out1, zf1 = out1.cpu().numpy(), zf1.cpu().numpy()
    _assert_stats(info1)
    with glf.Multi(3, devices=[0, 0, 0], backend=glf.MULTI_LOOPBACK) as world:
        out, zf, infos = world.image_processing(img, opt, want_float=True)
    assert [(i["row0"], i["row1"]) for i in infos] == [glf.shard_rows(img.shape[0], r, 3) for r in range(3)]
    for i in infos:
        _assert_stats(i)
        assert (i["p"], i["m"], i["outer_its"]) == (info1["p"], info1["m"], info1["outer_its"])
        np.testing.assert_allclose(i["eigvals"], info1["eigvals"], rtol=1e-5)
    np.testing.assert_allclose(zf, zf1, rtol=0, atol=5e-4)              # (tests/test_gpu_multi.py)
    assert np.mean(out != out1) < 1e-3 and psnr(out, out1) >= 60.0
