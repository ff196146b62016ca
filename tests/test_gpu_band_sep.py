"""The fused filter of the band form in separable rank-R form (k_band_sep_g / _rows / _cols, FILTER_FORM=sep: the photometric table as
its expansion P = F F^T, the sum factored into a row pass over the band rows and a column pass over the sample columns) on the shapes
of tests/test_gpu_band_vec.py: a radius larger than the image (every window clipped, a last tile of 8 pixels, a last workgroup with
waves without a row), m below the padded width of Psi, a narrow kernel, signal planes, three photometric scales (R = 16, 32, 48, and
one too sharp for an expansion, where k_band_vec must run), the BAND_NOSKIP schedule, three ranks, determinism.

The correction z - (1 - ysub) y (and each plane's) is held to the project's rule ||got - want|| <= 1e-5 ||want|| + 2^-24 ||z|| twice:
against the fp64 oracle's Nystroem extension fed the run's own Phi_A, eigenvalues, alpha and c, and against the FILTER_FORM=vec run
(the same sum pair by pair with the exact table). The 8-bit outputs of the two forms differ by at most 1 on at most 1e-4 of the pixels;
the oracle's correction must reach a whole grey level for that to say anything, which is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import oracle as orc  # noqa: E402

from conftest import psnr  # noqa: E402
from test_gpu_band_vec import BAND, CLIPPED, NARROW, _assert_rule, _image, _planes  # noqa: E402


def _assert_stats(info, sep=True):
    assert info["filter_fused"] == 1 and info["nystroem_path"] == 4
    assert info["nystroem_mfma_flops"] == 0 and info["nystroem_evaluated"] > 0
    assert (info["rank_terms"] > 0) == sep, info["rank_terms"]


def _oracle_phi(img, ns, opt, cinfo):
    """fp64 Phi [m, N] in raster order from the captured run's eigenpairs, at the run's h_loc and h_val"""
    h, w = img.shape
    idx = glf.Sampling(w, h, ns)
    lam = np.asarray(cinfo["eigvals"], dtype=np.float64)
    prm = orc.default_params()
    prm.h_loc = float(opt.h_loc)
    prm.h_val = float(opt.h_val)
    phi_A = cinfo["capture"]["phi_A"].cpu().numpy()[:, :lam.size].astype(np.float64).T
    return orc.permutation(orc.nystroem(img, idx, cinfo["alpha"], phi_A, lam, prm=prm), idx), lam


def _guide_case(shape, m, sep=True, **optkw):
    img, ns = _image(**shape)
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1, h_loc=shape["h_loc"], **optkw)
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        ctx.set_tuning(**BAND)
        _, _, cinfo = ctx.image_processing(d_img, opt, capture=True)
        res = {}
        for form in ("sep", "vec"):
            ctx.set_tuning(FILTER_FORM=form, **BAND)
            out, zf, info = ctx.image_processing(d_img, opt, want_float=True)
            res[form] = (out.cpu().numpy(), zf.cpu().numpy().astype(np.float64), info)
    (out_s, zf_s, info_s), (out_v, zf_v, info_v) = res["sep"], res["vec"]
    print("rank_terms %d, nystroem_evaluated %.4e (vec %.4e)" % (info_s["rank_terms"], info_s["nystroem_evaluated"], info_v["nystroem_evaluated"]))
    _assert_stats(info_s, sep)
    _assert_stats(info_v, False)
    for info in (info_s, info_v):
        np.testing.assert_array_equal(info["eigvals"], cinfo["eigvals"])
        assert info["alpha"] == cinfo["alpha"]
    phi, lam = _oracle_phi(img, ns, opt, cinfo)
    c = np.asarray(cinfo["capture"]["c"], dtype=np.float64)[:lam.size]
    want = (float(opt.gain) * ((lam * c) @ phi)).reshape(img.shape)      # z - y (the reference filter)
    assert np.abs(want).max() >= 1.0   # the filter moves pixels by whole grey levels: the 8-bit comparison below is not vacuous
    got_s, got_v = zf_s - img, zf_v - img
    _assert_rule("correction against the fp64 oracle", got_s, want, zf_s)
    _assert_rule("correction against FILTER_FORM=vec", got_s, got_v, zf_s)
    d = np.abs(out_s.astype(np.int32) - out_v.astype(np.int32))
    print("8-bit outputs: %d of %d pixels differ, max %d; %d changed by the filter" % ((d > 0).sum(), d.size, d.max(), (out_s != img).sum()))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-4
    assert (out_s != img).any()
    return info_s


@pytest.mark.parametrize("m", [20, 64])
def test_clipped_windows(m):
    """m = 20: ld = 32, and the 12 padded columns of Psi must not leak into q."""
    info = _guide_case(CLIPPED, m)
    assert info["m"] == m


def test_narrow_kernel():
    """h_loc = 6: three or four sample columns within the radius of a tile, one to five band rows per image row."""
    _guide_case(NARROW, 16)


@pytest.mark.parametrize("h_val", [60.0, 20.0])
def test_photometric_scales(h_val):
    """h_val = 60: R = 16, the column pass' blocks of 16 terms; h_val = 20: R = 48, three of them and an F table beyond 48 KiB of LDS."""
    _guide_case(CLIPPED, 20, h_val=h_val)


def test_sharp_kernel_takes_vec():
    """h_val = 10: no expansion of at most 64 terms (R = 0); FILTER_FORM=sep then runs k_band_vec, and rank_terms = 0 says so."""
    _guide_case(CLIPPED, 20, sep=False, h_val=10.0)


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
        for form in ("sep", "vec"):
            ctx.set_tuning(FILTER_FORM=form, **BAND)
            out, zf, so, info = ctx.image_processing_signals(d_img, d_sig, opt, want_float=True)
            res[form] = (out.cpu().numpy(), zf.cpu().numpy().astype(np.float64), so.cpu().numpy().astype(np.float64), info)
        ctx.set_tuning(FILTER_FORM="sep", **BAND)
        out1, zf1, _ = ctx.image_processing(d_img, opt, want_float=True)
    (out_s, zf_s, so_s, info_s), (out_v, zf_v, so_v, info_v) = res["sep"], res["vec"]
    _assert_stats(info_s)
    _assert_stats(info_v, False)
    np.testing.assert_array_equal(info_s["eigvals"], cinfo["eigvals"])
    # the guide does not see the planes
    np.testing.assert_array_equal(out_s, out1.cpu().numpy())
    np.testing.assert_array_equal(zf_s.astype(np.float32).view(np.int32), zf1.cpu().numpy().view(np.int32))
    phi, lam = _oracle_phi(img, ns, opt, cinfo)
    s = sig.reshape(nsig, -1).astype(np.float64)
    want = (float(opt.gain) * ((lam[:, None] * (phi @ s.T)).T @ phi)).reshape(sig.shape)
    for k in range(nsig):
        _assert_rule("plane %d against the fp64 oracle" % k, so_s[k] - sig[k], want[k], so_s[k])
        _assert_rule("plane %d against FILTER_FORM=vec" % k, so_s[k] - sig[k], so_v[k] - sig[k], so_s[k])
    _assert_rule("guide against FILTER_FORM=vec", zf_s - img, zf_v - img, zf_s)
    d = np.abs(out_s.astype(np.int32) - out_v.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-4


def _two_runs(tunings):
    img, ns = _image(**CLIPPED)
    opt = glf.default_options(num_samples=ns, num_eigvals=20, epsilon=0.1)
    res = []
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        for t in tunings:
            ctx.set_tuning(FILTER_FORM="sep", **t, **BAND)
            out, zf, info = ctx.image_processing(d_img, opt, want_float=True)
            res.append((out.clone(), zf.clone(), info))
    (o0, z0, i0), (o1, z1, i1) = res
    _assert_stats(i0)
    _assert_stats(i1)
    assert torch.equal(z0.view(torch.int32), z1.view(torch.int32))      # bit for bit
    assert torch.equal(o0, o1)
    np.testing.assert_array_equal(i0["eigvals"], i1["eigvals"])
    assert i0["alpha"] == i1["alpha"]
    return i0, i1


def test_noskip_is_bit_identical():
    """BAND_NOSKIP: the row pass takes every band row, and the waves without an image row walk the columns too: the order stays
    and every added term is an exact zero."""
    i0, i1 = _two_runs([dict(BAND_NOSKIP=None), dict(BAND_NOSKIP="1")])
    print("nystroem_evaluated: %.4e with the skips, %.4e without" % (i0["nystroem_evaluated"], i1["nystroem_evaluated"]))
    assert i1["nystroem_evaluated"] > i0["nystroem_evaluated"]


def test_deterministic():
    i0, i1 = _two_runs([dict(), dict()])
    assert i0["nystroem_evaluated"] == i1["nystroem_evaluated"]


def test_three_ranks_uneven_rows(monkeypatch):
    """93 rows over 3 ranks: 31 each, so every rank's row pass and column pass start at other rows than in one piece and end short."""
    monkeypatch.setenv("GLF_NYS_PATH", "band")
    monkeypatch.setenv("GLF_DEG_PATH", "grid")
    monkeypatch.setenv("GLF_MV_PATH", "band")
    monkeypatch.setenv("GLF_FILTER_FORM", "sep")
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
