"""The column pass of the separable rank-R filter on the matrix pipe (k_band_sep_cols_mfma, FILTER_FORM=sep: a banded GEMM with
M = expansion term, N = pixel, K = sample column in k-steps of 16, split-f16 operands, S scaled by one power of two per plane) where
only this form can go wrong; tests/test_gpu_band_sep.py runs on the same kernel and covers the clipped windows, m, R = 16 / 32 / 48,
the planes, BAND_NOSKIP, determinism and the ranks.

Here: windows of sample columns that move with the tile over three and over five k-steps (the second more than the four whose
Ec fragments sit in LDS at a time), a grid with fewer than 16 sample columns in all, and the operand scale: planes 2^12, 2^-12 and
2^+-30 times a plane and an all-zero plane in one run with the guide.

Every correction is held to the project's rule ||got - want|| <= 1e-5 ||want|| + 2^-24 ||z|| (_assert_rule) twice: against the
fp64 oracle fed the run's own eigenpairs and against FILTER_FORM=vec. The 8-bit outputs of the two forms differ by at most 1 on at
most 1e-4 of the pixels, and the oracle's correction must reach a whole grey level. Those two caps are conditions on the inputs:
shapes, seeds and the default gain are chosen so that the previous column pass (scalar loads, vector FMAs) stays inside them against
vec on the same inputs -- this file passes unchanged with that library."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402

from test_gpu_band_sep import _assert_stats, _guide_case, _oracle_phi  # noqa: E402
from test_gpu_band_vec import BAND, CLIPPED, _assert_rule, _image, _planes  # noqa: E402

# 365 samples on a 5 x 73 grid of pitch 14, radius 212: with tiles of 128 pixels the ranges of sample columns are
# (first column, count, k-steps) = (0, 24, 2) (0, 33, 3) (3, 39, 3) (12, 40, 3) (21, 40, 3) (31, 39, 3) (40, 33, 3) (49, 24, 2)
WIDE = dict(width=1024, height=75, frac=0.005, h_loc=40.0, seed=11)
# 1606 samples on an 11 x 146 grid of pitch 7: (0, 48, 3) (0, 67, 5) (6, 79, 5) (25, 78, 5) (43, 79, 5) (61, 79, 5) (80, 66, 5) (98, 48, 3)
WIDE_DENSE = dict(width=1024, height=75, frac=0.02, h_loc=40.0, seed=11)
# 112 samples on an 8 x 14 grid, radius 32: (0, 11, 1) (7, 7, 1) -- one part-filled k-step, nc = 14 < 16
FEW_COLUMNS = dict(width=200, height=120, frac=0.005, h_loc=6.0, seed=9)


def test_moving_windows_three_ksteps():
    """nc = 73; 2, 3, 3, 3, 3, 3, 3, 2 k-steps per tile of 128 pixels, the range starting at columns 0, 0, 3, 12, 21, 31, 40, 49:
    past column 0 for the middle tiles, clipped at both image edges, counts that are no multiple of 16. 75 rows: a last workgroup
    of 3."""
    _guide_case(WIDE, 16)


def test_moving_windows_five_ksteps():
    """nc = 146; 3, 5, 5, 5, 5, 5, 5, 3 k-steps per tile: more than the four k-steps of Ec fragments that LDS holds, so the fragments
    are formed again per term tile between barriers."""
    _guide_case(WIDE_DENSE, 16)


def test_fewer_than_16_sample_columns():
    """nc = 14: every tile is one part-filled k-step whose dead entries clamp to the last sample column."""
    _guide_case(FEW_COLUMNS, 16)


def _signals_case(shape, m, sig):
    """the guide and the planes `sig` [n, H, W] through sep and vec; returns the planes' outputs (float64) of both and the oracle's
    corrections, after holding every plane to the rule against the oracle and against vec"""
    img, ns = _image(**shape)
    nsig = sig.shape[0]
    opt = glf.default_options(num_samples=ns, num_eigvals=m, epsilon=0.1, h_loc=shape["h_loc"])
    with glf.Context(0) as ctx:
        d_img = ctx.to_device(img)
        d_sig = torch.from_numpy(sig).to(ctx.device)
        ctx.set_tuning(**BAND)
        _, _, cinfo = ctx.image_processing(d_img, opt, capture=True)
        res = {}
        for form in ("sep", "vec"):
            ctx.set_tuning(FILTER_FORM=form, **BAND)
            out, zf, so, info = ctx.image_processing_signals(d_img, d_sig, opt, want_float=True)
            res[form] = (out.cpu().numpy(), zf.cpu().numpy().astype(np.float64), so.cpu().numpy(), info)
    (out_s, zf_s, so_s, info_s), (out_v, zf_v, so_v, info_v) = res["sep"], res["vec"]
    _assert_stats(info_s)
    _assert_stats(info_v, False)
    np.testing.assert_array_equal(info_s["eigvals"], cinfo["eigvals"])
    phi, lam = _oracle_phi(img, ns, opt, cinfo)
    s = sig.reshape(nsig, -1).astype(np.float64)
    want = (float(opt.gain) * ((lam[:, None] * (phi @ s.T)).T @ phi)).reshape(sig.shape)
    for k in range(nsig):
        got = so_s[k].astype(np.float64) - sig[k]
        _assert_rule("plane %d against the fp64 oracle" % k, got, want[k], so_s[k])
        _assert_rule("plane %d against FILTER_FORM=vec" % k, got, so_v[k].astype(np.float64) - sig[k], so_s[k])
    _assert_rule("guide against FILTER_FORM=vec", zf_s - img, zf_v - img, zf_s)
    d = np.abs(out_s.astype(np.int32) - out_v.astype(np.int32))
    print("8-bit outputs: %d of %d pixels differ, max %d" % ((d > 0).sum(), d.size, d.max()))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-4
    assert (out_s != img).any()
    return so_s, so_v, want


def test_operand_scale():
    """One plane as it is, times 2^12, times 2^-12, and all zeros, beside the guide: four exponents in one run.
    The zero plane has no q: its scale must be finite and the plane must come back bit-equal to its input.
    A power of two commutes with every rounding of the path (no overflow, no subnormal at these sizes), so the scaled planes' outputs
    are exactly 2^+-12 times the unscaled plane's: the previous column pass (no operand scale: f32 throughout) has that property on
    these inputs, and a per-plane power-of-two scale of S must keep it."""
    h, w = CLIPPED["height"], CLIPPED["width"]
    base = _planes(h, w, 1)[0]
    sig = np.stack([base, base * np.float32(4096.0), base * np.float32(1.0 / 4096.0), np.zeros_like(base)])
    so_s, so_v, want = _signals_case(CLIPPED, 20, sig)
    assert np.abs(want[0]).max() > 0.0
    assert np.isfinite(so_s).all()
    np.testing.assert_array_equal(so_s[3].view(np.int32), sig[3].view(np.int32))
    exact = [bool(np.array_equal(so_s[1], so_s[0] * np.float32(4096.0))), bool(np.array_equal(so_s[2], so_s[0] * np.float32(1.0 / 4096.0)))]
    print("planes x 2^12 and x 2^-12 come back as exact multiples:", exact)
    assert all(exact)


def test_two_sizes_of_q_in_one_run():
    """Planes 2^-30 and 2^30 times a plane beside the guide, on the wide image: |q| of the three differs by nine orders of magnitude
    each way. One exponent shared by the planes would leave the small plane's S below the f16 halves' range (its values at 2^-60
    of the largest, the halves reach 2^-38) and miss the rule by orders of magnitude; per plane it is held as any other."""
    h, w = WIDE["height"], WIDE["width"]
    base = _planes(h, w, 1, seed=5)[0]
    sig = np.stack([base * np.float32(2.0 ** -30), base * np.float32(2.0 ** 30)])
    _signals_case(WIDE, 16, sig)
