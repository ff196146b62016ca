"""Joint filtering under a colour or a 16-bit guide with a communicator (glf_multi_image_processing_rgb_signals / _u16_signals,
loopback ranks on one device, 80 rows over 2 and 3 ranks: a ragged split). The guide equals the plain multi call on the same world
bit for bit (its c = Phi^T x is all-reduced in a collective of its own, shaped as in the plain call) and one context within
test_gpu_rgb_multi.py's / test_gpu_u16_multi.py's tolerances; the planes match one context by test_gpu_signals_multi.py's rule."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_pix_band import FMTS, _bits  # noqa: E402
from test_gpu_pix_signals import _run, _test_planes  # noqa: E402


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("n", [2, 3])
def test_loopback_pix_signals_match_plain_world_and_single_context(fmt, n):
    f = FMTS[fmt]
    w, h = 96, 80
    img, sig = f.image(h, w, seed=4), _test_planes(h, w, 2)
    opt = f.options(num_samples=60, num_eigvals=8, epsilon=0.05)
    with glf.Context(0) as ctx:
        out1, zf1, so1, info1 = _run(f, ctx, img, sig, opt)
    with glf.Multi(n, devices=[0] * n, backend=glf.MULTI_LOOPBACK) as world:
        fn, plain = ((world.image_processing_u16_signals, world.image_processing_u16) if f.u16 else
                     (world.image_processing_rgb_signals, world.image_processing_rgb))
        out, zf, so, infos = fn(img, sig, opt, want_float=True)
        pout, pzf, pinfos = plain(img, opt, want_float=True)                 # the plain call on the same world
    assert [(i["row0"], i["row1"]) for i in infos] == [glf.shard_rows(h, r, n) for r in range(n)]
    for i, pi in zip(infos, pinfos):
        assert (i["p"], i["m"], i["outer_its"]) == (info1["p"], info1["m"], info1["outer_its"])
        assert (i["nystroem_path"], i["matvec_path"], i["filter_fused"]) == (info1["nystroem_path"], info1["matvec_path"], info1["filter_fused"])
        np.testing.assert_allclose(i["eigvals"], info1["eigvals"], rtol=1e-5)
        np.testing.assert_array_equal(i["eigvals"], pi["eigvals"])
    # the guide: the plain multi call's outputs bit for bit, one context's within the format's multi tolerances
    np.testing.assert_array_equal(out, pout)
    np.testing.assert_array_equal(_bits(zf), _bits(pzf))
    scale = 257.0 if f.u16 else 1.0
    np.testing.assert_allclose(zf, zf1, rtol=0, atol=5e-4 * scale)
    d = out.astype(np.float64) - out1.astype(np.float64)
    psnr = float("inf") if not d.any() else 10.0 * np.log10(float(f.vmax) ** 2 / np.mean(d ** 2))
    assert np.mean(out != out1) < 1e-3 and psnr >= 60.0
    for k in range(sig.shape[0]):
        tol = 5e-4 * max(1.0, float(np.abs(sig[k]).max()) / 255.0)
        print("%s %d ranks plane %d: max |multi - single| %.2e <= %.2e" % (fmt, n, k, float(np.abs(so[k] - so1[k]).max()), tol))
        np.testing.assert_allclose(so[k], so1[k], rtol=0, atol=tol)
