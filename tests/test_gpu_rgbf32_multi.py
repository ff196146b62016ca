"""Float colour filtering under a communicator (glf_multi_image_processing_rgbf32 / _rgbf32_signals, loopback ranks on one device, 80
rows over 2 and 3 ranks: a ragged split), with the PIX_BAND key off and on.

The criterion is the colour suite's (tests/test_gpu_rgb_multi.py): the ranks' statistics equal one context's, the eigenvalues within
rtol 1e-5, the float z within 5e-4 grey levels of one context's -- and this image is the colour suite's pattern divided by 4, so
5e-4 / 4 here. (The colour suite's PSNR rule is
on its integer output, which the float call does not have: z is the output.) The guide of the planes call equals the plain call on
the same world bit for bit; a plane matches one context's within 5e-4 max(1, max |s| / 255). A NaN image is refused on the host
before any rank starts and leaves the world usable."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
import test_gpu_rgbf32 as t  # noqa: E402

ATOL = 5e-4 / 4.0


@pytest.mark.parametrize("band", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_loopback_rgbf32_matches_single_context(n, band):
    w, h = 96, 80
    img, sig = t._f32_image(h, w, seed=4), t._test_planes(h, w, 2)[:2]
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=t.H_VAL)
    tune = dict(PIX_BAND="1", NYS_PATH="band", MV_PATH="band") if band else {}
    with glf.Context(0) as ctx:
        ctx.set_tuning(**tune)
        z1, so1, info1 = t._signals(ctx, img, sig, opt)
    with glf.Multi(n, devices=[0] * n, backend=glf.MULTI_LOOPBACK) as world:
        world.set_tuning(**tune)
        z, so, infos = world.image_processing_rgbf32_signals(img, sig, opt)
        pz, pinfos = world.image_processing_rgbf32(img, opt)                 # the plain call on the same world
    assert z.shape == (h, w, 3) and z.dtype == np.float32
    assert t._route(info1) == ((4, 4, 0) if band else (0, 0, 0))
    assert [(i["row0"], i["row1"]) for i in infos] == [glf.shard_rows(h, r, n) for r in range(n)]
    for i, pi in zip(infos, pinfos):
        assert (i["p"], i["m"], i["outer_its"]) == (info1["p"], info1["m"], info1["outer_its"])
        assert t._route(i) == t._route(info1) and t._route(pi) == t._route(info1)
        np.testing.assert_allclose(i["eigvals"], info1["eigvals"], rtol=1e-5)
        np.testing.assert_array_equal(i["eigvals"], pi["eigvals"])
    np.testing.assert_array_equal(t._bits(z), t._bits(pz))
    print("rgbf32 %d ranks band %d: max |multi - single| %.2e <= %.2e" % (n, band, float(np.abs(z - z1).max()), ATOL))
    np.testing.assert_allclose(z, z1, rtol=0, atol=ATOL)
    for k in range(sig.shape[0]):
        tol = 5e-4 * max(1.0, float(np.abs(sig[k]).max()) / 255.0)
        print("rgbf32 %d ranks plane %d: max |multi - single| %.2e <= %.2e" % (n, k, float(np.abs(so[k] - so1[k]).max()), tol))
        np.testing.assert_allclose(so[k], so1[k], rtol=0, atol=tol)


def test_nan_image_is_refused_and_leaves_the_world_usable():
    w, h = 96, 80
    img = t._f32_image(h, w, seed=4)
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=t.H_VAL)
    poisoned = img.copy()
    poisoned[h - 1, w - 1, 2] = np.nan                                       # the last float of the image
    with glf.Multi(2, devices=[0, 0], backend=glf.MULTI_LOOPBACK) as world:
        with pytest.raises(glf.GlfError) as e:
            world.image_processing_rgbf32(poisoned, opt)
        assert e.value.status == glf.ERR_INVALID and "NaN" in str(e.value)
        with pytest.raises(glf.GlfError) as e:
            world.image_processing_rgbf32_signals(poisoned, np.zeros((1, h, w), dtype=np.float32), opt)
        assert e.value.status == glf.ERR_INVALID
        zm, _ = world.image_processing_rgbf32(img, opt)                       # the world is still usable
    assert np.isfinite(zm).all() and np.any(zm != img)
