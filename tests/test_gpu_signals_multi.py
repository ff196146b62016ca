"""Joint filtering under a communicator (glf_multi_image_processing_signals, loopback ranks on one device): the guide and the
signal planes must match one context. The planes are replicated on every rank, each rank filters its own pixel rows, and
Phi^T s is all-reduced in a collective of its own."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from conftest import psnr  # noqa: E402
from test_gpu_multi import _env_paths  # noqa: E402


def _planes(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(0.0, 40.0, (h, w)), np.linspace(-3.0, 7.0, h * w).reshape(h, w) ** 2]).astype(np.float32)


def _check(img, sig, opt, n):
    with glf.Context(0) as ctx:
        d_sig = torch.from_numpy(sig).to(ctx.device)
        out1, zf1, so1, info1 = ctx.image_processing_signals(ctx.to_device(img), d_sig, opt, want_float=True)
        out1, zf1, so1 = out1.cpu().numpy(), zf1.cpu().numpy(), so1.cpu().numpy()
    with glf.Multi(n, devices=[0] * n, backend=glf.MULTI_LOOPBACK) as world:
        out, zf, so, infos = world.image_processing_signals(img, sig, opt)
        pout, pzf, _ = world.image_processing(img, opt, want_float=True)     # the plain call on the same world
    h = img.shape[0]
    assert [(i["row0"], i["row1"]) for i in infos] == [glf.shard_rows(h, r, n) for r in range(n)]
    for i in infos:
        assert (i["p"], i["m"], i["outer_its"]) == (info1["p"], info1["m"], info1["outer_its"])
        np.testing.assert_allclose(i["eigvals"], info1["eigvals"], rtol=1e-5)
    # the guide: the plain multi call's outputs bit for bit, one context's within test_gpu_multi's tolerances
    np.testing.assert_array_equal(out, pout)
    np.testing.assert_array_equal(zf.view(np.int32), pzf.view(np.int32))
    np.testing.assert_allclose(zf, zf1, rtol=0, atol=5e-4)
    assert np.mean(out != out1) < 1e-3 and psnr(out, out1) >= 60.0
    for k in range(sig.shape[0]):
        scale = max(1.0, float(np.abs(sig[k]).max()) / 255.0)
        np.testing.assert_allclose(so[k], so1[k], rtol=0, atol=5e-4 * scale)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("paths", ["direct", "band"])
def test_loopback_signals_match_single_context(n, paths, monkeypatch):
    _env_paths(monkeypatch, paths)
    img = glf.synth_image(96, 80, seed=4)
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05)
    _check(img, _planes(80, 96, 2), opt, n)


def test_two_ranks_at_2048_default_paths_debug_pool(monkeypatch):
    """Rank 1's shard starts far below the degree table's reach of the top grid rows: the windowed degree sums must not read
    the m-tiles the contraction never wrote for them (the debug pool fills fresh buffers with NaN, so such a read shows)."""
    monkeypatch.setenv("GLF_POOL_DEBUG", "1")
    size = 2048
    img = glf.synth_image(size, size, seed=0)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=64, epsilon=0.1)
    _check(img, _planes(size, size, 9), opt, 2)


def test_multi_invalid_arguments_with_a_live_world():
    """nsig outside 1..4 or a null plane pointer on a live world: GLF_ERR_INVALID from those checks themselves."""
    img = glf.synth_image(64, 48, seed=1)
    sig = np.zeros((1, 48, 64), dtype=np.float32)
    out = np.zeros((48, 64), dtype=np.uint8)
    opt = glf.default_options(num_samples=60, num_eigvals=8)
    C = glf.C
    with glf.Multi(2, devices=[0, 0], backend=glf.MULTI_LOOPBACK) as world:
        for nsig, ps, po in ((0, sig, sig), (5, sig, sig), (1, None, sig), (1, sig, None)):
            rc = glf._lib.glf_multi_image_processing_signals(
                world._w, C.byref(opt), img.ctypes.data_as(C.c_void_p), 64, 48, nsig,
                ps.ctypes.data_as(C.c_void_p) if ps is not None else None, po.ctypes.data_as(C.c_void_p) if po is not None else None,
                out.ctypes.data_as(C.c_void_p), None, None, None)
            assert rc == glf.ERR_INVALID, (nsig, ps is None, po is None)
        _, _, so, _ = world.image_processing_signals(img, sig, opt)      # the world still works
        assert np.isfinite(so).all()
