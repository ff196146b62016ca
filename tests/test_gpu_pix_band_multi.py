"""The band form of the 16-bit and colour kernels (PIX_BAND) under a communicator: loopback worlds of 2 and 3 ranks at 1024^2 with
GLF_PIX_BAND=1 and GLF_MV_PATH=band in the environment against one context with the same keys, at the tolerances and route
assertions of test_gpu_u16_multi.py / test_gpu_rgb_multi.py (the absolute ones in 16-bit units for the 16-bit image). The route is
(4, 4, 0) on every rank and the eigen-solve is replicated, as for the grey band form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_rgb import _rgb_image  # noqa: E402
from test_gpu_u16 import H_VAL, _u16_image  # noqa: E402


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("fmt", ["u16", "rgb"])
def test_loopback_band_matches_single_context(fmt, n, monkeypatch):
    monkeypatch.setenv("GLF_PIX_BAND", "1")
    monkeypatch.setenv("GLF_MV_PATH", "band")
    size = 1024
    u16 = fmt == "u16"
    img = _u16_image(size, size, seed=4) if u16 else _rgb_image(size, size, seed=4)
    scale, vmax = (257.0, 65535.0) if u16 else (1.0, 255.0)
    opt = glf.default_options(num_samples=int(size * size * 0.005), num_eigvals=16, epsilon=0.1, h_val=H_VAL if u16 else 30.0)
    with glf.Context(0) as ctx:
        fn = ctx.image_processing_u16 if u16 else ctx.image_processing_rgb
        out1, zf1, info1 = fn(torch.from_numpy(img).to(ctx.device), opt, want_float=True)
        out1, zf1 = out1.cpu().numpy(), zf1.cpu().numpy()
    with glf.Multi(n, devices=[0] * n, backend=glf.MULTI_LOOPBACK) as world:
        out, zf, infos = (world.image_processing_u16 if u16 else world.image_processing_rgb)(img, opt, want_float=True)
    assert (info1["nystroem_path"], info1["matvec_path"], info1["filter_fused"]) == (4, 4, 0)
    assert info1["contraction"] == glf.CONTRACT_F16_SPLIT
    assert [(i["row0"], i["row1"]) for i in infos] == [glf.shard_rows(size, r, n) for r in range(n)]
    for i in infos:
        assert (i["p"], i["m"], i["outer_its"]) == (info1["p"], info1["m"], info1["outer_its"])
        assert (i["nystroem_path"], i["matvec_path"], i["filter_fused"]) == (4, 4, 0)
        assert i["contraction"] == glf.CONTRACT_F16_SPLIT and i["eigen_sharded"] == 0
        np.testing.assert_allclose(i["eigvals"], info1["eigvals"], rtol=1e-5)
    np.testing.assert_allclose(zf, zf1, rtol=0, atol=5e-4 * scale)
    d = out.astype(np.float64) - out1.astype(np.float64)
    psnr = float("inf") if not d.any() else 10.0 * np.log10(vmax ** 2 / np.mean(d ** 2))
    assert np.mean(out != out1) < 1e-3 and psnr >= 60.0
