"""16-bit greyscale filtering under a communicator (glf_multi_image_processing_u16, loopback ranks on one device): the outputs must
match one context within test_gpu_rgb_multi.py's tolerances, the absolute ones scaled by 257 to 16-bit units. The image is
replicated on every rank, each rank sums the degree and filters its own pixel rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glf  # noqa: E402
from test_gpu_u16 import H_VAL, _u16_image  # noqa: E402


def _check(img, opt, n):
    with glf.Context(0) as ctx:
        out1, zf1, info1 = ctx.image_processing_u16(torch.from_numpy(img).to(ctx.device), opt, want_float=True)
        out1, zf1 = out1.cpu().numpy(), zf1.cpu().numpy()
    with glf.Multi(n, devices=[0] * n, backend=glf.MULTI_LOOPBACK) as world:
        out, zf, infos = world.image_processing_u16(img, opt, want_float=True)
    h = img.shape[0]
    assert [(i["row0"], i["row1"]) for i in infos] == [glf.shard_rows(h, r, n) for r in range(n)]
    for i in infos:
        assert (i["p"], i["m"], i["outer_its"]) == (info1["p"], info1["m"], info1["outer_its"])
        assert (i["nystroem_path"], i["matvec_path"], i["filter_fused"]) == (info1["nystroem_path"], info1["matvec_path"], info1["filter_fused"])
        np.testing.assert_allclose(i["eigvals"], info1["eigvals"], rtol=1e-5)
    np.testing.assert_allclose(zf, zf1, rtol=0, atol=5e-4 * 257)
    d = out.astype(np.float64) - out1.astype(np.float64)
    psnr = float("inf") if not d.any() else 10.0 * np.log10(65535.0 ** 2 / np.mean(d ** 2))
    assert np.mean(out != out1) < 1e-3 and psnr >= 60.0


@pytest.mark.parametrize("n", [2, 3])
def test_loopback_u16_matches_single_context(n):
    opt = glf.default_options(num_samples=60, num_eigvals=8, epsilon=0.05, h_val=H_VAL)
    _check(_u16_image(80, 96, seed=4), opt, n)


def test_two_ranks_at_2048_default_paths():
    size = 2048
    opt = glf.default_options(num_samples=int(size * size * 0.0025), num_eigvals=32, epsilon=0.1, h_val=H_VAL)
    _check(_u16_image(size, size, seed=9), opt, 2)
