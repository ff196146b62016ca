"""The band form's skips against the same kernel without them. k_band's pixel-target kernel passes over every (pair of band
rows, half-block of 8 sample columns) outside a wave's window; the entries there are exact zeros in the arithmetic in use, so
executing them -- BAND_NOSKIP=1: every wave takes every unit of its workgroup's range, in the same order -- must not change a
bit of the result, only the executed work. A schedule that dropped a unit holding non-zero entries would differ here even
where the entries are far below what the parity tests can see. (The host-side counterpart: tests/test_band_plan.py.)"""
import numpy as np
import pytest

import glf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = glf.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused-filter", "phi-written"])
def test_band_skips_are_bit_identical(ctx, fused):
    import torch
    img = glf.synth_image(1024, 1024, seed=5)
    d_img = ctx.to_device(img)
    opt = glf.default_options(num_samples=int(1024 * 1024 * 0.005), num_eigvals=64, epsilon=0.1)
    res = {}
    try:
        for noskip in (0, 1):
            ctx.set_tuning(NYS_PATH="band", MV_PATH="band", DEG_PATH="grid", NO_FUSED_FILTER=None if fused else "1",
                           BAND_NOSKIP="1" if noskip else None)
            out, zf, info = ctx.image_processing(d_img, opt, want_float=True)
            res[noskip] = (out.clone(), zf.clone(), info)
    finally:
        ctx.reset_tuning()
    (o0, z0, i0), (o1, z1, i1) = res[0], res[1]
    assert i0["nystroem_path"] == 4 and i1["nystroem_path"] == 4
    assert i0["filter_fused"] == i1["filter_fused"] == (1 if fused else 0)
    assert i0["p"] == 5329 and i0["m"] == 64
    print("nystroem_evaluated: %.4e with the skips, %.4e without" % (i0["nystroem_evaluated"], i1["nystroem_evaluated"]))
    assert torch.equal(z0.view(torch.int32), z1.view(torch.int32))      # bit for bit
    assert torch.equal(o0, o1)
    np.testing.assert_array_equal(i0["eigvals"], i1["eigvals"])
    assert i0["alpha"] == i1["alpha"]
    assert i1["nystroem_evaluated"] > i0["nystroem_evaluated"]
