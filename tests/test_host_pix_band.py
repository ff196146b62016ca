"""-pix_band in the host program: with -depth16 or -color -rgb_graph it sets the PIX_BAND tuning key, and one more line names the
routes the call took. The test images are narrower than 1024 pixels, where the band form is not the automatic choice, so the child
process gets GLF_NYS_PATH=band and GLF_MV_PATH=band; the output must equal the Python call's made with the same three keys, byte for
byte (as the plain flags' tests do). Without one of the two modes the flag is a usage error."""
import os
import subprocess

import numpy as np
import pytest
import torch

import glf
from test_gpu_u16 import _u16_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "image-processing-graph-laplacian_amd", "image_processing")
SRC_RGB = os.path.join(ROOT, "tests", "golden", "pixel_mountains.png")
NS, M = 300, 16
KEYS = dict(PIX_BAND="1", NYS_PATH="band", MV_PATH="band")

pytestmark = pytest.mark.gpu


def _run(args, cwd, env_keys=None):
    os.makedirs(os.path.join(cwd, "results"), exist_ok=True)
    env = dict(os.environ)
    for k, v in (env_keys or {}).items():
        env["GLF_" + k] = v
    return subprocess.run([EXE] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize("flt", ["reference", "smooth"])
def test_depth16_pix_band_matches_python_call(tmp_path, flt):
    img = _u16_image(72, 96, seed=12)
    src = str(tmp_path / "in16.png")
    glf.write_png16(src, img)
    opt = glf.default_options(num_samples=NS, num_eigvals=M, h_val=30.0 * 257.0,
                              filter_mode={"reference": glf.FILTER_REFERENCE, "smooth": glf.FILTER_SMOOTH}[flt])
    with glf.Context(0) as ctx:
        ctx.set_tuning(**KEYS)
        want, _, info = ctx.image_processing_u16(torch.from_numpy(img).to(ctx.device), opt)
        want = want.cpu().numpy()
    assert (info["nystroem_path"], info["matvec_path"]) == (4, 4)
    r = _run(["-f", src, "-depth16", "-pix_band", "-num_samples", str(NS), "-num_eigvals", str(M), "-filter", flt], str(tmp_path),
             dict(NYS_PATH="band", MV_PATH="band"))
    assert r.returncode == 0, r.stderr.decode()
    assert "band form: nystroem_path 4, matvec_path 4" in r.stdout.decode().splitlines()
    got = glf.read_png16(os.path.join(str(tmp_path), "results", "output.png"))
    np.testing.assert_array_equal(got, want)
    assert np.any(got != img)


@pytest.mark.parametrize("flt", ["reference", "smooth"])
def test_color_rgb_graph_pix_band_matches_python_call(tmp_path, flt):
    rgb = glf.read_png_rgb(SRC_RGB)
    opt = glf.default_options(num_samples=NS, num_eigvals=M, filter_mode={"reference": glf.FILTER_REFERENCE, "smooth": glf.FILTER_SMOOTH}[flt])
    with glf.Context(0) as ctx:
        ctx.set_tuning(**KEYS)
        want, _, info = ctx.image_processing_rgb(torch.from_numpy(rgb).to(ctx.device), opt)
        want = want.cpu().numpy()
    assert (info["nystroem_path"], info["matvec_path"]) == (4, 4)
    r = _run(["-f", SRC_RGB, "-color", "-rgb_graph", "-pix_band", "-num_samples", str(NS), "-num_eigvals", str(M), "-filter", flt],
             str(tmp_path), dict(NYS_PATH="band", MV_PATH="band"))
    assert r.returncode == 0, r.stderr.decode()
    assert "band form: nystroem_path 4, matvec_path 4" in r.stdout.decode().splitlines()
    got = glf.read_png_rgb(os.path.join(str(tmp_path), "results", "output.png"))
    np.testing.assert_array_equal(got, want)
    assert np.any(got != rgb)


def test_the_environment_variable_works_without_the_flag(tmp_path):
    """GLF_PIX_BAND=1 alone selects the route (same PNG as with the flag); the route line belongs to the flag."""
    img = _u16_image(72, 96, seed=12)
    src = str(tmp_path / "in16.png")
    glf.write_png16(src, img)
    args = ["-f", src, "-depth16", "-num_samples", str(NS), "-num_eigvals", str(M)]
    r1 = _run(args + ["-pix_band"], str(tmp_path), dict(NYS_PATH="band", MV_PATH="band"))
    assert r1.returncode == 0, r1.stderr.decode()
    one = glf.read_png16(os.path.join(str(tmp_path), "results", "output.png"))
    r2 = _run(args, str(tmp_path), KEYS)
    assert r2.returncode == 0, r2.stderr.decode()
    two = glf.read_png16(os.path.join(str(tmp_path), "results", "output.png"))
    np.testing.assert_array_equal(one, two)
    assert "band form:" in r1.stdout.decode() and "band form:" not in r2.stdout.decode()
    r3 = _run(args, str(tmp_path))                                # neither: the entry-by-entry route, no route line
    assert r3.returncode == 0 and "band form:" not in r3.stdout.decode()


def test_pix_band_falls_back_and_says_so(tmp_path):
    """-pix_band on an image narrower than 1024 pixels with automatic paths: the fallback's numbers on the route line."""
    img = _u16_image(72, 96, seed=12)
    src = str(tmp_path / "in16.png")
    glf.write_png16(src, img)
    r = _run(["-f", src, "-depth16", "-pix_band", "-num_samples", str(NS), "-num_eigvals", str(M)], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()
    assert "band form: nystroem_path 0, matvec_path 0" in r.stdout.decode().splitlines()


@pytest.mark.parametrize("extra", [[], ["-color"], ["-color", "-chroma"], ["-fused"]])
def test_pix_band_alone_is_a_usage_error(tmp_path, extra):
    r = _run(["-f", SRC_RGB, "-pix_band"] + extra, str(tmp_path))
    assert r.returncode == 1 and b"-pix_band" in r.stderr and b"needs -depth16 or -color -rgb_graph" in r.stderr, r.stderr
    assert len(r.stderr.decode().strip().splitlines()) == 1
