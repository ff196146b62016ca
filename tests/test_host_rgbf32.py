"""-float_rgb in the host program: a colour Portable Float Map ("PF") is filtered on its three float channels
(glf_image_processing_rgbf32) and the result is written as a colour PFM. The output must equal the Python binding's z bit for bit;
-pix_band prints the route line, -planes writes the plane outputs, and the conflicting flags are refused with one message and a
non-zero exit."""
import os
import subprocess

import numpy as np
import pytest
import torch

import glf
import test_gpu_rgbf32 as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "image-processing-graph-laplacian_amd", "image_processing")
NS, M = 300, 16

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    os.makedirs(os.path.join(cwd, "results"), exist_ok=True)
    return subprocess.run([EXE] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _src(tmp_path):
    img = t._f32_image(72, 96, seed=12)
    p = str(tmp_path / "in.pfm")
    glf.write_pfm_rgb(p, img)
    return p, img


ARGS = ["-float_rgb", "-num_samples", str(NS), "-num_eigvals", str(M), "-h_val", repr(t.H_VAL)]


@pytest.mark.parametrize("flt", ["reference", "smooth"])
def test_float_rgb_matches_python_call(tmp_path, flt):
    src, img = _src(tmp_path)
    opt = glf.default_options(num_samples=NS, num_eigvals=M, h_val=t.H_VAL,
                              filter_mode={"reference": glf.FILTER_REFERENCE, "smooth": glf.FILTER_SMOOTH}[flt])
    with glf.Context(0) as ctx:
        want, _ = ctx.image_processing_rgbf32(torch.from_numpy(img).to(ctx.device), opt)
        want = want.cpu().numpy()
    r = _run(["-f", src] + ARGS + ["-filter", flt], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()
    out = r.stdout.decode()
    assert "float colour" in out and "Total computation time" in out
    path = os.path.join(str(tmp_path), "results", "output.pfm")
    assert open(path, "rb").read(2) == b"PF" and open(os.path.join(str(tmp_path), "results", "input.pfm"), "rb").read(2) == b"PF"
    got = glf.read_pfm_rgb(path)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    assert np.any(got != img)
    np.testing.assert_array_equal(glf.read_pfm_rgb(os.path.join(str(tmp_path), "results", "input.pfm")).view(np.int32), img.view(np.int32))


def test_float_rgb_pix_band_planes_and_two_ranks(tmp_path):
    src, img = _src(tmp_path)
    plane = str(tmp_path / "plane.png")
    glf.write_png(plane, glf.synth_image(96, 72, seed=3))
    r = _run(["-f", src] + ARGS + ["-pix_band", "-planes", plane], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()
    out = r.stdout.decode()
    assert "band form: nystroem_path" in out and "Planes: 1 plane filtered through the float colour graph" in out
    assert glf.read_png(os.path.join(str(tmp_path), "results", "plane_0.png")).shape == (72, 96)
    one = glf.read_pfm_rgb(os.path.join(str(tmp_path), "results", "output.pfm"))
    r2 = _run(["-f", src] + ARGS + ["-ngpu", "2", "-ngpu_backend", "loopback"], str(tmp_path))
    assert r2.returncode == 0, r2.stderr.decode()
    assert "rank 1: pixel rows" in r2.stdout.decode()
    two = glf.read_pfm_rgb(os.path.join(str(tmp_path), "results", "output.pfm"))
    np.testing.assert_allclose(two, one, rtol=0, atol=5e-4 / 4.0)     # (tests/test_gpu_rgbf32_multi.py's criterion)


@pytest.mark.parametrize("extra", [["-color"], ["-chroma"], ["-rgb_graph"], ["-depth16"], ["-float32"], ["-no_approx"],
                                   ["-kernel", "bilateral"], ["-kernel", "photometric"]])
def test_float_rgb_flag_errors(tmp_path, extra):
    src, _ = _src(tmp_path)
    r = _run(["-f", src, "-float_rgb"] + extra, str(tmp_path))
    assert r.returncode == 1 and b"-float_rgb" in r.stderr and extra[0].encode() in r.stderr, r.stderr
    assert len(r.stderr.decode().strip().splitlines()) == 1


def test_float_rgb_rejects_a_grey_pfm_a_png_and_a_nan(tmp_path):
    g = str(tmp_path / "grey.pfm")
    glf.write_pfm(g, t._grey_f32_image(40, 48, seed=1))
    r = _run(["-f", g, "-float_rgb"], str(tmp_path))
    assert r.returncode == 1 and b"-float_rgb" in r.stderr and b"Portable Float Map" in r.stderr, r.stderr
    p = str(tmp_path / "g8.png")
    glf.write_png(p, glf.synth_image(40, 32, seed=1))
    r = _run(["-f", p, "-float_rgb"], str(tmp_path))
    assert r.returncode == 1 and b"-float_rgb" in r.stderr and b"Portable Float Map" in r.stderr, r.stderr
    img = t._f32_image(40, 48, seed=1)
    img[7, 9, 1] = np.nan
    q = str(tmp_path / "nan.pfm")
    glf.write_pfm_rgb(q, img)
    r = _run(["-f", q, "-float_rgb", "-num_samples", "60", "-num_eigvals", "8"], str(tmp_path))
    assert r.returncode != 0 and b"NaN" in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "results", "output.pfm"))
