"""-depth16 in the host program: a 16-bit grey PNG is filtered on its 16-bit values (glf_image_processing_u16) and the output is
written as a 16-bit grey PNG. The output must equal the Python binding's, value for value; the flag refuses 8-bit input and the
colour and full-matrix flags; without it a 16-bit input is rejected as before."""
import os
import subprocess

import numpy as np
import pytest
import torch

import glf
from test_gpu_u16 import _u16_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "image-processing-graph-laplacian_amd", "image_processing")
NS, M = 300, 16

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    os.makedirs(os.path.join(cwd, "results"), exist_ok=True)
    return subprocess.run([EXE] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _src16(tmp_path):
    img = _u16_image(72, 96, seed=12)
    p = str(tmp_path / "in16.png")
    glf.write_png16(p, img)
    return p, img


@pytest.mark.parametrize("flt", ["reference", "smooth"])
def test_depth16_matches_python_call(tmp_path, flt):
    src, img = _src16(tmp_path)
    opt = glf.default_options(num_samples=NS, num_eigvals=M, h_val=30.0 * 257.0,
                              filter_mode={"reference": glf.FILTER_REFERENCE, "smooth": glf.FILTER_SMOOTH}[flt])
    with glf.Context(0) as ctx:
        want, _, _ = ctx.image_processing_u16(torch.from_numpy(img).to(ctx.device), opt)
        want = want.cpu().numpy()
    r = _run(["-f", src, "-depth16", "-num_samples", str(NS), "-num_eigvals", str(M), "-filter", flt], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()
    out = r.stdout.decode()
    assert "Computing Nystr" in out and "Total computation time" in out
    got = glf.read_png16(os.path.join(str(tmp_path), "results", "output.png"))
    np.testing.assert_array_equal(got, want)
    assert np.any(got != img)


def test_depth16_two_loopback_ranks(tmp_path):
    src, img = _src16(tmp_path)
    r1 = _run(["-f", src, "-depth16", "-num_samples", str(NS), "-num_eigvals", str(M)], str(tmp_path))
    assert r1.returncode == 0, r1.stderr.decode()
    one = glf.read_png16(os.path.join(str(tmp_path), "results", "output.png"))
    r2 = _run(["-f", src, "-depth16", "-num_samples", str(NS), "-num_eigvals", str(M), "-ngpu", "2", "-ngpu_backend", "loopback"],
              str(tmp_path))
    assert r2.returncode == 0, r2.stderr.decode()
    assert "rank 1: pixel rows" in r2.stdout.decode()
    two = glf.read_png16(os.path.join(str(tmp_path), "results", "output.png"))
    assert np.mean(one != two) < 1e-3 and int(np.abs(one.astype(np.int64) - two).max()) <= 1


@pytest.mark.parametrize("extra", [["-color"], ["-chroma"], ["-rgb_graph"], ["-no_approx"]])
def test_depth16_flag_errors(tmp_path, extra):
    src, _ = _src16(tmp_path)
    r = _run(["-f", src, "-depth16"] + extra, str(tmp_path))
    assert r.returncode == 1 and b"-depth16" in r.stderr and extra[0].encode() in r.stderr, r.stderr
    assert len(r.stderr.decode().strip().splitlines()) == 1


def test_depth16_rejects_8_bit_input(tmp_path):
    p = str(tmp_path / "g8.png")
    glf.write_png(p, glf.synth_image(40, 32, seed=1))
    r = _run(["-f", p, "-depth16"], str(tmp_path))
    assert r.returncode == 1 and b"-depth16" in r.stderr and b"8-bit" in r.stderr, r.stderr


def test_16_bit_input_without_the_flag_still_fails(tmp_path):
    src, _ = _src16(tmp_path)
    r = _run(["-f", src], str(tmp_path))
    assert r.returncode == 1 and b"Could not read" in r.stderr, r.stderr
