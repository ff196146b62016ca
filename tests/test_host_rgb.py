"""-color -rgb_graph in the host program: the graph is built from the RGB differences (glf_image_processing_rgb) and R, G, B are
filtered through it. The output must equal the Python binding's, byte for byte; the flag needs -color and excludes -chroma."""
import os
import subprocess

import numpy as np
import pytest
import torch

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "image-processing-graph-laplacian_amd", "image_processing")
SRC = os.path.join(ROOT, "tests", "golden", "pixel_mountains.png")
NS, M = 300, 16

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    os.makedirs(os.path.join(cwd, "results"), exist_ok=True)
    return subprocess.run([EXE] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize("extra,needle", [(["-rgb_graph"], b"needs -color"), (["-color", "-chroma", "-rgb_graph"], b"-chroma")])
def test_rgb_graph_flag_errors(tmp_path, extra, needle):
    r = _run(["-f", SRC] + extra, str(tmp_path))
    assert r.returncode == 1 and b"-rgb_graph" in r.stderr and needle in r.stderr, r.stderr


@pytest.mark.parametrize("flt", ["reference", "smooth"])
def test_color_rgb_graph_matches_python_call(tmp_path, flt):
    rgb = glf.read_png_rgb(SRC)
    opt = glf.default_options(num_samples=NS, num_eigvals=M, filter_mode={"reference": glf.FILTER_REFERENCE, "smooth": glf.FILTER_SMOOTH}[flt])
    with glf.Context(0) as ctx:
        want, _, _ = ctx.image_processing_rgb(torch.from_numpy(rgb).to(ctx.device), opt)
        want = want.cpu().numpy()
    r = _run(["-f", SRC, "-color", "-rgb_graph", "-num_samples", str(NS), "-num_eigvals", str(M), "-filter", flt], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()
    assert "graph from the RGB differences" in r.stdout.decode()
    got = glf.read_png_rgb(os.path.join(str(tmp_path), "results", "output.png"))
    np.testing.assert_array_equal(got, want)
    assert np.any(got != rgb)
