"""-color -chroma in the host program: the chroma planes go through the luma's graph (glf_image_processing_signals).
The output must equal, byte for byte, the RGB assembled here from the Python call on the same planes; -color alone keeps
the chroma untouched, as before."""
import os
import subprocess

import numpy as np
import pytest
import torch

import glf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "image-processing-graph-laplacian_amd", "image_processing")
SRC = os.path.join(ROOT, "tests", "golden", "pixel_mountains.png")
YUV_FROM_RGB = [[0.299, 0.587, 0.114], [-0.14714119, -0.28886916, 0.43601035], [0.61497538, -0.51496512, -0.10001026]]
NS, M = 300, 16


def _run(args, cwd):
    os.makedirs(os.path.join(cwd, "results"), exist_ok=True)
    return subprocess.run([EXE] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _rgb_from_yuv():
    """The host program's inverse (cofactors over the determinant, in its order of operations)."""
    a = YUV_FROM_RGB
    det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    inv = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            r0, r1, c0, c1 = (j + 1) % 3, (j + 2) % 3, (i + 1) % 3, (i + 2) % 3
            inv[i][j] = (a[r0][c0] * a[r1][c1] - a[r0][c1] * a[r1][c0]) / det
    return inv


def _assemble(zy, u, v):
    inv = _rgb_from_yuv()
    out = np.empty(zy.shape + (3,), dtype=np.uint8)
    for k in range(3):
        x = ((zy * inv[k][0]) + u * inv[k][1]) + v * inv[k][2]
        out[:, :, k] = np.clip(x, 0.0, 255.0).astype(np.uint8)
    return out


def _yuv(rgb):
    R, G, B = (rgb[:, :, c].astype(np.float64) for c in range(3))
    return [(R * a[0] + G * a[1]) + B * a[2] for a in YUV_FROM_RGB]


@pytest.mark.gpu
def test_chroma_needs_color(tmp_path):
    r = _run(["-f", SRC, "-chroma"], str(tmp_path))
    assert r.returncode == 1 and b"-chroma" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flt", ["reference", "smooth"])
def test_color_chroma_matches_python_call(tmp_path, flt):
    rgb = glf.read_png_rgb(SRC)
    y, u, v = _yuv(rgb)
    luma = np.clip(y + 0.5, 0.0, 255.0).astype(np.uint8)
    uv = np.stack([u, v]).astype(np.float32)
    opt = glf.default_options(num_samples=NS, num_eigvals=M, filter_mode={"reference": glf.FILTER_REFERENCE, "smooth": glf.FILTER_SMOOTH}[flt])
    with glf.Context(0) as ctx:
        out, zf, so, _ = ctx.image_processing_signals(ctx.to_device(luma), torch.from_numpy(uv).to(ctx.device), opt, want_float=True)
        zf, so = zf.cpu().numpy().astype(np.float64), so.cpu().numpy().astype(np.float64)
        _, zf_plain, _ = ctx.image_processing(ctx.to_device(luma), opt, want_float=True)
        zf_plain = zf_plain.cpu().numpy().astype(np.float64)
    args = ["-f", SRC, "-color", "-num_samples", str(NS), "-num_eigvals", str(M), "-filter", flt]
    d1, d0 = str(tmp_path / "chroma"), str(tmp_path / "plain")
    r = _run(args + ["-chroma"], d1)
    assert r.returncode == 0, r.stderr.decode()
    assert "Chroma: the U and V planes were filtered through the luma's graph (filter %s)" % flt in r.stdout.decode()
    got = glf.read_png_rgb(os.path.join(d1, "results", "output.png"))
    np.testing.assert_array_equal(got, _assemble(zf, so[0], so[1]))
    # without -chroma: the chroma planes pass through, as before
    r = _run(args, d0)
    assert r.returncode == 0, r.stderr.decode()
    assert "Chroma:" not in r.stdout.decode()
    got0 = glf.read_png_rgb(os.path.join(d0, "results", "output.png"))
    np.testing.assert_array_equal(got0, _assemble(zf_plain, u, v))
    assert np.any(got0 != got)                  # the chroma did change (by less than a grey level at most pixels: m = 16)
