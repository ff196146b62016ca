"""-planes in the host program: grey PNGs (8 or 16 bits) go as float planes through the graph of the 16-bit image (-depth16) or of
the colour image (-color -rgb_graph). results/output.png must be the run's without -planes byte for byte, and results/plane_<k>.png
the Python binding's plane rounded as clamp(floor(z + 0.5)) at the input plane's bit depth. Without one of the two modes the flag is
a usage error, and so is a plane of another size."""
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

pytestmark = pytest.mark.gpu


def _run(args, cwd, env_keys=None):
    os.makedirs(os.path.join(cwd, "results"), exist_ok=True)
    env = dict(os.environ)
    for k, v in (env_keys or {}).items():
        env["GLF_" + k] = v
    return subprocess.run([EXE] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _plane_files(tmp_path, h, w):
    """An 8-bit plane (a.png: a soft ramp with a square) and a 16-bit one (b16.png: a depth-like disc under noise): (paths, float
    planes [2, h, w], bit depths)."""
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    a = 40.0 + 150.0 * c / max(1, w - 1)
    a[h // 4: h // 2, w // 4: w // 2] = 230.0
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    b = 1000.0 + 400.0 * disc + np.random.default_rng(5).normal(0.0, 15.0, (h, w))
    b = np.clip(np.rint(b), 0, 65535).astype(np.uint16)
    pa, pb = str(tmp_path / "a.png"), str(tmp_path / "b16.png")
    glf.write_png(pa, a)
    glf.write_png16(pb, b)
    return [pa, pb], np.stack([a.astype(np.float32), b.astype(np.float32)]), (8, 16)


def _rounded(z, bits):
    return np.clip(np.floor(z.astype(np.float64) + 0.5), 0, 65535 if bits == 16 else 255).astype(np.uint16 if bits == 16 else np.uint8)


def _check_planes(tmp_path, so, bits, stdout, graph):
    for k, b in enumerate(bits):
        path = os.path.join(str(tmp_path), "results", "plane_%d.png" % k)
        got = glf.read_png16(path) if b == 16 else glf.read_png(path)
        np.testing.assert_array_equal(got, _rounded(so[k], b), err_msg="plane %d" % k)
    assert "Planes: %d planes filtered through the %s graph (filter reference)" % (len(bits), graph) in stdout.splitlines()


@pytest.mark.parametrize("extra", [[], ["-color"], ["-color", "-chroma"], ["-fused"]])
def test_planes_without_its_modes_is_a_usage_error(tmp_path, extra):
    r = _run(["-f", SRC_RGB, "-planes", SRC_RGB] + extra, str(tmp_path))
    assert r.returncode == 1 and b"-planes" in r.stderr and b"needs -depth16 or -color -rgb_graph" in r.stderr, r.stderr
    assert len(r.stderr.decode().strip().splitlines()) == 1


@pytest.mark.parametrize("mode", ["depth16", "rgb"])
def test_a_plane_of_another_size_is_an_error(tmp_path, mode):
    rgb = glf.read_png_rgb(SRC_RGB)
    h, w = rgb.shape[:2]
    small = str(tmp_path / "small.png")
    glf.write_png(small, np.zeros((h - 1, w), dtype=np.uint8))
    if mode == "depth16":
        src = str(tmp_path / "in16.png")
        glf.write_png16(src, _u16_image(h, w, seed=12))
        args = ["-f", src, "-depth16"]
    else:
        args = ["-f", SRC_RGB, "-color", "-rgb_graph"]
    r = _run(args + ["-planes", small, "-num_samples", str(NS), "-num_eigvals", str(M)], str(tmp_path))
    assert r.returncode == 1 and b"-planes" in r.stderr and b"small.png" in r.stderr, r.stderr


def test_color_rgb_graph_planes_match_python_call(tmp_path):
    rgb = glf.read_png_rgb(SRC_RGB)
    h, w = rgb.shape[:2]
    files, sig, bits = _plane_files(tmp_path, h, w)
    opt = glf.default_options(num_samples=NS, num_eigvals=M)
    with glf.Context(0) as ctx:
        _, _, so, _ = ctx.image_processing_rgb_signals(torch.from_numpy(rgb).to(ctx.device), torch.from_numpy(sig).to(ctx.device), opt)
        so = so.cpu().numpy()
    args = ["-f", SRC_RGB, "-color", "-rgb_graph", "-num_samples", str(NS), "-num_eigvals", str(M)]
    r0 = _run(args, str(tmp_path))
    assert r0.returncode == 0, r0.stderr.decode()
    plain = open(os.path.join(str(tmp_path), "results", "output.png"), "rb").read()
    r = _run(args + ["-planes", ",".join(files)], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()
    assert open(os.path.join(str(tmp_path), "results", "output.png"), "rb").read() == plain
    _check_planes(tmp_path, so, bits, r.stdout.decode(), "colour")
    assert "Planes:" not in r0.stdout.decode()


@pytest.mark.parametrize("band", [False, True])
def test_depth16_planes_match_python_call(tmp_path, band):
    h, w = 72, 96
    img = _u16_image(h, w, seed=12)
    src = str(tmp_path / "in16.png")
    glf.write_png16(src, img)
    files, sig, bits = _plane_files(tmp_path, h, w)
    keys = dict(NYS_PATH="band", MV_PATH="band") if band else {}
    opt = glf.default_options(num_samples=NS, num_eigvals=M, h_val=30.0 * 257.0)
    with glf.Context(0) as ctx:
        if band:
            ctx.set_tuning(PIX_BAND="1", **keys)
        _, _, so, info = ctx.image_processing_u16_signals(torch.from_numpy(img).to(ctx.device), torch.from_numpy(sig).to(ctx.device), opt)
        so = so.cpu().numpy()
    assert (info["nystroem_path"], info["matvec_path"]) == ((4, 4) if band else (0, 0))
    args = ["-f", src, "-depth16", "-num_samples", str(NS), "-num_eigvals", str(M)] + (["-pix_band"] if band else [])
    r0 = _run(args, str(tmp_path), keys)
    assert r0.returncode == 0, r0.stderr.decode()
    plain = open(os.path.join(str(tmp_path), "results", "output.png"), "rb").read()
    r = _run(args + ["-planes", ",".join(files)], str(tmp_path), keys)
    assert r.returncode == 0, r.stderr.decode()
    assert open(os.path.join(str(tmp_path), "results", "output.png"), "rb").read() == plain
    if band:
        assert "band form: nystroem_path 4, matvec_path 4" in r.stdout.decode().splitlines()
    _check_planes(tmp_path, so, bits, r.stdout.decode(), "16-bit")


def test_depth16_planes_on_two_loopback_ranks(tmp_path):
    """-depth16 -ngpu 2 goes through glf_multi_image_processing_u16_signals: the planes of the Python world's call."""
    h, w = 72, 96
    img = _u16_image(h, w, seed=12)
    src = str(tmp_path / "in16.png")
    glf.write_png16(src, img)
    files, sig, bits = _plane_files(tmp_path, h, w)
    opt = glf.default_options(num_samples=NS, num_eigvals=M, h_val=30.0 * 257.0)
    with glf.Multi(2, devices=[0, 0], backend=glf.MULTI_LOOPBACK) as world:
        want, _, so, _ = world.image_processing_u16_signals(img, sig, opt)
    r = _run(["-f", src, "-depth16", "-ngpu", "2", "-ngpu_backend", "loopback", "-num_samples", str(NS), "-num_eigvals", str(M),
              "-planes", ",".join(files)], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()
    np.testing.assert_array_equal(glf.read_png16(os.path.join(str(tmp_path), "results", "output.png")), want)
    _check_planes(tmp_path, so, bits, r.stdout.decode(), "16-bit")
