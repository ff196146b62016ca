"""Guides in the colour, 16-bit and float pixel formats for the stage tests (tests/test_gpu_operator.py, tests/test_gpu_nystroem.py): one
pattern per (size, seed) in each format's range, with the format's kernel id, h_val and numpy reference module."""
import numpy as np

import glf
import rgb_ref
import u16_ref

FORMATS = ("rgb8", "u16", "f32", "rgbf32")


def pattern(h, w, seed, channels):
    """Smooth ramps, a disc of another level and noise, per channel, in 0 .. 1."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    disc = (r - h / 2) ** 2 + (c - w / 3) ** 2 < (min(h, w) / 4) ** 2
    planes = []
    for k in range(channels):
        v = 0.2 + 0.5 * (c / max(1, w - 1) if k != 1 else 1.0 - r / max(1, h - 1)) + 0.15 * np.sin((r + 3 * k) / 9.0)
        v[disc] = (0.85, 0.15, 0.6)[k]
        planes.append(np.clip(v + rng.normal(0.0, 0.025, v.shape), 0.0, 1.0))
    return np.stack(planes, axis=2) if channels == 3 else planes[0]


def pix_case(fmt, w, h, seed):
    """(image, kernel, h_val, reference module) of a pixel format: the pattern in the format's range, h_val 30 / 255 of that range."""
    if fmt == "rgb8":
        return np.rint(255.0 * pattern(h, w, seed, 3)).astype(np.uint8), glf.KERNEL_BILATERAL_RGB, 30.0, rgb_ref
    if fmt == "u16":
        return np.rint(65535.0 * pattern(h, w, seed, 1)).astype(np.uint16), glf.KERNEL_BILATERAL_U16, 30.0 * 257.0, u16_ref
    if fmt == "f32":          # signed fractional values, -35 .. +30.5
        return (65.535 * pattern(h, w, seed, 1) - 35.0).astype(np.float32), glf.KERNEL_BILATERAL_F32, 30.0 * 257.0 / 1000.0, u16_ref
    return (63.75 * pattern(h, w, seed, 3) - 20.0).astype(np.float32), glf.KERNEL_BILATERAL_RGBF32, 30.0 / 4.0, rgb_ref
