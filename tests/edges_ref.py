"""The reference of the spectral edge map (glf_graph_edges, include/glf.h), in two parts.

(a) An emulation of the pinned arithmetic, bit for bit, in numpy: per (pixel, direction) q = +0, then for c ascending
d = Phi[nb][c] - Phi[px][c] and x = s_c d in float32 (numpy rounds each once, to nearest even, subnormals kept) and
q = fmaf(x, x, q). numpy has no fused multiply-add; fmaf32 builds it: the product of two float32 is exact in float64 (48 bits), the
float64 sum p + q is taken with its exact error (TwoSum) and rounded to odd -- where the sum is inexact, of its two float64
neighbours the one with an odd last bit -- and one cast to float32 then rounds as a single rounding of the exact value would
(float64 carries more than two bits beyond float32, at every float32 exponent, the subnormal ones included).
tests/test_edges_ref.py checks fmaf32 against exact rational arithmetic.

(b) The float64 map q* = sum_c (s_c (Phi[nb][c] - Phi[px][c]))^2 with s = fl32(scale), and its bound ("Spectral edge
map"): |q - q*| <= gamma(dim + 4) q* + dim 2^-149, gamma(n) = n u / (1 - n u), u = 2^-24; the float64 evaluation of q* itself adds
at most (dim + 4) 2^-52 q*, which the bound returned here includes.

`defect` seeds a wrong kernel into the emulation (tests/test_edges_ref.py shows that the comparisons reject each):
  wrap          E and SE at col = W - 1 take the raster neighbour px + 1 / px + W + 1 of the next image row
  swap          SE and SW exchanged
  one_endpoint  the mask tested on the pixel only, not on its neighbour
  scale_after   the scale applied after the square: q += s_c d^2
  split         the chain cut in two halves that are added at the end (numerically fine: for the bit comparison only)"""
import numpy as np

U = 2.0 ** -24
DIRS = ("E", "S", "SE", "SW")
OFFSETS = {"E": (0, 1), "S": (1, 0), "SE": (1, 1), "SW": (1, -1)}
TINY = np.float32(2.0 ** -126)   # the smallest normal float32


def fmaf32(x, y, q):
    """fl32(x y + q) with one rounding, for float32 arrays."""
    x, y, q = (np.asarray(a, dtype=np.float32) for a in (x, y, q))
    p = x.astype(np.float64) * y.astype(np.float64)                  # exact
    b = q.astype(np.float64)
    s = p + b
    bb = s - p
    e = (p - (s - bb)) + (b - bb)                                    # p + b = s + e exactly
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    other = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    odd = np.where((e != 0) & even & np.isfinite(s), other, s)       # round to odd
    return odd.astype(np.float32)


def _geometry(h, w, defect=None):
    """Per direction: (the neighbour's flat index [h, w], clipped into the image, and whether the neighbour is inside)."""
    row, col = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    offs = dict(OFFSETS)
    if defect == "swap":
        offs["SE"], offs["SW"] = offs["SW"], offs["SE"]
    geo = {}
    for d in DIRS:
        dr, dc = offs[d]
        inside = (row + dr < h) & (col + dc >= 0) & (col + dc < w)
        nb = (row + dr) * w + col + dc
        if defect == "wrap" and dc == 1:
            inside = (row + dr < h) & (nb < h * w)
        geo[d] = (np.clip(nb, 0, h * w - 1), inside)
    return geo


def _live(geo, d, valid, defect=None):
    nb, inside = geo[d]
    if valid is None:
        return inside
    v = np.asarray(valid).reshape(-1) != 0
    return inside & v.reshape(inside.shape) & (True if defect == "one_endpoint" else v[nb])


def emulate(phi, scale, dim, h, w, valid=None, defect=None):
    """(planes float32 [4, h, w] in the order of DIRS, whether a non-zero intermediate was subnormal). phi: float32 [h w, >= dim];
    scale: [>= dim], rounded to float32 here; valid: [h, w] or None."""
    phi = np.asarray(phi)
    assert phi.dtype == np.float32 and phi.shape[0] == h * w and phi.shape[1] >= dim
    s = np.asarray(scale, dtype=np.float64).astype(np.float32)
    geo = _geometry(h, w, defect)
    out = np.zeros((4, h, w), dtype=np.float32)
    subnormal = False

    def tiny(a):
        return bool(np.any((a != 0) & (np.abs(a) < TINY)))

    for k, name in enumerate(DIRS):
        nb, _ = geo[name]
        live = _live(geo, name, valid, defect)
        a, b = phi[:, :dim].reshape(h, w, -1), phi[nb][:, :, :dim]
        halves = [np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32)]
        for c in range(dim):
            q = halves[1 if defect == "split" and c >= dim // 2 else 0]
            d = b[:, :, c] - a[:, :, c]
            if defect == "scale_after":
                q[...] = q + s[c] * (d * d)
                continue
            x = s[c] * d
            q[...] = fmaf32(x, x, q)
            subnormal = subnormal or tiny(d[live]) or tiny(x[live]) or tiny(q[live])
        out[k] = np.where(live, halves[0] + halves[1] if defect == "split" else halves[0], np.float32(0.0))
    return out, subnormal


def gamma(n):
    return n * U / (1.0 - n * U)


def exact(phi, scale, dim, h, w, valid=None):
    """(q* float64 [4, h, w], bound [4, h, w], live bool [4, h, w]) on phi's own values with the scale fl32(scale)."""
    p = np.asarray(phi)[:, :dim].astype(np.float64)
    s = np.asarray(scale, dtype=np.float64).astype(np.float32).astype(np.float64)[:dim]
    geo = _geometry(h, w)
    q, live = np.zeros((4, h, w)), np.zeros((4, h, w), dtype=bool)
    for k, name in enumerate(DIRS):
        nb, _ = geo[name]
        live[k] = _live(geo, name, valid)
        x = (p[nb] - p.reshape(h, w, -1)) * s
        q[k] = np.where(live[k], (x * x).sum(axis=2), 0.0)
    return q, (gamma(dim + 4) + (dim + 4) * 2.0 ** -52) * q + dim * 2.0 ** -149, live


def boundary(planes, live, dtype=np.float32):
    """Graph.boundary restated: ([h, w] from the four planes [4, h, w] (E, S, SE, SW) and their live masks, the live count): the
    eight terms added in the library's order, in float32 as the library does, or in float64."""
    e = np.asarray(planes, dtype=dtype)
    h, w = e.shape[1:]
    total, count = np.zeros((h, w), dtype=dtype), np.zeros((h, w), dtype=dtype)
    for k in range(4):
        total += e[k]
        count += live[k]
    total[:, 1:] += e[0, :, :-1]
    count[:, 1:] += live[0, :, :-1]
    total[1:, :] += e[1, :-1, :]
    count[1:, :] += live[1, :-1, :]
    total[1:, 1:] += e[2, :-1, :-1]
    count[1:, 1:] += live[2, :-1, :-1]
    total[1:, :-1] += e[3, :-1, 1:]
    count[1:, :-1] += live[3, :-1, 1:]
    return np.where(count > 0, total / np.maximum(count, 1), 0).astype(dtype), count
