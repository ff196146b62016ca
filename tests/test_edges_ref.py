"""The reference of the spectral edge map (tests/edges_ref.py) checked on the CPU: its fused multiply-add against exact rational
arithmetic, its bound against its own emulation, and both comparisons of tests/test_gpu_graph_edges.py -- bit for bit against the
emulation, within the bound of the float64 map -- against kernels with seeded defects (emulated: edges_ref's `defect`)."""
from fractions import Fraction

import numpy as np
import pytest

import edges_ref as er

H, W, LD, DIM = 13, 11, 8, 5


def _round_f32(v):
    """The Fraction v rounded to the nearest float32, ties to even, subnormals kept (|v| well inside the float32 range)."""
    if v == 0:
        return np.float32(0.0)
    sign, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                                      # 2^e <= a < 2^(e + 1)
    shift = max(e, -126) - 23                                        # the last place of a float32 at that exponent
    scaled = a / Fraction(2) ** shift
    n, rest = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rest
    if twice > scaled.denominator or (twice == scaled.denominator and n & 1):
        n += 1
    return np.float32(sign * float(Fraction(n) * Fraction(2) ** shift))   # (exact: n has at most 25 bits)


def test_fmaf32_against_exact_arithmetic():
    rng = np.random.default_rng(1)
    n = 4000
    x = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-60, 11, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    q = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-120, 21, n)).astype(np.float32)
    # the cases a plain double rounding gets wrong: q a neighbour of x^2, x^2 a tie of q's last place, q = 0
    q[:800] = (x[:800].astype(np.float64) ** 2).astype(np.float32)
    q[800:1200] = np.float32(0.0)
    x[1200:1600] = (np.sqrt(q[1200:1600].astype(np.float64)) * 2.0 ** -12).astype(np.float32)
    got = er.fmaf32(x, x, q)
    bad = 0
    for i in range(n):
        want = _round_f32(Fraction(float(x[i])) * Fraction(float(x[i])) + Fraction(float(q[i])))
        bad += int(got[i].view(np.uint32) != want.view(np.uint32))
    assert bad == 0, "%d of %d fused multiply-adds differ from the exactly rounded value" % (bad, n)
    # and the construction is needed: rounding the float64 sum to nearest first is wrong somewhere in this set
    naive = (x.astype(np.float64) * x.astype(np.float64) + q.astype(np.float64)).astype(np.float32)
    print("double rounding differs from fmaf32 in %d of %d" % (int(np.count_nonzero(naive != got)), n))


def _case(seed=0):
    rng = np.random.default_rng(seed)
    phi = rng.normal(size=(H * W, LD)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, LD)
    valid = (rng.uniform(size=(H, W)) >= 0.2).astype(np.uint8)
    return phi, scale, valid


def _bits_equal(a, b):
    return bool(np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32)))


def _within(got, q, bound):
    return bool(np.all(np.abs(got.astype(np.float64) - q) <= bound))


@pytest.mark.parametrize("masked", [False, True])
def test_emulation_is_within_its_bound_and_keeps_the_contract(masked):
    phi, scale, valid = _case()
    v = valid if masked else None
    out, subnormal = er.emulate(phi, scale, DIM, H, W, v)
    assert not subnormal
    q, bound, live = er.exact(phi, scale, DIM, H, W, v)
    assert _within(out, q, bound)
    frac = float((np.abs(out - q) / bound)[live].max())
    print("worst fraction of the bound %.3f" % frac)
    assert 0.0 < frac <= 1.0
    # +0 by bits wherever the edge is not live: the borders of each direction and the masked endpoints
    assert not out.view(np.uint32)[~live].any()
    assert not live[0][:, -1].any() and not live[2][:, -1].any() and not live[3][:, 0].any() and not live[1:, -1, :].any()
    assert live[0][:, :-1].all() or masked
    # zero-scale columns, appended or interleaved, change nothing; the scale times 2 gives the planes times 4
    s0 = np.concatenate([scale[:DIM], [0.0, 0.0]])
    _phi = np.concatenate([phi[:, :DIM], phi[:, :2]], axis=1)
    assert _bits_equal(er.emulate(_phi, s0, DIM + 2, H, W, v)[0], out)
    s1 = np.array([scale[0], 0.0, scale[1], scale[2], 0.0, scale[3], scale[4]])
    _phi = phi[:, [0, 6, 1, 2, 7, 3, 4]]
    assert _bits_equal(er.emulate(np.ascontiguousarray(_phi), s1, 7, H, W, v)[0], out)
    assert _bits_equal(er.emulate(phi, 2.0 * scale, DIM, H, W, v)[0], np.float32(4.0) * out)


@pytest.mark.parametrize("defect", ["wrap", "swap", "one_endpoint", "scale_after", "split"])
def test_seeded_defects_are_rejected(defect):
    phi, scale, valid = _case()
    out, _ = er.emulate(phi, scale, DIM, H, W, valid)
    q, bound, _ = er.exact(phi, scale, DIM, H, W, valid)
    bad, _ = er.emulate(phi, scale, DIM, H, W, valid, defect=defect)
    assert not _bits_equal(bad, out), "the bit comparison accepts the defect"
    if defect == "split":
        assert _within(bad, q, bound)                                 # (another order of the same sum: the bound cannot tell)
    else:
        assert not _within(bad, q, bound), "the bound accepts the defect"


def test_boundary_restatement():
    phi, scale, valid = _case()
    out, _ = er.emulate(phi, scale, DIM, H, W, valid)
    _, _, live = er.exact(phi, scale, DIM, H, W, valid)
    b, count = er.boundary(out, live)
    assert count.max() == 8 and count.min() == 0
    v = valid != 0
    for (r, c) in ((0, 0), (5, 5), (H - 1, W - 1), (H - 1, 0), (3, W - 1)):
        terms = []
        for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1), (0, -1), (-1, 0), (-1, -1), (-1, 1)):
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and v[r, c] and v[rr, cc]:
                terms.append(float((((phi[rr * W + cc, :DIM].astype(np.float64) - phi[r * W + c, :DIM]) *
                                     scale[:DIM].astype(np.float32).astype(np.float64)) ** 2).sum()))
        want = sum(terms) / len(terms) if terms else 0.0
        assert len(terms) == count[r, c]
        assert abs(float(b[r, c]) - want) <= 32 * er.U * want, (r, c)
