"""The reference of the blend read-out (tests/blend_ref.py) checked on the CPU against a direct restatement of the rule of
include/glf.h that sorts out lo, hi and the weight in Python ints and rationals, pixel by pixel, and rounds the two fused
multiply-adds exactly; and the comparison that tests/test_gpu_graph_blend.py rests on -- the outputs bit for bit (any NaN equal to
any NaN), the slot indices and the weight -- against kernels with seeded defects (emulated: blend_ref's `defect`), one test each.
Names no symbol of the library: passes with or without the feature."""
import math
from fractions import Fraction

import numpy as np
import pytest

import blend_ref as br
from test_edges_ref import _round_f32

CASES = [(1, 2), (1, 32), (4, 8), (16, 2), (3, 10), (2, 3), (1, 5), (6, 5)]
N = 320


def _direct(table, level, nout, nlevels):
    """(out float32 [nout, N], lo, hi int [nout, N], f as Fractions [N]) by the rule text, one pixel at a time."""
    z = np.full((br.SLOTS, table.shape[1]), np.nan, dtype=np.float32)
    z[:table.shape[0]] = table
    n = z.shape[1]
    out = np.empty((nout, n), dtype=np.float32)
    lo_all, hi_all, f_all = np.empty((nout, n), dtype=np.int64), np.empty((nout, n), dtype=np.int64), []
    for px in range(n):
        t = float(level[px])
        if math.isnan(t):
            tc = Fraction(0)
        elif math.isinf(t):
            tc = Fraction(nlevels - 1 if t > 0 else 0)
        else:
            tc = min(max(Fraction(t), Fraction(0)), Fraction(nlevels - 1))
        i = min(math.floor(tc), nlevels - 2)
        f = tc - i
        assert 0 <= f <= 1 and (f < 1 or i == nlevels - 2)
        f_all.append(f)
        for o in range(nout):
            lo = o * nlevels + i
            hi = lo + 1
            assert o * nlevels <= lo and hi < (o + 1) * nlevels                  # both inside the output's bank
            lo_all[o, px], hi_all[o, px] = lo, hi
            zl, zh = z[lo, px], z[hi, px]
            if f == 0:
                out[o, px] = zl
            elif f == 1:
                out[o, px] = zh
            elif np.isfinite(zl) and np.isfinite(zh):
                inner = _round_f32(Fraction(float(zl)) - f * Fraction(float(zl)))
                out[o, px] = _round_f32(f * Fraction(float(zh)) + Fraction(float(inner)))
            else:                                                                 # Inf / NaN: no rounding is involved
                with np.errstate(invalid="ignore"):
                    out[o, px] = np.float32(float(f) * np.float64(zh) + (np.float64(zl) - float(f) * np.float64(zl)))
    return out, lo_all, hi_all, f_all


def _agree(got, want):
    """The comparison: outputs by bits (NaN matches NaN), both slot indices, the weight."""
    out, lo, hi, f = got
    wout, wlo, whi, wf = want
    nan = np.isnan(out) & np.isnan(wout)
    same = bool(np.all(nan | (out.view(np.uint32) == wout.view(np.uint32))))
    same_f = bool(np.array_equal(f.view(np.uint32), np.array([float(x) for x in wf], dtype=np.float32).view(np.uint32)))
    return same and same_f and bool(np.array_equal(lo, wlo)) and bool(np.array_equal(hi, whi))


def _tables(slots, rng):
    """name -> table float32 [slots, N]: random scores, and the adversarial ones."""
    plain = rng.normal(size=(slots, N)).astype(np.float32)
    wide = (rng.normal(size=(slots, N)) * 10.0 ** rng.integers(-30, 30, size=(slots, N))).astype(np.float32)
    wide[:, ::7] = -wide[:, ::7][::-1]
    wide[rng.random((slots, N)) < 0.05] = np.float32(-0.0)
    poison = plain.copy()                                                        # every other slot Inf / NaN: a clean neighbour is one step away
    poison[1::2] = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)[rng.integers(0, 3, size=poison[1::2].shape)]
    poison2 = plain.copy()
    poison2[0::2] = np.float32(np.inf)
    tiny = (plain * np.float32(2.0 ** -140)).astype(np.float32)                  # subnormal scores
    return dict(plain=plain, wide=wide, poison=poison, poison2=poison2, tiny=tiny)


def _runs(defect=None):
    """Every (case, table): whether the emulation (with a defect seeded, or none) agrees with the direct restatement."""
    res = {}
    for nout, nlevels in CASES:
        rng = np.random.default_rng(1000 * nout + nlevels)
        level = br.special_levels(nlevels, N, rng)
        for name, table in _tables(nout * nlevels, rng).items():
            res[(nout, nlevels, name)] = _agree(br.emulate(table, level, nout, nlevels, defect), _direct(table, level, nout, nlevels))
    return res


def test_cases_are_the_stated_ones():
    assert all(nout * nlevels <= br.SLOTS for nout, nlevels in CASES)
    assert {(1, 2), (1, 32), (4, 8), (16, 2), (3, 10)} <= set(CASES)
    level = br.special_levels(8, N, np.random.default_rng(0))
    assert np.isnan(level).sum() == 1 and np.isposinf(level).sum() == 1 and np.isneginf(level).sum() == 1
    assert all((level == b).any() and (level == b + 0.5).any() for b in range(7)) and (level < 0).any() and (level > 7).any()
    assert all((level == np.nextafter(np.float32(b), np.float32(9))).any() and (level == np.nextafter(np.float32(b), np.float32(-9))).any()
               for b in range(1, 8))


def test_slot_ownership():
    assert sorted(br.acc_row(g, h) for h in range(2) for g in range(16)) == list(range(32))
    assert all((br.acc_row(g, h) >> 2) & 1 == h for h in range(2) for g in range(16))
    table = np.arange(32 * 3, dtype=np.float32).reshape(32, 3)
    img = br.image(table)
    assert np.array_equal(img[:32], table) and np.isnan(img[32]).all()
    assert np.array_equal(br.image(table, "wrong_half")[:32], table[np.arange(32) ^ 4])


def test_emulation_is_the_rule():
    res = _runs()
    assert all(res.values()), [key for key, ok in res.items() if not ok]


def _rejected(defect, where=None):
    res = _runs(defect)
    bad = [key for key, ok in res.items() if not ok]
    print("%s: rejected in %d of %d runs" % (defect, len(bad), len(res)))
    assert bad, defect
    if where is not None:
        assert any(key[2] == where for key in bad), (defect, where, bad)


def test_rejects_swapped_weights():
    _rejected("swap", "plain")


def test_rejects_an_uncapped_i():
    _rejected("uncapped")


def test_rejects_a_missing_clamp_at_zero():
    _rejected("no_clamp0", "plain")


def test_rejects_hi_from_the_next_output():
    _rejected("hi_next", "plain")


def test_rejects_the_wrong_half_wave():
    _rejected("wrong_half", "plain")


def test_rejects_the_plain_lerp_at_f_1_by_bits():
    """f (z_hi - z_lo) + z_lo at f = 1: (z_hi - z_lo) + z_lo is not z_hi in general."""
    _rejected("plain_lerp", "plain")
    nout, nlevels = 1, 2
    table = np.array([[1.0], [np.float32(1e-8)]], dtype=np.float32)
    level = np.array([1.0], dtype=np.float32)
    got = br.emulate(table, level, nout, nlevels, "plain_lerp")[0]
    want = br.emulate(table, level, nout, nlevels)[0]
    assert want[0, 0] == np.float32(1e-8) and got[0, 0].view(np.uint32) != want[0, 0].view(np.uint32)


def test_rejects_a_missing_f_0_select_by_an_inf_beside():
    """Without the select the lerp runs at f = 0: 0 * Inf is a NaN where the rule returns z_lo."""
    res = _runs("no_f0")
    assert not any(ok for key, ok in res.items() if key[2] in ("poison", "poison2")), res
    table = np.array([[2.0], [np.inf]], dtype=np.float32)
    level = np.array([0.0], dtype=np.float32)
    assert br.emulate(table, level, 1, 2)[0][0, 0] == 2.0 and np.isnan(br.emulate(table, level, 1, 2, "no_f0")[0][0, 0])


@pytest.mark.parametrize("nout,nlevels", [(1, 2), (4, 8)])
def test_an_unselected_slot_never_reaches_the_output(nout, nlevels):
    """Overwriting, per pixel, every slot but the ones taken with a weight other than zero changes no bit."""
    rng = np.random.default_rng(9)
    level = br.special_levels(nlevels, N, rng)
    table = rng.normal(size=(nout * nlevels, N)).astype(np.float32)
    out, lo, hi, f = br.emulate(table, level, nout, nlevels)
    poisoned = np.full_like(table, np.nan)
    px = np.arange(N)
    for o in range(nout):
        keep_lo, keep_hi = f != 1, f != 0
        poisoned[lo[o][keep_lo], px[keep_lo]] = table[lo[o][keep_lo], px[keep_lo]]
        poisoned[hi[o][keep_hi], px[keep_hi]] = table[hi[o][keep_hi], px[keep_hi]]
    again = br.emulate(poisoned, level, nout, nlevels)[0]
    assert np.isfinite(out).all() and np.array_equal(out.view(np.uint32), again.view(np.uint32))
