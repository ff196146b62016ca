"""The bound of tests/degree_ref.py separates a right degree kernel from a subtly wrong one. CPU only.

A numpy emulation of the grid-factored degree (degree_ref.emulate_grid: the f32 histogram in ascending column order, the host's
power-of-two scale, the (hi, lo) splits and three products per 16-row k-step, f32 per chunk of 512 rows, f64 over the chunks of a grid
row's reach and over the values) runs on two of the shapes of tests/test_gpu_degree.py, wide_5 (one chunk, a window, 70 grid columns
padded to 72, a width that is no multiple of 4) and window_3 (three chunks). It must pass the bound on every sample for D, Uy and a
signed U_s; with one defect at a time it must not, on both shapes where the defect exists:
  the Er-lo x Wt-hi product left out
  a grid row's chunk range one chunk short                 (window_3: wide_5 has one chunk)
  a grid row's reach one image row short                   (at the largest distance where Er >= 2^-10; see below)
  a padding grid column read in place of the last one      (wide_5: window_3's four columns have no padding)
  the last partial 4-column strip of the direct sweep given weight 1 instead of 0   (a model of degree_chunk_lut's strips; wide_5)
  the histogram weight taken at the neighbouring column    (weighted form)
The reach: the kernels take their radius from the f32 table's first exact zero, so the image row one short of THAT radius weighs less
than 2^-126 of a degree that is at least 1 -- dropping it changes no bit of the result, which test_a_radius_one_short_of_the_exact_zero
asserts. The defect that must break the bound is the same off-by-one where a row still matters.

The table test derives each GPU shape's launch plan (zmfma shape, chunks, m-groups, the window's first m-tiles) from the host's rules and
asserts gamma < 2^-11 / 6 for the grid form at every shape, so that a lost lo product is visible."""
import numpy as np
import pytest

import glf
import oracle as orc
import degree_ref as dref

_CASES = {}
APPLIES = {
    "drop_lo_hi": ("wide_5", "window_3"), "chunk_short": ("window_3",), "reach_short": ("wide_5", "window_3"),
    "padding_column": ("wide_5",), "neighbour_weight": ("wide_5", "window_3"),
}


class _Case:
    pass


def _case(name):
    if name not in _CASES:
        c = _Case()
        c.w, c.h, c.rows, c.cols, c.h_loc, c.idx = dref.shape(name)
        c.img = glf.synth_image(c.w, c.h, seed=3)
        c.plane = dref.signed_plane(c.w, c.h, 1)
        c.ref = dref.reference(c.img, c.idx, c.h_loc, dref.H_VAL, plane=c.plane)
        c.plan = dref.grid_plan(c.w, c.h, c.rows, c.cols, c.h_loc)
        c.g, c.BD, c.BY, c.BS = dref.bounds("grid", c.ref, h_loc=c.h_loc, h_val=dref.H_VAL, width=c.w, radius=c.plan["radius"])
        _CASES[name] = c
    return _CASES[name]


def test_the_reference_is_the_oracles():
    """The chunked float64 reference against the oracle's degree at 1e-13, all rows and a shard."""
    c = _case("wide_5")
    prm = orc.default_params()
    prm.h_loc, prm.h_val = c.h_loc, dref.H_VAL
    np.testing.assert_allclose(c.ref.D, orc.degree(c.img, c.idx, prm), rtol=1e-13)
    shard = dref.reference(c.img, c.idx, c.h_loc, dref.H_VAL, rows=(7, 19))
    np.testing.assert_allclose(shard.D, orc.degree(c.img, c.idx, prm, row0=7, row1=19), rtol=1e-13)
    assert c.ref.Uabs.min() > 0 and (np.abs(c.ref.Us) < 0.2 * c.ref.Uabs).any()      # the signed plane cancels on some samples


@pytest.mark.parametrize("name", ["wide_5", "window_3"])
def test_emulated_grid_form_is_within_the_bound(name):
    c = _case(name)
    D, Uy = dref.emulate_grid(c.img, c.rows, c.cols, c.h_loc, dref.H_VAL)
    Us, _ = dref.emulate_grid(c.img, c.rows, c.cols, c.h_loc, dref.H_VAL, plane=c.plane)
    for what, x, ref, B in (("D", D, c.ref.D, c.BD), ("Uy", Uy, c.ref.Uy, c.BY), ("Us", Us, c.ref.Us, c.BS)):
        ratio, ok = dref.check(x, ref, B)
        print("%s %s: gamma 2^%.2f, worst error / bound %.4f" % (name, what, np.log2(c.g), ratio))
        assert ok, (what, ratio)


@pytest.mark.parametrize("defect", sorted(APPLIES))
@pytest.mark.parametrize("name", ["wide_5", "window_3"])
def test_one_defect_at_a_time_breaks_the_bound(name, defect):
    if name not in APPLIES[defect]:
        c = _case(name)           # the defect does not exist at this shape: say why, by the shape's own numbers
        assert (defect, name) in (("chunk_short", "wide_5"), ("padding_column", "window_3"))
        assert c.plan["chunks"] == 1 if defect == "chunk_short" else c.plan["ncp"] == c.plan["nc"]
        return
    c = _case(name)
    weighted = defect == "neighbour_weight"
    x, _ = dref.emulate_grid(c.img, c.rows, c.cols, c.h_loc, dref.H_VAL, plane=c.plane if weighted else None, defect=defect)
    ratio, ok = dref.check(x, c.ref.Us if weighted else c.ref.D, c.BS if weighted else c.BD)
    print("%s %s: worst error / bound %.1f" % (name, defect, ratio))
    assert not ok and ratio > 1.0, ratio


@pytest.mark.parametrize("name", ["wide_5", "window_3"])
def test_a_radius_one_short_of_the_exact_zero(name):
    """The image row at distance radius - 1 weighs 2^15 Er < 2^-25: a zero (hi, lo) pair. Dropping it changes no bit."""
    c = _case(name)
    assert dref.etab32(c.h_loc, c.plan["radius"])[-1] < 2.0 ** -126
    a = dref.emulate_grid(c.img, c.rows, c.cols, c.h_loc, dref.H_VAL)
    b = dref.emulate_grid(c.img, c.rows, c.cols, c.h_loc, dref.H_VAL, defect="zero_radius_short")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_last_strip_of_the_direct_sweep():
    """degree_chunk_lut pads a row to a multiple of 4 columns with pixels of value 0 and gives them weight 0. With weight 1 the dark
    samples see two more pixels per row (150 = 4 x 37 + 2)."""
    c = _case("wide_5")
    g, BD, _, _ = dref.bounds("direct", c.ref)
    ratio, ok = dref.check(dref.emulate_direct_strips(c.img, c.idx, c.h_loc, dref.H_VAL), c.ref.D, BD)
    print("direct strips: gamma 2^%.2f, worst error / bound %.4f" % (np.log2(g), ratio))
    assert ok, ratio
    ratio, ok = dref.check(dref.emulate_direct_strips(c.img, c.idx, c.h_loc, dref.H_VAL, pad_weight=1.0), c.ref.D, BD)
    print("direct strips, padding weight 1: worst error / bound %.1f" % ratio)
    assert not ok and ratio > 1.0, ratio


def test_plan_and_gamma_of_every_grid_shape():
    """Each GPU shape's realised (p, nr, nc, radius, zmfma shape, chunks, m-groups) from the host's rules, and the gamma condition."""
    idx = glf.Sampling(53, 37, 20)
    assert (sorted(set((idx // 53).tolist())), sorted(set((idx % 53).tolist()))) == tuple(list(g) for g in dref.FIVES_GRID)
    assert dref.zero_radius(40.0, 4096) == 408 and dref.zero_radius(5.0, 4096) == 51      # ceil(10.2 h_loc)
    for name in dref.SHAPES:
        w, h, rows, cols, h_loc, idx = dref.shape(name)
        assert np.all(np.diff(idx.astype(np.int64)) > 0) and idx[-1] < w * h
        pl = dref.grid_plan(w, h, rows, cols, h_loc)
        got = (idx.size, pl["nr"], pl["nc"], pl["radius"], pl["shape"], pl["chunks"], pl["mgroups"])
        assert got == dref.TABLE[name], (name, got)
        g = dref.gamma("grid", width=w, radius=pl["radius"], weighted=True)
        print("%-15s p %4d nr %3d nc %2d radius %3d shape %d chunks %d mgroups %d gamma 2^%.2f" % ((name,) + got + (np.log2(g),)))
        assert g < 2.0 ** -11 / 6, (name, g)
    assert dref.grid_plan(*dref.shape("ten")[:5])["mtiles"] == 7 and dref.grid_plan(*dref.shape("three_groups")[:5])["mtiles"] == 11
    assert dref.grid_plan(*dref.shape("window_3")[:5])["mt0"] == [0, 2, 5]
    # window_refused: chunk 0 reaches five m-tiles
    w, h, rows, cols, h_loc, _ = dref.shape("window_refused")
    assert sum(1 for r in rows if r <= 511 + 50) > 4 * 32
    # ZMFMA_GROUPS=1 on `ten`: groups of five, two of them
    forced = dref.grid_plan(*dref.shape("ten")[:5], zmfma_groups=True)
    assert (forced["shape"], forced["mgroups"]) == (dref.FIVES, 2)
    # the row shards of window_3 and window_refused keep their shapes
    for rows_ in ((300, 900), (0, 1), (1099, 1100), (0, 300), (900, 1100)):
        for name, shp in (("window_3", dref.WINDOW), ("window_refused", dref.TEN)):
            w, h, rows, cols, h_loc, _ = dref.shape(name)
            pl = dref.grid_plan(w, h, rows, cols, h_loc, row0=rows_[0], row1=rows_[1])
            if name == "window_3" or rows_ == (300, 900):
                assert pl["shape"] == shp, (name, rows_, pl)
            print(name, rows_, pl["shape"], pl["chunks"], pl["mgroups"], pl["mt0"])
    # the other forms' gamma, for the record
    for form, kw in (("direct", {}), ("pix", dict(fmt="rgb8")), ("pix", dict(fmt="u16")), ("pix", dict(fmt="f32")), ("pix", dict(fmt="rgbf32")),
                     ("nlm", dict(h_val=3.0))):
        print("%-6s %-7s gamma 2^%.2f" % (form, kw.get("fmt", ""), np.log2(dref.gamma(form, **kw))))
