"""The bound of tests/nystroem_ref.py separates a right direct split-f16 Nystroem kernel from a subtly wrong one. CPU only.

A numpy emulation of k_nystroem_f16s (column scales, hi / lo splits of 2^15 K and of the scaled Psi, three products per step, f32
accumulation in chunk order) runs on the "tiny" and "mid" shapes of tests/test_gpu_nystroem.py with K_B from the oracle and the test
block of nystroem_ref.make_block. It must pass the bound gamma (K_B^T |Psi|) + a of the f16s form on every element; the same
emulation with one defect at a time must not:
  the lo x hi product left out                      (2^-11 of a product against a gamma below 2^-13.6)
  the last 64-sample chunk left out                 (the unit vector at sample p - 1 reads nothing)
  one sample's entries taken at the next pixel      (a column index off by one: the unit vector at that sample shows the shifted row)
  the farthest grid row of samples dropped          (a band one row too short)
  a rounded inverse scale on one column             (one binade off)
Where the bound is zero (the all-zero column, the padding) the result must be exactly zero; no element is left out."""
import numpy as np
import pytest

import glf
import oracle as orc
import nystroem_ref as nref

S = np.float32(-1.0 / 1500.0)        # a scale of the size of -alpha, with a lo half
_CASES = {}


class _Case:
    pass


def _case(shape):
    if shape not in _CASES:
        w, h, ns, seed, h_loc, p, nr, nc = nref.SHAPES[shape]
        c = _Case()
        c.w, c.h, c.p, c.nr, c.nc = w, h, p, nr, nc
        c.img = glf.synth_image(w, h, seed=seed)
        c.idx = glf.Sampling(w, h, ns)
        assert c.idx.size == p and nref.grid_shape(c.idx, w) == (nr, nc)
        _, KB = orc.affinity(c.img, c.idx, want_KB=True)          # [p, N - p], the non-sample pixels in raster order
        c.K = np.ascontiguousarray(KB.T)
        c.phi_A, c.pinv = nref.make_block(p, 64, 59, seed=21)
        c.Psi = nref.psi64(c.phi_A, np.r_[c.pinv, np.zeros(5, dtype=np.float32)], S)
        c.ref = nref.reference(c.img, c.idx, c.Psi, h_loc, nref.H_VAL)
        # the reference's kernel (the definition, in chunks of image rows) is the oracle's, pixel for pixel
        np.testing.assert_allclose(c.ref.rowsum, c.K.sum(axis=1), rtol=1e-13)
        assert (np.abs(c.ref.phi - c.K @ c.Psi) <= 1e-13 * c.ref.kabs).all()
        assert c.ref.first == p and c.ref.pixels.size == w * h - p
        c.psi32 = nref.psi32(c.phi_A, np.r_[c.pinv, np.zeros(5, dtype=np.float32)], S)
        _CASES[shape] = c
    return _CASES[shape]


def _run(c, defect=None, **kw):
    g = nref.gamma("f16s", c.p)
    B = nref.bound("f16s", g, c.ref, c.Psi)
    Phi = nref.emulate_direct_f16s(c.K, c.psi32, defect=defect, **kw)
    return nref.check(Phi, c.ref.phi, B) + (g, B, Phi)


@pytest.mark.parametrize("shape", ["tiny", "mid"])
def test_emulated_kernel_is_within_the_bound(shape):
    c = _case(shape)
    ratio, ok, g, B, Phi = _run(c)
    print("%s: gamma 2^%.2f, worst |Phi - Phi_ref| / bound %.3f" % (shape, np.log2(g), ratio))
    assert ok, ratio
    # the bound is positive wherever the reference is not zero, and zero exactly on the all-zero column and the padding
    assert (B[c.ref.phi != 0] > 0).all()
    zero_cols = [nref.COL_ZERO] + list(range(59, 64))
    assert not B[:, zero_cols].any() and not Phi[:, zero_cols].any()
    assert (B[:, [j for j in range(59) if j != nref.COL_ZERO]] > 0).all()
    # (the LUT kernel's smaller c: the emulation, which has no generation error at all, passes that bound too)
    assert nref.check(Phi, c.ref.phi, nref.bound("f16s_lut", nref.gamma("f16s_lut", c.p), c.ref, c.Psi))[1]


@pytest.mark.parametrize("shape", ["tiny", "mid"])
@pytest.mark.parametrize("defect", nref.DEFECTS)
def test_one_defect_at_a_time_breaks_the_bound(shape, defect):
    c = _case(shape)
    kw = {}
    if defect == "column_off_by_one":
        kw = dict(sample=c.p // 2)
    elif defect == "band_row_short":
        kw = dict(grid=(c.nr, c.nc, (c.idx // c.w).astype(np.int64)), width=c.w, pixels=c.ref.pixels)
    elif defect == "rounded_inverse_scale":
        mx = np.abs(c.psi32).max(axis=0)
        frac = np.where(mx > 0, np.frexp(mx)[0], 0.0)
        col = int(np.argmax(frac[:59] > 0.75))                  # (a maximum above sqrt(2) 2^k: round(log2) is k + 1, floor is k)
        assert frac[col] > 0.75
        kw = dict(column=col)
    ratio, ok, g, B, Phi = _run(c, defect=defect, **kw)
    print("%s %s: worst |Phi - Phi_ref| / bound %.1f" % (shape, defect, ratio))
    assert not ok and ratio > 1.0, ratio


# chains whose gamma is not below 2^-16, with the reason; nothing else may reach it. A form name alone: at every shape.
LONG_CHAINS = {
    "f32": "v_exp_f32's argument carries three roundings, each amplified by up to 150 ln 2: c = 316 alone is 2^-15.7",
    "pix_f32": "as f32, with dist2's roundings in the exponent as well",
    ("f16s", "big"): "v_exp_f32's argument carries four roundings amplified by up to 40.5 ln 2 (c = 120) and s = 3 is 12 u: 124 links are "
                     "left, and the twelve chunks of p = 720 make 144",
}


def test_counts_of_every_form_at_the_gpu_shapes():
    """gamma per form at the shapes and widths tests/test_gpu_nystroem.py runs them at (p, nr, nc as realised; the pixel formats on tiny
    and mid). gamma < 2^-11 / 6 everywhere, so that a lost lo product (2^-11 of a product) is always visible; gamma < 2^-16 except for the
    chains of LONG_CHAINS."""
    seen_long = set()
    for name, (w, h, ns, seed, h_loc, p, nr, nc) in nref.SHAPES.items():
        assert nr * nc == p
        forms = sorted({(f, None) for f, ld in nref.bound_forms(name)})
        if name in ("tiny", "mid"):
            forms += [("pix_f32", fmt) for fmt in nref.PIX_EXPONENT_ROUNDINGS] + [("pix_band", None)]
        for form, fmt in forms:
            kw = dict(nr=nr, nc=nc, fmt=fmt)
            K, s, c = nref.counts(form, p, **kw)
            g = nref.gamma(form, p, **kw)
            print("%-7s %-9s %-7s K %4d s %d c %3d gamma 2^%.2f" % (name, form, fmt or "", K, s, c, np.log2(g)))
            assert g < 2.0 ** -11 / 6, (name, form, g)
            key = form if form in LONG_CHAINS else (form, name)
            if key in LONG_CHAINS:
                assert g >= 2.0 ** -16, (name, form, g)
                seen_long.add(key)
            else:
                assert g < 2.0 ** -16, (name, form, g)
    assert seen_long == set(LONG_CHAINS)
    # the LUT kernel runs where the test expects it
    assert [s for s in nref.SHAPES if nref.lut_runs(s, 64)] == ["lut", "mid", "big", "narrow"]
    assert not any(nref.lut_runs(s, 128) for s in nref.SHAPES) and not nref.lut_runs("mid", 32, no_lut=True)
