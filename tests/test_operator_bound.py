"""The bound of tests/operator_ref.py separates a right split-f16 sweep from a subtly wrong one. CPU only.

A numpy emulation of the stored split-f16 form (hi = float16(v), lo = float16(v - hi), the three products accumulated in float32 in
tile order, the power-of-two column scales of k_mv_col_absmax, K slabs summed in order) is applied to the golden L_A of
tests/golden/syn32.npz (p = 9) and to the Laplacian of 300 requested samples (320 realised) built with the oracle on a 192 x 64
synthetic image (the "mid" shape of tests/test_gpu_operator.py). It must pass the bound gamma (|L| |X|) + a of the f16s form -- K = 12 ceil(T / ksplit) + ksplit,
s = 3 -- and the same emulation with one defect at a time must not:
  the lo x hi product left out            (2^-11 of a product; gamma is 2^-17.8 at p = 320, ksplit = 1)
  the last K tile one binade too large    (a mis-scaled tile)
  one row taking its neighbour's degree   (a wrong row of D in L_A's diagonal)"""
import numpy as np
import pytest

import glf
import oracle as orc
import operator_ref as oref


def _golden(golden):
    g = golden("syn32.npz")
    return g["K_A"], g["D_A"], float(g["alpha"])


def _mid():
    img = glf.synth_image(192, 64, seed=5)
    idx = glf.Sampling(192, 64, 300)
    KA, _ = orc.affinity(img, idx, want_KB=False)
    D = orc.degree(img, idx)
    return KA, D, 1.0 / D.mean()


_CASES = {}


def _case(name, golden):
    if name not in _CASES:
        KA, D, alpha = _golden(golden) if name == "syn32" else _mid()
        _CASES[name] = (KA, D, alpha)
    return _CASES[name]


def _laplacian32(KA, D, alpha, wrong_degree_row=None):
    d = D.copy()
    if wrong_degree_row is not None:
        d[wrong_degree_row] = D[wrong_degree_row + 1]
    return (alpha * (np.diag(d) - KA)).astype(np.float32)


def _run(KA, D, alpha, ld, ksplit, defect=None, wrong_degree_row=None):
    p = D.size
    X = oref.make_block(p, ld, ld - 5, seed=11)
    A = _laplacian32(KA, D, alpha)                        # the reference: the right stored matrix, f32 bits widened
    A64, X64 = A.astype(np.float64), X[:p].astype(np.float64)
    Yref = A64 @ X64
    absL = np.abs(A64)
    g = oref.gamma("f16s", p, ksplit=ksplit)
    B = oref.bound("f16s", g, absL @ np.abs(X64), X64, p, absL_rowsum=absL.sum(axis=1))
    Y = oref.emulate_f16s(_laplacian32(KA, D, alpha, wrong_degree_row), X, p, ksplit=ksplit, defect=defect)
    assert not Y[p:].any() and not Y[:, ld - 5:].any()
    return oref.check(Y, Yref, B, p) + (g,)


@pytest.mark.parametrize("name,ld,ksplit", [("syn32", 32, 1), ("mid", 32, 1), ("mid", 64, 1), ("mid", 256, 1), ("mid", 64, 3), ("mid", 64, 5)])
def test_emulated_sweep_is_within_the_bound(golden, name, ld, ksplit):
    KA, D, alpha = _case(name, golden)
    if name == "syn32":
        ksplit = 1
    ratio, ok, g = _run(KA, D, alpha, ld, ksplit)
    print("%s ld %d ksplit %d: gamma 2^%.2f, worst |Y - Yref| / bound %.3f" % (name, ld, ksplit, np.log2(g), ratio))
    assert g < 2.0 ** -16
    assert ok, ratio


@pytest.mark.parametrize("name", ["syn32", "mid"])
@pytest.mark.parametrize("defect", ["drop_lo_hi", "last_tile_scale", "neighbour_degree"])
def test_one_defect_at_a_time_breaks_the_bound(golden, name, defect):
    KA, D, alpha = _case(name, golden)
    kw = dict(wrong_degree_row=D.size // 2) if defect == "neighbour_degree" else dict(defect=defect)
    for ksplit in ((1,) if name == "syn32" else (1, 3)):
        ratio, ok, g = _run(KA, D, alpha, 64, ksplit, **kw)
        print("%s %s ksplit %d: worst |Y - Yref| / bound %.1f" % (name, defect, ksplit, ratio))
        assert not ok and ratio > 1.0, ratio


# (form, shape) pairs of the GPU tests whose gamma is not below 2^-16, with the reason; nothing else may exceed it
LONG_CHAINS = {
    ("f32", "slabs"): "k_block_matvec is one chain of p64 / 2 = 704 MFMAs per output (it has no K split): 705 2^-24 = 2^-14.5",
    ("band", "slabs"): "k_band generates the entries, so one output's chain is every (grid row, 16-column block) of the band: "
                       "30 x 3 k-steps x 3 MFMAs = 270 links, 2^-15.7; the image is smaller than the radius, the band is the whole grid",
}


def test_counts_of_every_form_at_the_gpu_shapes():
    """s and gamma per form at the shapes tests/test_gpu_operator.py runs them at (p, nr, nc as realised; the stored split-f16 form
    with the K slabs an MI355X takes: 1, and 8 at slabs; the other pixel formats on tiny and mid only). s <= 8 and gamma < 2^-16
    hold everywhere except where named: the rank form has s = 9 (three GEMMs, both operands split in each), and the two chains of
    LONG_CHAINS. Every gamma stays a factor 6 under a lost lo product's 2^-11."""
    shapes = {"tiny": (24, 4, 6), "edge128": (132, 11, 12), "mid": (320, 10, 32), "slabs": (1350, 30, 45)}
    seen_long = set()
    for name, (p, nr, nc) in shapes.items():
        assert nr * nc == p
        forms = [("f32", {}), ("f16s", dict(ksplit=8 if name == "slabs" else 1)), ("grid", dict(nr=nr, nc=nc)), ("rank", dict(nr=nr, nc=nc)),
                 ("band", dict(nr=nr, nc=nc))] + ([("pix_band", dict(nr=nr, nc=nc))] if name in ("tiny", "mid") else [])
        for form, kw in forms:
            K, s, c = oref.counts(form, p, **kw)
            g = oref.gamma(form, p, **kw)
            print("%-8s %-8s %-12s K %4d s %d c %3d gamma 2^%.2f" % (name, form, kw.get("ksplit", ""), K, s, c, np.log2(g)))
            assert s == 9 if form == "rank" else s <= 8, (form, s)
            assert g < 2.0 ** -11 / 6
            if (form, name) in LONG_CHAINS:
                assert g >= 2.0 ** -16
                seen_long.add((form, name))
            else:
                assert g < 2.0 ** -16, (name, form, g)
    assert seen_long == set(LONG_CHAINS)
