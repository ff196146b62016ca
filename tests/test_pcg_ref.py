"""The float64 reference of the block PCG (tests/pcg_ref.py) and the right-hand sides of tests/test_gpu_pcg.py (tests/pcg_cases.py)
meet the conditions the GPU test relies on. CPU only.

  * every non-zero column's count is robust: pcg64 at 2 rtol, rtol and rtol / 2 and pcg_f32 at rtol agree on it; a column of
    dimension d takes at most d steps, exactly d where the spectrum is wide enough (dense70); a column times 2^+-30 takes what its
    base takes; the all-zero column takes none;
  * the staircase at ld 256 has 160, 100, 48 and 20 columns active after the steps 1 .. 4, so that the packed sweeps of the steps
    2 .. 5 are 192, 128, 64 and 32 columns wide (block_pcg_work's rule: 32 up to 32 active columns, else a multiple of 64);
  * pcg_f32 stays inside drift_bound with the operator term left out, whole solves and solves cut at 1 and 2 steps;
  * three defects seeded into pcg_f32, one at a time, are each rejected by the drift check or the count check."""
import numpy as np
import pytest

import pcg_cases as pc
import pcg_ref as pr

RTOL = pc.RTOL


def _ids(cases):
    return ["%s-%d-%d" % c for c in cases]


@pytest.mark.parametrize("name,ld,m", pc.CASES, ids=_ids(pc.CASES))
def test_counts_are_robust(name, ld, m):
    c, r = pc.shape(name), pc.rhs(name, ld, m)
    assert r.B.shape == (pr.round_up(c.p, 64), ld) and not r.B[c.p:].any() and not r.B[:, m:].any()
    count, robust = pr.counts_robust(c.A, c.dinv, r.B, m, RTOL)
    kind = np.array(r.kind)
    seen = set(kind[:m])
    assert {"eig1", "eig2", "eig3", "eig4", "general", "scaled-", "scaled+", "unit", "zero", "halfzero"} <= seen, seen
    for j in range(ld):
        k = kind[j]
        if k in ("zero", "pad"):
            assert count[j] == 0 and not r.B[:, j].any()
            continue
        assert robust[j], "column %d (%s) of %s: no robust count" % (j, k, (name, ld, m))
        assert count[j] >= 1
        if k.startswith("eig"):
            d = int(k[3:])
            assert count[j] <= d and (count[j] == d or (name != "dense70" and d > 2)), (j, k, count[j])
        if k.startswith("scaled"):
            b = r.base[j]
            assert count[j] == count[b]
            np.testing.assert_array_equal(r.B[:, j], r.B[:, b] * np.float32(2.0 ** (30 if k == "scaled+" else -30)))
    if name == "dense70":
        assert count[kind == "general"].min() >= 4, "a general column of the densely sampled shape takes at least 4 steps"
        lam = pr.eigenbasis(c.A, c.dinv)[0]
        assert 1.3 < lam[-1] / lam[0] < 1.4
    assert not r.B[0:c.p:2, list(kind).index("halfzero")].any()
    u = r.B[:, list(kind).index("unit")]
    assert np.count_nonzero(u) == 1 and u.max() == 1.0


def test_the_staircase_passes_through_every_narrow_width():
    name, ld, m = pc.STAIRCASE
    c, r = pc.shape(name), pc.rhs(name, ld, m)
    for t in (pr.pcg64(c.A, c.dinv, r.B, m, RTOL), pr.pcg_f32(c.A, c.dinv, r.B, m, RTOL)):
        assert t.nactive[:5] == [m - 1] + list(pr.STAIRCASE_AFTER), t.nactive
        assert t.nactive[5] == 0 and t.iters == 5
        widths = [ld] + [32 if na <= 32 else pr.round_up(na, 64) for na in t.nactive[1:t.iters]]   # the sweep of step k + 1 is sized by the count after step k
        assert widths == [256, 192, 128, 64, 32]


def _worst(d, bound, m):
    pos = bound[:, :m] > 0
    assert (d[:, :m][~pos] == 0).all()
    return float((d[:, :m][pos] / bound[:, :m][pos]).max())


@pytest.mark.parametrize("name,ld,m", pc.CASES, ids=_ids(pc.CASES))
def test_the_emulation_stays_inside_the_drift_bound(name, ld, m):
    c, r = pc.shape(name), pc.rhs(name, ld, m)
    absL = np.abs(c.A)
    for max_it in (1, 2, 1000):
        t = pr.pcg_f32(c.A, c.dinv, r.B, m, RTOL, max_it)
        X, R = t.X_final.astype(np.float32), t.R_final.astype(np.float32)
        assert (X == t.X_final).all() and (R == t.R_final).all()        # the stored vectors are f32 values
        d = pr.drift(c.A, r.B, X, R, c.p)
        bound = pr.drift_bound(t, absL)
        ratio = _worst(d, bound, m)
        print("%s ld %d m %d max_it %d: worst drift / bound %.3f, %d steps" % (name, ld, m, max_it, ratio, t.iters))
        assert ratio <= 1.0
        assert t.iters <= max_it
        zero = list(r.kind).index("zero")
        assert not X[:, zero].any() and not X[:, m:].any()


@pytest.mark.parametrize("defect", pr.DEFECTS)
@pytest.mark.parametrize("name,ld,m", [("dense70", 64, 59), pc.STAIRCASE, ("slabs", 32, 27)], ids=_ids([("dense70", 64, 59), pc.STAIRCASE, ("slabs", 32, 27)]))
def test_seeded_defects_are_rejected(name, ld, m, defect):
    """What the GPU test does with the device's X, R and counts, done to a pcg_f32 with one defect: the drift against the bound of
    the clean emulation's trajectory, the counts against pcg64's. Each defect fails the check named here."""
    c, r = pc.shape(name), pc.rhs(name, ld, m)
    ref = pr.pcg64(c.A, c.dinv, r.B, m, RTOL)
    clean = pr.pcg_f32(c.A, c.dinv, r.B, m, RTOL)
    bound = pr.drift_bound(clean, np.abs(c.A))
    with np.errstate(all="ignore"):        # a defective recurrence may diverge; it is cut three steps after the reference's last
        bad = pr.pcg_f32(c.A, c.dinv, r.B, m, RTOL, max_it=ref.iters + 3, defect=defect)
        d = pr.drift(c.A, r.B, bad.X_final.astype(np.float32), bad.R_final.astype(np.float32), c.p)
    ratio = _worst(np.where(np.isfinite(d), d, np.inf), bound, m)
    wrong = int((bad.count[:m] != ref.count[:m]).sum())
    print("%s on %s ld %d: worst drift / bound %.3g, %d of %d counts differ" % (defect, name, ld, ratio, wrong, m))
    assert (clean.count == ref.count).all() and _worst(pr.drift(c.A, r.B, clean.X_final.astype(np.float32), clean.R_final.astype(np.float32), c.p), bound, m) <= 1.0
    if defect == "r_next_alpha":
        assert ratio > 100.0           # R is no residual of X any more: orders of magnitude, not a rounding
    else:
        assert wrong >= 1
        kind = np.array(r.kind[:m])
        if defect == "bn2_col0":       # the columns 2^+-30 away from column 0 stop at the wrong step
            assert (bad.count[:m][kind == "scaled-"] != ref.count[:m][kind == "scaled-"]).any() or \
                   (bad.count[:m][kind == "scaled+"] != ref.count[:m][kind == "scaled+"]).any()
