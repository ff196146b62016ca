"""The epilogue of glf_graph_softmax (include/glf.h, "softmax read-out") restated in numpy f32, and the error bounds of DESIGN.md
("Softmax read-out") as functions that the GPU tests import. No GPU.

  the kernel's way   a lane holds the 16 classes j = (g & 3) + 8 (g >> 2) + 4 h of half-wave h; per lane over g ascending for the
                     classes < k: best by a strict >, one exchange with the other half; d = score - best, t = beta2 d, e = 2^t,
                     S = S + e, A = fma(e, e > 0 ? t : 0, A), one exchange each; r = 1 / S, p = e r,
                     lse = fma(fl32(ln 2), log2 S, fl32(beta) best), entropy = fl32(ln 2) (log2 S - A r).
                     np.exp2 / np.log2 in f32 stand in for v_exp_f32 / v_log_f32 (both within an ulp of them; numpy keeps the
                     subnormal results that the hardware flushes, which the bounds' absolute terms cover).
  the bounds         against the exact softmax of the same f32 scores, u = 2^-24, t*_j = beta log2 e (score_j - best):
                     eps_j = 2 u + 3 ln 2 min(|t*_j|, 126) u     (v_exp_f32 at 1 ulp = 2 u, the project's constant; beta2, d and t carry
                                                                 3 u of relative error into the exponent; a class below 2^-126 is
                                                                 covered by the absolute term whatever its t)
                     eps_S = max_{t*_i >= -126} eps_i + 16 u      (15 additions in the lane, one across the halves)
                     |p - p*|     <= p* (eps_j + eps_S + 3 u) (1 + 2^-10) + 2^-126
                     |lse - lse*| <= (eps_S + 3 u ln S* + 2 u |beta best| + u |lse*|) (1 + 2^-10) + 2^-120
                     |H - H*|     <= (ln 2 sum_j p*_j |t*_j| (eps_j + eps_S + 22 u) + eps_S + 2 u ln S*
                                      + 3 u (ln S* + ln 2 sum_j p*_j |t*_j|)) (1 + 2^-10) + 2^-100

The restatement must stay within the bounds of an f64 softmax on random and adversarial score tables for every k from 1 to 32, and
the bounds must reject five seeded defects: the max not subtracted (scores around 100), beta applied twice, the sum taken over one
half-wave's 16 classes only, a slot >= k included, ln 2 missing from the entropy."""
import numpy as np
import pytest

U = 2.0 ** -24
LN2 = np.float32(np.log(2.0))
LOG2E = 1.4426950408889634074


def _fma(a, b, c):
    """fl32(a b + c) for f32 arrays (the product is exact in f64; the double rounding of the sum is far below the bounds)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_way(scores, k, beta, defect=None):
    """(p [n, k], lse [n], entropy [n]) of f32 score tables [n, 32] by the kernel's epilogue, classes < k."""
    s = np.asarray(scores, dtype=np.float32)
    n = s.shape[0]
    f = np.float32
    beta2 = f(beta * LOG2E)
    if defect == "beta twice":
        beta2 = f(beta2 * f(beta))
    kk = k + 1 if defect == "slot k included" and k < 32 else k
    lanes = [[j for j in ((g & 3) + 8 * (g >> 2) + 4 * h for g in range(16)) if j < kk] for h in (0, 1)]
    with np.errstate(all="ignore"):
        bests = []
        for h in (0, 1):
            b = np.full(n, -np.inf, dtype=f)
            for j in lanes[h]:
                b = np.where(s[:, j] > b, s[:, j], b)
            bests.append(b)
        best = np.where(bests[1] > bests[0], bests[1], bests[0])
        if defect == "max not subtracted":
            best = np.zeros(n, dtype=f)
        e = np.zeros((n, 32), dtype=f)
        S2, A2 = [], []
        for h in (0, 1):
            S, A = np.zeros(n, dtype=f), np.zeros(n, dtype=f)
            for j in lanes[h]:
                d = (s[:, j] - best).astype(f)
                t = (beta2 * d).astype(f)
                e[:, j] = np.exp2(t).astype(f)
                S = (S + e[:, j]).astype(f)
                A = _fma(e[:, j], np.where(e[:, j] > 0, t, f(0)).astype(f), A)
            S2.append(S)
            A2.append(A)
        S = S2[0] if defect == "one half-wave" else (S2[0] + S2[1]).astype(f)
        A = (A2[0] + A2[1]).astype(f)
        r = (f(1) / S).astype(f)
        p = (e[:, :k] * r[:, None]).astype(f)
        L = np.log2(S).astype(f)
        lse = _fma(np.full(n, LN2), L, (f(beta) * best).astype(f))
        x = (L - (A * r).astype(f)).astype(f)
        ent = x if defect == "no ln 2" else (LN2 * x).astype(f)
    return p, lse, ent


def exact(scores, beta):
    """The f64 softmax of scores [k, ...] along axis 0 -> dict(p, lse, entropy, t: t*_j, lnS, w: sum_j p*_j |t*_j|, best)."""
    z = np.asarray(scores, dtype=np.float64)
    best = z.max(axis=0)
    t = beta * LOG2E * (z - best)
    e = np.exp2(t)
    S = e.sum(axis=0)
    p = e / S
    w = np.where(p > 0, p * np.abs(np.where(p > 0, t, 0.0)), 0.0).sum(axis=0)
    lnS = np.log(S)
    return dict(p=p, lse=beta * best + lnS, entropy=lnS + np.log(2.0) * w, t=t, lnS=lnS, w=w, best=best, beta=beta)


def bounds(x):
    """(bound on |p - p*| [k, ...], on |lse - lse*|, on |entropy - entropy*|) for exact()'s dict, by the module text."""
    at = np.minimum(np.abs(x["t"]), 126.0)
    eps = 2 * U + 3 * np.log(2.0) * at * U
    eps_s = np.where(x["t"] >= -126.0, eps, 0.0).max(axis=0) + 16 * U
    so = 1.0 + 2.0 ** -10
    bp = x["p"] * (eps + eps_s + 3 * U) * so + 2.0 ** -126
    blse = (eps_s + 3 * U * x["lnS"] + 2 * U * np.abs(x["beta"] * x["best"]) + U * np.abs(x["lse"])) * so + 2.0 ** -120
    wt = (x["p"] * at * (eps + eps_s + 22 * U)).sum(axis=0)
    bh = (np.log(2.0) * wt + eps_s + 2 * U * x["lnS"] + 3 * U * (x["lnS"] + np.log(2.0) * x["w"])) * so + 2.0 ** -100
    return bp, blse, bh


def fractions(p, lse, ent, x):
    """The largest |error| / bound of each output (numpy arrays, classes on axis 0 of p); a NaN counts as infinitely far out."""
    bp, blse, bh = bounds(x)
    out = []
    for got, want, b in ((p, x["p"], bp), (lse, x["lse"], blse), (ent, x["entropy"], bh)):
        if got is None:
            out.append(0.0)
            continue
        q = np.abs(np.asarray(got, dtype=np.float64) - want) / b
        out.append(float(np.where(np.isnan(q), np.inf, q).max()))
    return tuple(out)


def _tables():
    """Score tables [pixels, 32] of finite f32 scores: of order one, wide (classes far below the best), near-ties, and large common
    offsets."""
    rng = np.random.default_rng(8)
    smooth = rng.normal(size=(200, 32))
    wide = 30.0 * rng.normal(size=(200, 32))
    ties = np.round(rng.normal(size=(100, 32)) * 2) / 2
    offset = smooth[:100] + 100.0 * rng.normal(size=(100, 1))
    far = smooth[:50].copy()
    far[:, ::3] = -1e30                                                      # classes that underflow to e = +0
    far[:, 1] = 0.0
    return np.concatenate([smooth, wide, ties, offset, far]).astype(np.float32)


TABLES = _tables()
BETAS = (0.25, 1.0, 8.0)


@pytest.mark.parametrize("k", range(1, 33))
def test_the_restatement_is_within_the_bounds(k):
    worst = [0.0, 0.0, 0.0]
    for beta in BETAS:
        p, lse, ent = kernel_way(TABLES, k, beta)
        x = exact(TABLES[:, :k].T, beta)
        fr = fractions(p.T, lse, ent, x)
        worst = [max(a, b) for a, b in zip(worst, fr)]
        assert np.all(p >= 0) and np.all(p <= 1)
        assert abs(p.astype(np.float64).sum(axis=1) - 1.0).max() <= bounds(x)[0].sum(axis=0).max() + k * U
    print("k %d: largest error / bound: p %.3f lse %.3f entropy %.3f" % (k, *worst))
    assert max(worst) <= 1.0, (k, worst)
    if k == 1:
        p, lse, ent = kernel_way(TABLES, 1, 8.0)
        assert np.all(p == 1) and not ent.view(np.uint32).any()
        np.testing.assert_array_equal(lse, np.float32(8.0) * TABLES[:, 0] + np.float32(0.0))


def test_special_values():
    f = np.float32
    row = np.zeros((5, 32), dtype=f)
    row[0, :4] = [1.0, -np.inf, 2.0, 0.5]                                    # -inf beside finite scores: p = +0 exactly
    row[1, :4] = [1.0, np.nan, 2.0, 0.5]
    row[2, :4] = [1.0, np.inf, 2.0, 0.5]
    row[3, :4] = -np.inf
    row[4, :4] = [1.0, -1e30, 2.0, 0.5]
    p, lse, ent = kernel_way(row, 4, 1.0)
    assert p[0, 1] == 0 and not np.signbit(p[0, 1]) and np.isfinite(p[0]).all() and np.isfinite(lse[0]) and np.isfinite(ent[0])
    for i in (1, 2, 3):
        assert np.isnan(p[i]).all() and np.isnan(lse[i]) and np.isnan(ent[i]), i
    p3, lse3, ent3 = kernel_way(row[[0, 4]][:, [0, 2, 3] + list(range(4, 32)) + [1]], 3, 1.0)   # the same pixels without class 1
    for i in (0, 1):
        np.testing.assert_array_equal(p[[0, 4]][i, [0, 2, 3]].view(np.uint32), p3[i].view(np.uint32))
    np.testing.assert_array_equal(lse[[0, 4]].view(np.uint32), lse3.view(np.uint32))
    np.testing.assert_array_equal(ent[[0, 4]].view(np.uint32), ent3.view(np.uint32))


@pytest.mark.parametrize("defect", ["max not subtracted", "beta twice", "one half-wave", "slot k included", "no ln 2"])
def test_a_seeded_defect_is_rejected(defect):
    rng = np.random.default_rng(31)
    tables = rng.normal(size=(200, 32)).astype(np.float32)
    if defect == "max not subtracted":
        tables = (tables + np.float32(100.0)).astype(np.float32)
    for k, beta in ((5, 8.0), (12, 0.25), (31, 8.0)):
        x = exact(tables[:, :k].T, beta)
        good = fractions(*_t(kernel_way(tables, k, beta)), x)
        bad = fractions(*_t(kernel_way(tables, k, beta, defect)), x)
        print("%s, k %d beta %g: error / bound %s against %s without the defect" % (defect, k, beta, bad, good))
        assert max(good) <= 1.0
        assert max(bad) > 1.0, (defect, k, beta, bad)


def _t(out):
    return out[0].T, out[1], out[2]
