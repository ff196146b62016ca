"""The Jacobi-preconditioned block PCG of the eigen-solve (csrc/eigen.hip: block_pcg_work and the k_cg_* kernels) in plain numpy: the
recurrences in float64, the same with every stored vector rounded to f32 where the kernels round, a bound on how far the recurrence
residual R may drift from B - A X, and the right-hand sides of tests/test_pcg_ref.py (CPU) and tests/test_gpu_pcg.py.

The solve, per column j of the block (columns never mix: every scalar below is per column):
    z = d b, r = b, p = z, x = 0, rz = r.z, bn2 = b.b; active = j < m and bn2 > 0                    k_cg_init, k_cg_init_scalars
    step k = 1, 2, ... on the active columns:
        alpha = rz / p.Ap                                                                            k_cg_dot, k_cg_alpha
        x += alpha p, r -= alpha Ap                                                                  k_cg_update
        r.r <= rtol^2 bn2: the column leaves (its count is k); else beta = r.(d r) / rz, rz = r.(d r)  k_cg_beta
        p = d r + beta p                                                                             k_cg_pupdate
d = 1 / diag(A) as an f32 vector (k_dinv_from_degree: 1.0f / (float)(alpha (D_i - 1))).

Where the kernels round (csrc/eigen.hip, line numbers as of this commit), and pcg_f32 with them:
    :642      z = d * b                        one f32 product
    :646-647  r.z, b.b                         float64 sums of float64 products of the f32 values
    :692      p.Ap                             the same
    :706      alpha = rz / pap                 float64; :718 cast to f32 once, the same value for both updates
    :726      x = fmaf(alpha, p, x)            one rounding
    :727      r = fmaf(-alpha, Ap, r)          one rounding
    :729-730  r.r and r.(d r)                  d * r one f32 product (:730), the sums float64
    :749      r.r <= rtol^2 bn2                float64
    :753      beta = rz_new / rz_old           float64; :772 cast to f32
    :792      p = fmaf(beta, p, d * r)         d * r one f32 product, then one rounding
The product A p is taken in float64 and rounded to f32 once: the emulation stands for the recurrences, not for a sweep (the sweeps
have tests/operator_ref.py). An fmaf is emulated as the float64 expression rounded to f32: the product of two f32 values is exact in
float64, the sum is rounded to 53 bits before it is rounded to 24, which differs from one rounding only on near-ties.

drift_bound is a MODEL, not a theorem about the device: see its docstring."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126       # the smallest normal f32

DEFECTS = ("r_next_alpha", "stale_rz", "bn2_col0")


class Trajectory:
    """What one solve went through. count[j]: the steps column j took (0: never active; max_it where it was cut); active0[j]: it
    was active at the start; unconverged[j]: still active at exit; alpha[k], P[k]: alpha_k (length ld) and the block p_k the step
    k + 1 used; X[k], R[k]: the blocks after that step; stepped[k][j]: column j took that step. X[-1] and R[-1] are the result
    (all-zero X and R = B where no step was taken: X_final, R_final hold them in every case)."""

    def __init__(self):
        self.alpha, self.P, self.X, self.R, self.stepped, self.nactive = [], [], [], [], [], []


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _pcg(A, dinv, B, m, rtol, max_it, f32, defect=None):
    A = np.asarray(A, dtype=np.float64)
    p, ld = A.shape[0], B.shape[1]
    rnd = _f32 if f32 else (lambda a: a)
    d = np.asarray(dinv, dtype=np.float32).astype(np.float64)[:, None]
    b = np.asarray(B[:p], dtype=np.float32).astype(np.float64)
    z = rnd(d * b)                                               # :642
    R, P, X = b.copy(), z.copy(), np.zeros_like(b)               # :643-645
    rz, bn2 = (b * z).sum(axis=0), (b * b).sum(axis=0)           # :646-647
    active = (np.arange(ld) < m) & (bn2 > 0.0)                   # :665
    t = Trajectory()
    t.active0 = active.copy()
    t.count = np.zeros(ld, dtype=int)
    t.bn2 = bn2
    rtol2 = rtol * rtol
    it = 0
    t.nactive.append(int(active.sum()))
    while active.any() and it < max_it:
        it += 1
        a = np.flatnonzero(active)
        AP = np.zeros_like(P)
        AP[:, a] = rnd(A @ P[:, a])                              # the sweep: float64, rounded once
        pap = (P * AP).sum(axis=0)                               # :692
        alpha = np.zeros(ld)
        alpha[a] = rz[a] / pap[a]                                # :706
        alpha = rnd(alpha)                                       # :718
        alpha_r = np.roll(alpha, -1) if defect == "r_next_alpha" else alpha
        t.alpha.append(alpha.copy())
        t.P.append(P.copy())
        t.stepped.append(active.copy())
        X[:, a] = rnd(alpha[a] * P[:, a] + X[:, a])              # :726
        R[:, a] = rnd(-alpha_r[a] * AP[:, a] + R[:, a])          # :727
        rr = (R * R).sum(axis=0)                                 # :729
        rz_new = (R * rnd(d * R)).sum(axis=0)                    # :730
        ref = bn2[0] if defect == "bn2_col0" else bn2
        done = active & (rr <= rtol2 * ref)                      # :749
        t.count[active] = it
        cont = active & ~done
        beta = np.zeros(ld)
        beta[cont] = rz_new[cont] / rz[cont]                     # :753
        if defect != "stale_rz":
            rz[cont] = rz_new[cont]                              # :754
        active = cont
        beta = rnd(beta)                                         # :772
        c = np.flatnonzero(active)
        P[:, c] = rnd(beta[c] * P[:, c] + rnd(d * R[:, c]))      # :792
        t.X.append(X.copy())
        t.R.append(R.copy())
        t.nactive.append(int(active.sum()))
    t.iters = it
    t.unconverged = active.copy()
    t.X_final, t.R_final = X, R
    return t


def pcg64(A, dinv, B, m, rtol=1e-5, max_it=1000):
    """The recurrences in float64 (B and dinv: their f32 values widened). A: float64 [p, p]; B: [rows >= p, ld]. -> Trajectory."""
    return _pcg(A, dinv, B, m, rtol, max_it, False)


def pcg_f32(A, dinv, B, m, rtol=1e-5, max_it=1000, defect=None):
    """The same with the kernels' roundings (the table above). defect: None, or one of DEFECTS seeded into the recurrences --
    "r_next_alpha": R updated with the next column's alpha (X with its own); "stale_rz": rz is never replaced, so that every beta
    and every later alpha divide by the first; "bn2_col0": the stopping rule tested against column 0's b.b."""
    assert defect is None or defect in DEFECTS
    return _pcg(A, dinv, B, m, rtol, max_it, True, defect)


def drift_bound(traj, absL, op_bound=None):
    """A componentwise bound [p, ld] on |(B - A X) - R| after the solve of `traj` (a pcg_f32 trajectory: the magnitudes come from
    it). With t = b - A x the true residual, one step changes t - r by  alpha delta - A e_x - e_r:  delta the error of the sweep
    A p, e_x and e_r the roundings of the two fmaf. Summed over the steps k the column took:
        |alpha_k| op_bound(p_k)                      the sweep: operator_ref.bound of the form on the operand p_k (None: left out)
      + 2^-24 (|r_k+1| + (|L| |x_k+1|))              the two fmaf roundings
      + 2^-24 |alpha_k| (|L| |p_k|)                  the cast of alpha to f32 (it also covers a sweep rounded once: pcg_f32's)
      + 2^-126 (1 + |alpha_k| + sum_l |L_il|)        each of those roundings where its result lies below the normal f32 range (a unit
                                                     vector's A p holds kernel values down to 1e-47): lost, or flushed to zero
    and the whole doubled, because the device's trajectory is not the emulation's: its sweeps err differently, so its alpha_k,
    p_k, x_k and r_k differ from these by a relative O(gamma), and the magnitudes are taken from here. This is a model: the
    factor 2 is not derived. op_bound: callable P (float64 [p, ld]) -> [p, ld]."""
    absL = np.asarray(absL, dtype=np.float64)
    tot = np.zeros_like(traj.X_final)
    for k in range(len(traj.alpha)):
        s = traj.stepped[k]
        al, aP = np.abs(traj.alpha[k])[None, :], np.abs(traj.P[k])
        step = U * (np.abs(traj.R[k]) + absL @ np.abs(traj.X[k])) + U * al * (absL @ aP)
        step = step + TINY * (1.0 + al + absL.sum(axis=1)[:, None])
        if op_bound is not None:
            step = step + al * op_bound(traj.P[k])
        tot[:, s] += step[:, s]
    return 2.0 * tot


def drift(A, B, X, R, p):
    """|(B - A X) - R| in float64 of the f32 values, rows < p."""
    f8 = np.float64
    return np.abs(B[:p].astype(f8) - np.asarray(A, dtype=f8) @ X[:p].astype(f8) - R[:p].astype(f8))


# ---- right-hand sides ------------------------------------------------------------------------------------------------------------

def round_up(x, k):
    return (x + k - 1) // k * k


class Rhs:
    """B: float32 [round_up(p, 64), ld], columns m .. ld - 1 zero. kind[j]: "eig1" .. "eig4" (designed: a combination of that many
    eigenvectors of the preconditioned operator), "general", "scaled-" / "scaled+" (the column before it times 2^-30 / 2^+30),
    "unit", "zero", "halfzero", "pad". base[j]: for a scaled column the index of the column it scales, else -1."""


def eigenbasis(A, dinv):
    """Eigenvalues (ascending) and M^(1/2) V of M^(-1/2) A M^(-1/2), M = diag(1 / dinv): b = M^(1/2) V c lies in the invariant
    subspace of the pencil (A, M) spanned by the columns where c is not zero, and the PCG ends in as many steps as those
    columns have distinct eigenvalues."""
    s = np.sqrt(np.asarray(dinv, dtype=np.float32).astype(np.float64))
    lam, V = np.linalg.eigh(s[:, None] * np.asarray(A, dtype=np.float64) * s[None, :])
    return lam, V / s[:, None]


def spread(lam, d, shift):
    """d indices into the ascending spectrum with eigenvalues as far apart as it allows: the two ends, then the eigenvalue farthest
    from those chosen, again and again. d = 1: any one (`shift` moves along the spectrum)."""
    n = lam.size
    if d == 1:
        return [(shift * 7) % n]
    idx = [0, n - 1]
    while len(idx) < d:
        gap = np.min(np.abs(lam[:, None] - lam[idx][None, :]), axis=1)
        idx.append(int(np.argmax(gap)))
    assert len(set(idx)) == d, idx
    return sorted(idx)


STAIRCASE_AFTER = (160, 100, 48, 20)     # active columns after the steps 1 .. 4 of the staircase: the sweeps of the steps 2 .. 5 are 192, 128, 64, 32 wide


def make_rhs(A, dinv, p, ld, m, seed=0, rtol=1e-5, staircase=False):
    """The right-hand sides of one (p, ld, m) from the float64 operator A [p, p] and the f32 preconditioner dinv. Column layout, in
    order: the designed groups (dimension 1, 2, 3, 4: as many of each), then all-zero, a unit vector, zero on the even samples, a
    general column with its 2^-30 and its 2^+30 multiple, a dimension-2 column with its two multiples, and general random columns
    up to m. staircase (ld 256, a spectrum wide enough for a column of dimension 5 to take 5 steps): no general filler; the groups
    of dimension 1 .. 5 are sized, given the counts of the fixed columns, so that STAIRCASE_AFTER columns are active after the
    steps 1 .. 4. A column whose count is not robust (counts_robust) is drawn again, up to 20 times -- other weights on the same
    eigenvectors (up to 2^+-attempt), another position of the unit vector, another random draw: the column changes, never the rule."""
    rng = np.random.default_rng(1000 * seed + 7 * ld + m)
    lam, MV = eigenbasis(A, dinv)
    rows = round_up(p, 64)

    def designed(dim, k):
        def draw(attempt):
            c = (1.0 + 0.25 * rng.random(dim)) * 2.0 ** rng.uniform(-attempt, attempt, dim) * rng.choice([-1.0, 1.0], dim)
            v = MV[:, spread(lam, dim, k)] @ c
            return v / np.abs(v).max()
        return draw

    def general(mask=None):
        def draw(attempt):
            v = rng.normal(size=p)
            if mask is not None:
                v[mask] = 0.0
            return v
        return draw

    def unit(attempt):
        e = np.zeros(p)
        e[(p // 2 + attempt) % p] = 1.0
        return e

    def robust_columns(draws, want=None):
        """One column per draw function, each drawn again until its count is robust (and, where want[j] > 0, equal to it)
        -> (columns, counts)."""
        vs = [d(0) for d in draws]
        for attempt in range(1, 21):
            Bt = np.zeros((rows, round_up(len(vs), 32)), dtype=np.float32)
            Bt[:p, :len(vs)] = np.stack(vs, axis=1)
            cnt, ok = counts_robust(A, dinv, Bt, len(vs), rtol)
            ok = ok[:len(vs)] if want is None else ok[:len(vs)] & ((np.asarray(want) <= 0) | (cnt[:len(vs)] == np.asarray(want)))
            bad = np.flatnonzero(~ok)
            if bad.size == 0:
                return vs, cnt[:len(vs)]
            for j in bad:
                vs[j] = draws[j](attempt)
        raise AssertionError("columns %s have no robust count after 20 draws" % list(bad))

    (e, h, g, d2), cf = robust_columns([unit, general(np.arange(p) % 2 == 0), general(), designed(2, 1)])
    fixed = [(np.zeros(p), "zero", None), (e, "unit", None), (h, "halfzero", None),
             (g, "general", None), (g * 2.0 ** -30, "scaled-", -1), (g * 2.0 ** 30, "scaled+", -2),
             (d2, "eig2", None), (d2 * 2.0 ** -30, "scaled-", -1), (d2 * 2.0 ** 30, "scaled+", -2)]
    if staircase:
        assert ld == 256
        cf = np.r_[cf[0], cf[1], [cf[2]] * 3, [cf[3]] * 3]    # the counts of the non-zero fixed columns
        after = (m - 1,) + STAIRCASE_AFTER + (0,)             # every column but the all-zero one starts active
        groups = [(s, after[s - 1] - after[s] - int(((cf == s) if s < 5 else (cf >= 5)).sum())) for s in (1, 2, 3, 4, 5)]
        assert all(n >= 1 for _, n in groups), groups
    else:
        n = max(1, (m - len(fixed) - 3) // 4)
        groups = [(1, n), (2, n), (3, n), (4, n)]
    draws = [designed(dim, k) for dim, n in groups for k in range(n)]
    kinds = ["eig%d" % dim for dim, n in groups for k in range(n)]
    nfill = m - len(draws) - len(fixed)
    assert nfill >= 0, (m, len(draws))
    want = [dim for dim, n in groups for k in range(n)] + [0] * nfill if staircase else None    # the staircase needs the exact counts
    vs, _ = robust_columns(draws + [general()] * nfill, want)
    cols, base = vs[:len(draws)], [-1] * len(draws)
    for v, kind, rel in fixed:
        base.append(-1 if rel is None else len(cols) + rel)
        cols.append(v)
        kinds.append(kind)
    cols += vs[len(draws):]
    kinds += ["general"] * nfill
    base += [-1] * nfill
    r = Rhs()
    r.B = np.zeros((rows, ld), dtype=np.float32)
    r.B[:p, :m] = np.stack(cols, axis=1).astype(np.float32)
    for j, b in enumerate(base):      # a scaled column is the exact power-of-two multiple of the f32 column it scales
        if b >= 0:
            r.B[:, j] = r.B[:, b] * np.float32(2.0 ** (-30 if kinds[j] == "scaled-" else 30))
    r.kind = kinds + ["pad"] * (ld - m)
    r.base = base + [-1] * (ld - m)
    r.m, r.ld, r.p = m, ld, p
    return r


def counts_robust(A, dinv, B, m, rtol=1e-5, max_it=200):
    """(counts of pcg64 at rtol, robust[j]): a column's count is robust when pcg64 at 2 rtol, rtol and rtol / 2 and pcg_f32 at rtol
    all give it."""
    c = [pcg64(A, dinv, B, m, r, max_it).count for r in (2 * rtol, rtol, rtol / 2)] + [pcg_f32(A, dinv, B, m, rtol, max_it).count]
    c = np.stack(c)
    return c[1], (c == c[1][None, :]).all(axis=0)
